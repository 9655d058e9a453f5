#!/usr/bin/env python3
"""A list of windows of the 8192^2 mirror tile (config 3) at 1/2, 1/4 and 1/8 scale in one launch
(mh_decode_windows_scaled) against what a caller did before it, with one prepared table:

  (a) one mh_decode_windows_scaled launch for the N windows, window p into slot p;
  (b) N mh_decode_region_scaled launches, one per window, each into its slot -- what a caller does
      on the parent -- all inside the clocked region;
  (c) one mh_decode_windows launch at full size, then one reduction pass over the N slots in torch
      (an integer reshape-sum, rounded and narrowed to bytes);
  (d) mh_decode_windows alone on the same windows: (c) without its second pass.

The claim checked is (a) < (b) by more than the +-4 % box-to-box spread at every row of N >= 16 (the
exit status says so); (a)/(b) at N = 1 -- the cost of the descriptor trip --, (a)/(c) and (a)/(d) are
reported. scripts/bench_windows.py's rows and method: windows of 256 x 256 pixels at seeded random
block positions, N = 1, 16, 64 and 256, and one row of 64 windows of 1024 x 768, each at k = 1, 2,
3; two resident 8192^2 frames of one table alternate region by region; every region is cold -- a
1 GiB device copy evicts the Infinity Cache and the L2s first (bench.FLUSH), off the clock -- the
launches of a region are enqueued behind bench.py's launch gate between two HIP events, the figure
is the events' distance, the routes alternate region by region, and the table gives the median
(min .. max) over the timed regions. Every route's output is compared with the box means of the
encoder's input before timing ((d) with the input itself).

    python scripts/bench_windows_scaled.py [--out profiles/windows_scaled_decode_ab.txt] [--regions 15]

runs one step per scale as a child process under its own `timeout` and writes what they printed to
--out. `--step k1|k2|k3` runs one here.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SIDE = 8192
ROWS = [((256, 256), 1), ((256, 256), 16), ((256, 256), 64), ((256, 256), 256), ((1024, 768), 64)]
SEED = 20261
SPREAD = 0.04                                     # the project's box-to-box spread
STEPS = {"k1": 500, "k2": 500, "k3": 500}         # step -> its time limit, seconds


def step_scale(k, regions):
    import numpy as np
    import torch
    from bench_region import _fmt, _setup, _timed
    from metalhuffman_amd import decoder as D
    dev, tabs, sets = _setup()
    s = 1 << k
    gw = SIDE // 8
    print(f"[k{k}] N windows of one {SIDE}x{SIDE} mirror-tile frame at 1/{s} scale, seeded random block positions, "
          f"one prepared table, cold regions, HIP events, median (min .. max) us over {regions} regions")
    print(f"  {'window':<10} {'N':>4} {'grid':>9}   {'(a) mh_decode_windows_scaled':<32} "
          f"{'(b) N x mh_decode_region_scaled':<32} {'(c) mh_decode_windows + reduce':<32} "
          f"{'(d) mh_decode_windows':<32} (a)/(b)  (a)/(c)  (a)/(d)")
    rows, ok = [], True
    rng = np.random.default_rng(SEED)
    for (w, h), n in ROWS:
        bw, bh = w // 8, h // 8
        pos = np.stack([np.zeros(n, np.int64), rng.integers(0, gw - bw + 1, n), rng.integers(0, gw - bh + 1, n)],
                       axis=1)
        wins = torch.from_numpy(np.concatenate([pos, np.zeros((n, 1), np.int64)], axis=1).astype(np.int32)).to(dev)
        regs = [D.Region(int(p[1]), int(p[2]), bw, bh) for p in pos]
        out_a = torch.empty((n, h // s, w // s), dtype=torch.uint8, device=dev)
        out_b = torch.empty_like(out_a)
        out_c = torch.empty_like(out_a)
        big = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        slots_b = [out_b[p:p + 1] for p in range(n)]

        def reduce_into(dst, src):
            acc = src.view(n, h // s, s, w // s, s).sum(dim=(2, 4), dtype=torch.int32)
            dst.copy_((acc + (s * s // 2)) >> (2 * k))

        def route_a(st):
            D.decode_windows_scaled(st["fr"], tabs, wins, (bw, bh), k, out=out_a)

        def route_b(st):
            for p in range(n):
                D.decode_region_scaled(st["fr"], tabs, regs[p], k, out=slots_b[p])

        def route_c(st):
            D.decode_windows(st["fr"], tabs, wins, (bw, bh), out=big)
            reduce_into(out_c, big)

        def route_d(st):
            D.decode_windows(st["fr"], tabs, wins, (bw, bh), out=big)

        for st in sets:  # parity first (and the warm-up of every kernel)
            full = torch.stack([st["ref"][8 * r.by0: 8 * r.by0 + h, 8 * r.bx0: 8 * r.bx0 + w] for r in regs])
            want = torch.empty_like(out_a)
            reduce_into(want, full)
            for out, exp, fn, name in ((out_a, want, route_a, "a"), (out_b, want, route_b, "b"),
                                       (out_c, want, route_c, "c"), (big, full, route_d, "d")):
                out.fill_(0xA5)
                big.fill_(0xA5)
                fn(st)
                torch.cuda.synchronize(dev)
                if not torch.equal(out, exp):
                    raise SystemExit(f"bench_windows_scaled: route ({name}) differs from the box means of the "
                                     f"encoder's input ({n} x {w}x{h}, k = {k})")
        g, wv = D.decode_windows_scaled_shape(sets[0]["fr"], n, (bw, bh), k)
        res = _timed(dev, {"a": route_a, "b": route_b, "c": route_c, "d": route_d}, sets, regions)
        ratio = {x: round(res["a"]["median_us"] / res[x]["median_us"], 4) for x in "bcd"}
        gated = n >= 16
        if gated and not ratio["b"] < 1.0 - SPREAD:
            ok = False
        rows.append({"window": [w, h], "n_windows": n, "log2_scale": k, "size_blocks": [bw, bh],
                     "positions": pos[:, 1:].tolist(), "shape": {"groups_per_window": g, "waves_per_group": wv},
                     "routes": res, "a_over_b": ratio["b"], "a_over_c": ratio["c"], "a_over_d": ratio["d"],
                     "gated": gated})
        print(f"  {f'{w}x{h}':<10} {n:>4} {f'{n}x{g}x{wv}':>9}   {_fmt(res['a']):<32} {_fmt(res['b']):<32} "
              f"{_fmt(res['c']):<32} {_fmt(res['d']):<32} {ratio['b']:.3f}    {ratio['c']:.3f}    {ratio['d']:.3f}")
    print(f"  (a) < (b) by more than {SPREAD:.0%} at every row of N >= 16: {'yes' if ok else 'NO'}")
    print(json.dumps({"step": f"k{k}", "device": torch.cuda.get_device_name(dev), "seed": SEED, "claim_holds": ok,
                      "rows": rows}))
    return ok


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_scaled_decode_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        return 0 if step_scale(int(args.step[1]), args.regions) else 3
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_windows_scaled.py --regions {args.regions}   "
            f"(library stamp {B.library_stamp()[:16]})\n"]
    claim = True
    for step in sorted(STEPS):  # each under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, "-u", os.path.abspath(__file__), "--step", step,
               "--regions", str(args.regions)]
        lines = []
        with subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True) as p:  # (stderr passes through)
            for line in p.stdout:  # row by row, as the step prints them
                sys.stdout.write(line)
                sys.stdout.flush()
                lines.append(line)
        if p.returncode not in (0, 3):
            print(f"bench_windows_scaled: step {step} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
        claim = claim and p.returncode == 0
        text.append("".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return 0 if claim else 3


if __name__ == "__main__":
    sys.exit(main())
