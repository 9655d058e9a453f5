#!/usr/bin/env python3
"""A list of windows of the 8192^2 mirror tile (config 3) in one launch (mh_decode_windows) against
what a caller did before it, with one prepared table:

  (a) one mh_decode_windows launch for the N windows, window p into slot p;
  (b) N mh_decode_region launches, one per window, each into its slot -- what a caller does on the
      parent -- all inside the clocked region;
  (c) one full-frame mh_decode into a W x H raster, then N device copies of the windows out of it.

Windows of 256 x 256 pixels (32 x 32 blocks) at seeded random block positions, N = 1, 16, 64 and
256, and one row of 64 windows of 1024 x 768 (128 x 96 blocks). At N = 1 (a) against (b) is the
windows kernel against mh_decode_region on the same window: the cost of the descriptor trip.
scripts/bench_region.py's frame and method: two resident 8192^2 frames of one table (the mirror tile
and a block shuffle of it) alternate region by region; every region is cold -- a 1 GiB device copy
evicts the Infinity Cache and the L2s first (bench.FLUSH), off the clock -- the launches of a region
are enqueued behind bench.py's launch gate between two HIP events, the figure is the events'
distance, the routes alternate region by region, and the table gives the median (min .. max) over
the timed regions. Every route's output is compared with the encoder's input before timing.

    python scripts/bench_windows.py [--out profiles/windows_decode_ab.txt] [--regions 15]

runs the step as a child process under its own `timeout` and writes what it printed to --out.
`--step lists` runs it here.
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
STEPS = {"lists": 540}  # step -> its time limit, seconds


def step_lists(regions):
    import numpy as np
    import torch
    from bench_region import _fmt, _setup, _timed
    from metalhuffman_amd import decoder as D
    dev, tabs, sets = _setup()
    full = torch.empty((1, SIDE, SIDE), dtype=torch.uint8, device=dev)
    gw = SIDE // 8
    print(f"[lists] N windows of one {SIDE}x{SIDE} mirror-tile frame at seeded random block positions, one prepared "
          f"table, cold regions, HIP events, median (min .. max) us over {regions} regions")
    print(f"  {'window':<10} {'N':>4} {'size (blocks)':<14} {'grid':>9}   {'(a) mh_decode_windows':<34} "
          f"{'(b) N x mh_decode_region':<34} {'(c) mh_decode + N copies':<34} (a)/(b)  (a)/(c)")
    rows = []
    rng = np.random.default_rng(SEED)
    for (w, h), n in ROWS:
        bw, bh = w // 8, h // 8
        pos = np.stack([np.zeros(n, np.int64), rng.integers(0, gw - bw + 1, n), rng.integers(0, gw - bh + 1, n)],
                       axis=1)
        wins = torch.from_numpy(np.concatenate([pos, np.zeros((n, 1), np.int64)], axis=1).astype(np.int32)).to(dev)
        regs = [D.Region(int(p[1]), int(p[2]), bw, bh) for p in pos]
        out_a = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        out_b = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        out_c = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
        slots_b = [out_b[p:p + 1] for p in range(n)]

        def route_a(s):
            D.decode_windows(s["fr"], tabs, wins, (bw, bh), out=out_a)

        def route_b(s):
            for p in range(n):
                D.decode_region(s["fr"], tabs, regs[p], out=slots_b[p])

        def route_c(s):
            D.decode(s["fr"], tabs, out=full)
            for p in range(n):
                r = regs[p]
                out_c[p].copy_(full[0, 8 * r.by0: 8 * r.by0 + h, 8 * r.bx0: 8 * r.bx0 + w])

        for s in sets:  # parity first (and the warm-up of every kernel)
            want = torch.stack([s["ref"][8 * r.by0: 8 * r.by0 + h, 8 * r.bx0: 8 * r.bx0 + w] for r in regs])
            for out, fn, name in ((out_a, route_a, "a"), (out_b, route_b, "b"), (out_c, route_c, "c")):
                out.fill_(0xA5)
                fn(s)
                torch.cuda.synchronize(dev)
                if not torch.equal(out, want):
                    raise SystemExit(f"bench_windows: route ({name}) differs from the encoder's input ({n} x {w}x{h})")
        g, wv = D.decode_windows_shape(sets[0]["fr"], n, (bw, bh))
        res = _timed(dev, {"a": route_a, "b": route_b, "c": route_c}, sets, regions)
        ab = round(res["a"]["median_us"] / res["b"]["median_us"], 4)
        ac = round(res["a"]["median_us"] / res["c"]["median_us"], 4)
        rows.append({"window": [w, h], "n_windows": n, "size_blocks": [bw, bh], "positions": pos[:, 1:].tolist(),
                     "shape": {"groups_per_window": g, "waves_per_group": wv}, "routes": res, "a_over_b": ab,
                     "a_over_c": ac})
        print(f"  {f'{w}x{h}':<10} {n:>4} {f'{bw}x{bh}':<14} {f'{n}x{g}x{wv}':>9}   {_fmt(res['a']):<34} "
              f"{_fmt(res['b']):<34} {_fmt(res['c']):<34} {ab:.3f}    {ac:.3f}")
    print(json.dumps({"step": "lists", "device": torch.cuda.get_device_name(dev), "seed": SEED, "rows": rows}))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_decode_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        step_lists(args.regions)
        return 0
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_windows.py --regions {args.regions}   (library stamp {B.library_stamp()[:16]})\n"]
    for step in ("lists",):  # under its own time limit
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--regions", str(args.regions)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)  # (stderr passes through)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"bench_windows: step {step} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
        text.append(p.stdout)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
