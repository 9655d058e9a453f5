#!/usr/bin/env python3
"""A list of crops at PIXEL origins of the 8192^2 mirror tile (config 3) in one launch
(mh_decode_crops) against what a caller did before it, with one prepared table:

  (a) one mh_decode_crops launch for the N crops, crop p dense in slot p;
  (b) what a caller did on the parent: decode_windows at windows_of_rects' block size (one block
      larger in each direction) into an oversized raster, plus ONE torch gather (advanced indexing
      with the per-crop (dx, dy)) into a dense [n, h, w] -- both inside the clocked region;
  (c) one mh_decode_windows launch of ceil(w / 8) x ceil(h / 8) blocks at the crops' block-aligned
      origins: the parent's kernel on the same blocks less the extra block row and column a
      non-aligned crop touches, and without the shift. It does not produce the crops; it is the
      yardstick for the output stage's cost.

Crops of 224 x 224 pixels at seeded random pixel origins, N = 1, 16, 64 and 256, and 64 crops of
1024 x 768. scripts/bench_region.py's frame and method, as scripts/bench_windows.py: two resident
8192^2 frames of one table alternate region by region; every region is cold -- a 1 GiB device copy
evicts the Infinity Cache and the L2s first (bench.FLUSH), off the clock -- the launches of a region
are enqueued behind bench.py's launch gate between two HIP events, the figure is the events'
distance, the routes alternate region by region, and the table gives the median (min .. max) over
the timed regions. Routes (a) and (b) are compared with the encoder's input before timing, (c) with
its own rectangles of it.

    python scripts/bench_crops.py [--out profiles/crops_decode_ab.txt] [--regions 15]

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
ROWS = [((224, 224), 1), ((224, 224), 16), ((224, 224), 64), ((224, 224), 256), ((1024, 768), 64)]
SEED = 20262
STEPS = {"lists": 540}  # step -> its time limit, seconds


def step_lists(regions):
    import numpy as np
    import torch
    from bench_region import _fmt, _setup, _timed
    from metalhuffman_amd import decoder as D
    dev, tabs, sets = _setup()
    print(f"[lists] N crops of one {SIDE}x{SIDE} mirror-tile frame at seeded random PIXEL origins, one prepared "
          f"table, cold regions, HIP events, median (min .. max) us over {regions} regions")
    print(f"  {'crop':<10} {'N':>4} {'grid':>9}   {'(a) mh_decode_crops':<34} "
          f"{'(b) windows + gather':<34} {'(c) mh_decode_windows, aligned':<34} (a)/(b)  (a)/(c)  blocks a/c")
    rows = []
    rng = np.random.default_rng(SEED)
    for (w, h), n in ROWS:
        # (origins at least a block inside the right and bottom edge, so that (b)'s grown windows fit the grid)
        x0 = rng.integers(0, SIDE - w - 7, n)
        y0 = rng.integers(0, SIDE - h - 7, n)
        f = np.zeros(n, np.int64)
        crops = torch.from_numpy(np.stack([f, x0, y0, f], axis=1).astype(np.int32)).to(dev)
        wl, (bw, bh), dx, dy = D.windows_of_rects(SIDE, SIDE, f, x0, y0, w, h)
        wins_b = torch.from_numpy(np.concatenate([wl, np.zeros((n, 1), np.int64)], axis=1).astype(np.int32)).to(dev)
        cbw, cbh = (w + 7) // 8, (h + 7) // 8
        wins_c = torch.from_numpy(np.stack([f, x0 // 8, y0 // 8, f], axis=1).astype(np.int32)).to(dev)
        out_a = torch.empty((n, h, (w + 7) // 8 * 8), dtype=torch.uint8, device=dev)
        big_b = torch.empty((n, 8 * bh, 8 * bw), dtype=torch.uint8, device=dev)
        out_c = torch.empty((n, 8 * cbh, 8 * cbw), dtype=torch.uint8, device=dev)
        # the gather's index tensors, broadcast: [n, 1, 1], [n, h, 1], [n, 1, w]
        I = torch.arange(n, device=dev)[:, None, None]
        Y = (torch.from_numpy(dy).to(dev)[:, None] + torch.arange(h, device=dev)[None, :])[:, :, None]
        X = (torch.from_numpy(dx).to(dev)[:, None] + torch.arange(w, device=dev)[None, :])[:, None, :]
        res_b = {}

        def route_a(s):
            D.decode_crops(s["fr"], tabs, crops, (w, h), out=out_a)

        def route_b(s):
            D.decode_windows(s["fr"], tabs, wins_b, (bw, bh), out=big_b)
            res_b["out"] = big_b[I, Y, X]

        def route_c(s):
            D.decode_windows(s["fr"], tabs, wins_c, (cbw, cbh), out=out_c)

        for s in sets:  # parity first (and the warm-up of every kernel)
            want = torch.stack([s["ref"][int(y): int(y) + h, int(x): int(x) + w] for x, y in zip(x0, y0)])
            want_c = torch.stack([s["ref"][int(y) // 8 * 8: int(y) // 8 * 8 + 8 * cbh,
                                           int(x) // 8 * 8: int(x) // 8 * 8 + 8 * cbw] for x, y in zip(x0, y0)])
            out_a.fill_(0xA5)
            big_b.fill_(0xA5)
            out_c.fill_(0xA5)
            route_a(s)
            route_b(s)
            route_c(s)
            torch.cuda.synchronize(dev)
            for got, ref, name in ((out_a[:, :, :w], want, "a"), (res_b["out"], want, "b"), (out_c, want_c, "c")):
                if not torch.equal(got, ref):
                    raise SystemExit(f"bench_crops: route ({name}) differs from the encoder's input ({n} x {w}x{h})")
        g, wv = D.decode_crops_shape(sets[0]["fr"], n, (w, h))
        res = _timed(dev, {"a": route_a, "b": route_b, "c": route_c}, sets, regions)
        ab = round(res["a"]["median_us"] / res["b"]["median_us"], 4)
        ac = round(res["a"]["median_us"] / res["c"]["median_us"], 4)
        # blocks decoded: (a) the blocks each crop touches, (c) ceil(w / 8) x ceil(h / 8) per crop
        blocks_a = int((((x0 % 8 + w + 7) // 8) * ((y0 % 8 + h + 7) // 8)).sum())
        blocks = round(blocks_a / (n * cbw * cbh), 4)
        rows.append({"crop": [w, h], "n_crops": n, "origins": np.stack([x0, y0], axis=1).tolist(),
                     "windows_b_blocks": [bw, bh], "windows_c_blocks": [cbw, cbh],
                     "shape": {"groups_per_crop": g, "waves_per_group": wv}, "routes": res, "a_over_b": ab,
                     "a_over_c": ac, "blocks_a_over_c": blocks})
        print(f"  {f'{w}x{h}':<10} {n:>4} {f'{n}x{g}x{wv}':>9}   {_fmt(res['a']):<34} {_fmt(res['b']):<34} "
              f"{_fmt(res['c']):<34} {ab:.3f}    {ac:.3f}    {blocks:.3f}")
    print(json.dumps({"step": "lists", "device": torch.cuda.get_device_name(dev), "seed": SEED, "rows": rows}))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crops_decode_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        step_lists(args.regions)
        return 0
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_crops.py --regions {args.regions}   (library stamp {B.library_stamp()[:16]})\n"]
    for step in ("lists",):  # under its own time limit
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--regions", str(args.regions)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)  # (stderr passes through)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"bench_crops: step {step} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
        text.append(p.stdout)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
