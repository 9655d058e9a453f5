#!/usr/bin/env python3
"""Scaled region decode (mh_decode_region_scaled) of windows of the 8192^2 mirror tile (config 3) at
1/2, 1/4 and 1/8 scale against what a caller did before it, with one prepared table:

  (a) mh_decode_region_scaled of the blocks that cover the window, into the reduced raster;
  (b) mh_decode_region into a raster of the region's full size, then one reduction pass over it in
      torch (an integer reshape-sum, rounded and narrowed to bytes);
  (c) mh_decode_region alone on the same window: (b) without its second pass.

The claim checked is (a) < (b) at every row (the exit status says so); (a) / (c) is reported. The
windows are scripts/bench_region.py's four (256^2, 1024x768, 2048x1536, 4096^2, interior position)
and the whole frame; its method too: two resident frames of one table alternate region by region,
every region is cold -- a 1 GiB device copy evicts the Infinity Cache and the L2s first
(bench.FLUSH), off the clock -- the launches of a region are enqueued behind bench.py's launch
gate between two HIP events, the figure is the events' distance, the routes alternate region by
region, and the table gives the median (min .. max) over the timed regions. (a) is compared with
the box means of the encoder's input before timing.

    python scripts/bench_scaled.py [--out profiles/scaled_decode_ab.txt] [--regions 15]

runs the measurement as a child process under its own `timeout` and writes what it printed to
--out. `--step scaled` runs it here.
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
WINDOWS = [(256, 256), (1024, 768), (2048, 1536), (4096, 4096), (SIDE, SIDE)]
LIMIT = 900  # seconds


def step_scaled(regions):
    import torch
    import bench_region as BR
    from metalhuffman_amd import decoder as D
    dev, tabs, sets = BR._setup()
    print(f"[scaled] windows of one {SIDE}x{SIDE} mirror-tile frame at 1/2, 1/4, 1/8 scale, one prepared table, cold "
          f"regions, HIP events, median (min .. max) us over {regions} regions")
    print(f"  {'window':<11} {'scale':<6} {'region (blocks)':<20} {'grid':>8}   {'(a) mh_decode_region_scaled':<32} "
          f"{'(b) mh_decode_region + reduce':<32} {'(c) mh_decode_region':<32} (a)/(b)  (a)/(c)")
    rows, ok = [], True
    for (w, h) in WINDOWS:
        x0, y0 = min(8 * 301 + 3, SIDE - w), min(8 * 205 + 5, SIDE - h)
        region, _, _ = D.region_of_rect(SIDE, SIDE, x0, y0, w, h)
        rw, rh = region.pixel_size(SIDE, SIDE)
        assert rw == 8 * region.bw and rh == 8 * region.bh      # SIDE is a multiple of 8: whole cells only
        px, py = 8 * region.bx0, 8 * region.by0
        big = torch.empty((1, rh, rw), dtype=torch.uint8, device=dev)
        for k in (1, 2, 3):
            s = 1 << k
            out_a = torch.empty((1, rh // s, rw // s), dtype=torch.uint8, device=dev)
            out_b = torch.empty_like(out_a)

            def reduce_into(dst, src):
                acc = src.view(1, rh // s, s, rw // s, s).sum(dim=(2, 4), dtype=torch.int32)
                dst.copy_((acc + (s * s // 2)) >> (2 * k))

            def route_a(st):
                D.decode_region_scaled(st["fr"], tabs, region, k, out=out_a)

            def route_b(st):
                D.decode_region(st["fr"], tabs, region, out=big)
                reduce_into(out_b, big)

            def route_c(st):
                D.decode_region(st["fr"], tabs, region, out=big)

            for st in sets:  # parity first (and the warm-up of every kernel)
                want = torch.empty_like(out_a)
                reduce_into(want, st["ref"][py:py + rh, px:px + rw].contiguous().view(1, rh, rw))
                out_a.fill_(0xA5)
                out_b.fill_(0xA5)
                route_a(st)
                route_b(st)
                torch.cuda.synchronize(dev)
                if not torch.equal(out_a, want) or not torch.equal(out_b, want):
                    raise SystemExit(f"bench_scaled: a route differs from the box means of the encoder's input "
                                     f"({w}x{h}, k = {k})")
            g, wv = D.decode_region_scaled_shape(sets[0]["fr"], region, k)
            res = BR._timed(dev, {"a": route_a, "b": route_b, "c": route_c}, sets, regions)
            ab = round(res["a"]["median_us"] / res["b"]["median_us"], 4)
            ac = round(res["a"]["median_us"] / res["c"]["median_us"], 4)
            ok = ok and ab < 1.0
            rows.append({"window": [w, h], "log2_scale": k, "region": list(region),
                         "shape": {"groups_per_frame": g, "waves_per_group": wv}, "routes": res, "a_over_b": ab,
                         "a_over_c": ac})
            print(f"  {f'{w}x{h}':<11} {f'1/{s}':<6} {str(tuple(region)):<20} {f'{g}x{wv}':>8}   {BR._fmt(res['a']):<32} "
                  f"{BR._fmt(res['b']):<32} {BR._fmt(res['c']):<32} {ab:.3f}    {ac:.3f}")
    print(f"(a) < (b) at every row: {'yes' if ok else 'NO'}")
    print(json.dumps({"step": "scaled", "device": torch.cuda.get_device_name(dev), "rows": rows, "a_below_b": ok}))
    return 0 if ok else 1


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=["scaled"], help="run the measurement in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scaled_decode_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        return step_scaled(args.regions)
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--step", "scaled",
           "--regions", str(args.regions)]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)  # (stderr passes through)
    sys.stdout.write(p.stdout)
    sys.stdout.flush()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# python scripts/bench_scaled.py --regions {args.regions}   (library stamp {B.library_stamp()[:16]})\n\n")
        f.write(p.stdout)
    if p.returncode != 0:
        print(f"bench_scaled: the measurement failed or (a) >= (b) somewhere (exit {p.returncode})", file=sys.stderr)
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
