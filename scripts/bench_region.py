#!/usr/bin/env python3
"""Region decode (mh_decode_region) of windows of the 8192^2 mirror tile (config 3) against what a
caller did before it, with one prepared table:

  (a) mh_decode_region of the blocks that cover the window, into a raster of the region's size;
  (b) full-frame mh_decode into a W x H raster, then a device copy of the window out of it;
  (c) the mapping's own cost: mh_decode_region over the FULL frame against mh_decode_frames
      (n = 1) on the same frame, the same table, the same raster.

Windows of 256^2, 1024x768, 2048x1536 and 4096^2 pixels, each at an interior position and at the
frame's right/bottom edge. Two resident 8192^2 frames of one table (the mirror tile and a block
shuffle of it) alternate region by region. scripts/bench_multitable.py's method: every region is
cold -- a 1 GiB device copy evicts the Infinity Cache and the L2s first (bench.FLUSH), off the
clock -- the launches of a region are enqueued behind bench.py's launch gate between two HIP
events, the figure is the events' distance, the routes alternate region by region, and the table
gives the median (min .. max) over the timed regions. Every route's output is compared with the
encoder's input before timing. Lane utilisation bw / (64 ceil(bw / 64)) is printed per window.

    python scripts/bench_region.py [--out profiles/region_decode_ab.txt] [--regions 15]

runs each step (windows, full) as a child process under its own `timeout`, stops at the first
failure and writes what the steps printed to --out. `--step NAME` runs one step here.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDE = 8192
WINDOWS = [(256, 256), (1024, 768), (2048, 1536), (4096, 4096)]
STEPS = {"windows": 420, "full": 300}  # step -> its time limit, seconds


def _stats(us):
    import numpy as np
    return {"median_us": round(float(np.median(us)), 2), "min_us": round(float(min(us)), 2),
            "max_us": round(float(max(us)), 2), "regions": len(us), "us": [round(float(u), 2) for u in us]}


def _fmt(v):
    return f"{v['median_us']:9.2f} ({v['min_us']:.2f} .. {v['max_us']:.2f})"


def _setup():
    """Two resident frames of one table, their inputs on the device, one prepared table."""
    import numpy as np
    import torch
    import bench
    from metalhuffman_amd import decoder as D
    from metalhuffman_amd import frames as F
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if not bench.GATE.ok():
        raise SystemExit("bench_region: the launch gate (scripts/micro/liblaunch_gate.so) is not built")
    base = F.mirror_tile(F.bigbridge(), SIDE, SIDE)
    imgs = [base, F.block_shuffle(base, 100)]
    efs = bench.encode_many(imgs, threads=2)
    assert np.array_equal(efs[0].canon, efs[1].canon)
    t1, t2 = efs[0].tables()
    tabs = D.DeviceTables.upload(t1, t2, dev)
    sets = [{"ref": torch.from_numpy(im).to(dev), "fr": D.DeviceFrames.pack([ef], dev)} for im, ef in zip(imgs, efs)]
    return dev, tabs, sets


def _timed(dev, routes, sets, regions):
    """routes: {name: fn(set)}; alternating region by region, region 0 a rehearsal."""
    import torch
    import bench
    stream = torch.cuda.current_stream(dev).cuda_stream
    times = {name: [] for name in routes}
    for r in range(regions + 1):
        for name, fn in sorted(routes.items()):
            s = sets[r % 2]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            bench.FLUSH(dev)
            torch.cuda.synchronize(dev)
            bench.GATE.arm(stream)
            e0.record()
            fn(s)
            e1.record()
            bench.GATE.open()
            torch.cuda.synchronize(dev)
            if r:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    return {name: _stats(us) for name, us in times.items()}


def step_windows(regions):
    import torch
    from metalhuffman_amd import decoder as D
    dev, tabs, sets = _setup()
    full = torch.empty((1, SIDE, SIDE), dtype=torch.uint8, device=dev)
    print(f"[windows] windows of one {SIDE}x{SIDE} mirror-tile frame, one prepared table, cold regions, HIP events, "
          f"median (min .. max) us over {regions} regions")
    print(f"  {'window':<11} {'at':<9} {'region (blocks)':<22} {'lanes':>6} {'grid':>9}   "
          f"{'(a) mh_decode_region':<34} {'(b) mh_decode + copy of the window':<34} (a)/(b)")
    rows = []
    for (w, h) in WINDOWS:
        for where, (x0, y0) in (("interior", (8 * 301 + 3, 8 * 205 + 5)), ("edge", (SIDE - w, SIDE - h))):
            x0, y0 = min(x0, SIDE - w), min(y0, SIDE - h)
            region, dx, dy = D.region_of_rect(SIDE, SIDE, x0, y0, w, h)
            segs = -(-region.bw // 64)
            util = region.bw / (64 * segs)
            rw, rh = region.pixel_size(SIDE, SIDE)
            out_a = torch.empty((1, rh, 8 * region.bw), dtype=torch.uint8, device=dev)
            out_b = torch.empty((1, h, w), dtype=torch.uint8, device=dev)

            def route_a(s):
                D.decode_region(s["fr"], tabs, region, out=out_a)

            def route_b(s):
                D.decode(s["fr"], tabs, out=full)
                out_b.copy_(full[:, y0:y0 + h, x0:x0 + w])

            for s in sets:  # parity first (and the warm-up of every kernel)
                want = s["ref"][y0:y0 + h, x0:x0 + w]
                out_a.fill_(0xA5)
                out_b.fill_(0xA5)
                route_a(s)
                route_b(s)
                torch.cuda.synchronize(dev)
                if not torch.equal(out_a[0, dy:dy + h, dx:dx + w], want) or not torch.equal(out_b[0], want):
                    raise SystemExit(f"bench_region: a route differs from the encoder's input ({w}x{h} {where})")
            g, wv = D.decode_region_shape(sets[0]["fr"], region)
            res = _timed(dev, {"a": route_a, "b": route_b}, sets, regions)
            ratio = round(res["a"]["median_us"] / res["b"]["median_us"], 4)
            rows.append({"window": [w, h], "where": where, "origin": [x0, y0], "region": list(region),
                         "tiles": region.bh * segs, "lane_utilisation": round(util, 4),
                         "shape": {"groups_per_frame": g, "waves_per_group": wv}, "routes": res, "a_over_b": ratio})
            print(f"  {f'{w}x{h}':<11} {where:<9} {str(tuple(region)):<22} {util:6.3f} {f'{g}x{wv}':>9}   "
                  f"{_fmt(res['a']):<34} {_fmt(res['b']):<34} {ratio:.3f}")
    print(json.dumps({"step": "windows", "device": torch.cuda.get_device_name(dev), "rows": rows}))


def step_full(regions):
    import torch
    from metalhuffman_amd import decoder as D
    dev, tabs, sets = _setup()
    bw = SIDE // 8
    region = D.Region(0, 0, bw, bw)
    tset = D.DeviceTableSet(tabs.lut.reshape(1, -1), torch.zeros(1, dtype=torch.int32, device=dev))
    out = torch.empty((1, SIDE, SIDE), dtype=torch.uint8, device=dev)

    def route_region(s):
        D.decode_region(s["fr"], tabs, region, out=out)

    def route_frames(s):
        D.decode_frames(s["fr"], tset, out=out)

    for name, fn in (("region", route_region), ("frames", route_frames)):
        for s in sets:
            out.fill_(0xA5)
            fn(s)
            torch.cuda.synchronize(dev)
            if not torch.equal(out[0], s["ref"]):
                raise SystemExit(f"bench_region: route ({name}) differs from the encoder's input (full frame)")
    res = _timed(dev, {"frames": route_frames, "region": route_region}, sets, regions)
    gr, _ = D.decode_region_shape(sets[0]["fr"], region)
    gf, _ = D.decode_frames_shape(sets[0]["fr"])
    ratio = round(res["region"]["median_us"] / res["frames"]["median_us"], 4)
    print(f"[full] (c) the whole {SIDE}x{SIDE} frame, n = 1, the same table and raster, cold regions, median "
          f"(min .. max) us over {regions} regions")
    print(f"  mh_decode_region {{0, 0, {bw}, {bw}}}  ({bw * (bw // 64)} tiles of 64 blocks, grid {gr}x8)   {_fmt(res['region'])}")
    print(f"  mh_decode_frames                    ({bw * bw // 64} tiles of 64 blocks, grid {gf}x8)   {_fmt(res['frames'])}")
    print(f"  region / frames = {ratio:.3f}")
    print(json.dumps({"step": "full", "device": torch.cuda.get_device_name(dev), "routes": res,
                      "region_over_frames": ratio, "groups": {"region": gr, "frames": gf}}))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_decode_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        step_windows(args.regions) if args.step == "windows" else step_full(args.regions)
        return 0
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_region.py --regions {args.regions}   (library stamp {B.library_stamp()[:16]})\n"]
    for step in ("windows", "full"):  # each under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--regions", str(args.regions)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)  # (stderr passes through)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"bench_region: step {step} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
        text.append(p.stdout)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
