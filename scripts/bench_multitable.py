#!/usr/bin/env python3
"""Batch decode with one table per frame (mh_decode_frames) against the two routes that existed
before it, on 64 frames of 2048x1536 per region:

  (a) mh_decode_frames: one launch, a prepared table per frame (mh_build_luts_device);
  (b) mh_decode on ONE shared table: the batch kernel, one launch (only when the frames share it);
  (c) 64 one-frame mh_decode calls, each with its own tables (mh_build_tables_device per frame):
      the only route for distinct tables before (a). Launches 2..64 carry MH_FLAG_ANY_ORDER,
      as bench.py's eager regions do (every launch writes its own raster).

Two frame sets: 64 BigBridge block shuffles (one table, so all three routes decode identical
input) and 64 crops of a mirror-tiled BigBridge at 64 different origins (64 tables; (b) does not
apply). A few of those crops hold a tile whose code span exceeds the kernels' 4352-byte LDS window:
the batch loops finish such a wave's tiles in their slow loop (no prefetch), and the slowest wave
ends the launch. The step `distinct_fit` is the same measurement on crops without such a tile.
Regions are cold, as bench.py's: two resident sets of 64 frames alternate, and a 1 GiB device
copy evicts the Infinity Cache and the L2s before every region (bench.FLUSH), off the clock. The
launches of a region are enqueued behind bench.py's launch gate between two HIP events; the
figure is the events' distance (gate release -> end of the last decode). The routes alternate
region by region. Every route's output is compared with the encoder inputs before timing.
Also: mh_build_luts_device for 64 headers against 64 mh_build_tables_device calls.

    python scripts/bench_multitable.py [--out profiles/multitable_decode_ab.txt] [--regions 15]

runs each step (shared, distinct, distinct_fit, tables) as a child process under its own `timeout`, stops at
the first failure and writes what the steps printed to --out. `--step NAME` runs one step here.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_FRAMES = 64
STEPS = {"shared": 300, "distinct": 300, "distinct_fit": 300, "tables": 120}  # step -> its time limit, seconds


def _stats(us):
    import numpy as np
    return {"median_us": round(float(np.median(us)), 2), "min_us": round(float(min(us)), 2),
            "max_us": round(float(max(us)), 2), "regions": len(us), "us": [round(float(u), 2) for u in us]}


def _oversize_tiles(ef):
    """Tiles (64 blocks) of a frame whose staged code span exceeds the kernels' LDS window
    (hdr_resolve in csrc/mh_decode.hip: 16-byte aligned start, end + 24 bytes of read-ahead)."""
    import numpy as np
    o = ef.block_offsets.astype(np.int64)
    ends = np.append(o[64::64], ef.payload_bytes * 8)
    span = ((ends >> 3) + 24) - ((o[0::64] >> 3) & ~15)
    return int((((span + 15) & ~15) > 4352).sum())


def _frame_sets(kind):
    """Two sets of 64 (image, encoded frame): block shuffles of BigBridge (one table) or crops of
    a 2 x 2 mirror-tiled BigBridge at different origins (a table each; origins whose tree is deeper than
    16 bits are passed over)."""
    import numpy as np
    import bench
    import metalhuffman_amd as mh
    from metalhuffman_amd import frames as F
    bb = F.bigbridge()
    h, w = bb.shape
    if kind == "shared":
        imgs = [F.block_shuffle(bb, 20000 + k) for k in range(2 * N_FRAMES)]
        efs = bench.encode_many(imgs)
        assert all(np.array_equal(ef.canon, efs[0].canon) for ef in efs)
    else:
        src = F.mirror_tile(bb, 2 * h, 2 * w)  # (plain tiling: every crop a cyclic shift, 8 tables in all)
        imgs, efs = [], []
        k = 0
        while len(imgs) < 2 * N_FRAMES:
            im = np.ascontiguousarray(src[37 * k % h:, 101 * k % w:][:h, :w])
            k += 1
            try:
                ef = mh.encode_frame(im)
            except mh.MHError:
                continue
            if kind == "distinct_fit" and _oversize_tiles(ef):
                continue
            efs.append(ef)
            imgs.append(im)
        assert len({ef.canon.tobytes() for ef in efs}) == 2 * N_FRAMES
    return [(imgs[i:i + N_FRAMES], efs[i:i + N_FRAMES]) for i in (0, N_FRAMES)]


def step_decode(kind, regions):
    import numpy as np
    import torch
    import bench
    from metalhuffman_amd import _native as N
    from metalhuffman_amd import decoder as D
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if not bench.GATE.ok():
        raise SystemExit("bench_multitable: the launch gate (scripts/micro/liblaunch_gate.so) is not built")
    sets = []
    for imgs, efs in _frame_sets(kind):
        s = {"ref": torch.from_numpy(np.stack(imgs)).to(dev),
             "batch": D.DeviceFrames.pack(efs, dev, shared_table=(kind == "shared")),
             "tset": D.DeviceTableSet.from_canonical_headers(np.stack([ef.canon for ef in efs]), dev),
             "singles": [D.DeviceFrames.pack([ef], dev) for ef in efs],
             "tabs": [D.DeviceTables.from_canonical_header(ef.canon, dev) for ef in efs],
             "out": torch.empty((N_FRAMES, efs[0].height, efs[0].width), dtype=torch.uint8, device=dev)}
        s["tset"].check_status()
        for t in s["tabs"]:
            t.check_status()
        s["payload"] = sum(ef.payload_bytes for ef in efs)
        s["oversize"] = sum(_oversize_tiles(ef) for ef in efs)
        sets.append(s)

    def route_a(s):
        D.decode_frames(s["batch"], s["tset"], out=s["out"])

    def route_b(s):
        D.decode(s["batch"], s["tabs"][0], out=s["out"])

    def route_c(s):
        for i, fr in enumerate(s["singles"]):
            D.decode(fr, s["tabs"][i], out=s["out"][i:i + 1], extra_flags=N.MH_FLAG_ANY_ORDER if i else 0)

    routes = {"a": route_a, "c": route_c}
    if kind == "shared":
        routes["b"] = route_b
    for name, fn in sorted(routes.items()):  # parity first (and the warm-up of every kernel)
        for s in sets:
            s["out"].fill_(0xA5)
            fn(s)
            torch.cuda.synchronize(dev)
            if not torch.equal(s["out"], s["ref"]):
                raise SystemExit(f"bench_multitable: route ({name}) differs from the encoder inputs ({kind})")
    stream = torch.cuda.current_stream(dev).cuda_stream
    times = {name: [] for name in routes}
    for r in range(regions + 1):  # region 0 of every route is a rehearsal, not recorded
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
    g, wv = D.decode_frames_shape(sets[0]["batch"])
    px = N_FRAMES * sets[0]["batch"].width * sets[0]["batch"].height
    res = {"step": kind, "device": torch.cuda.get_device_name(dev), "frames_per_region": N_FRAMES,
           "frame": [sets[0]["batch"].width, sets[0]["batch"].height],
           "payload_bytes_per_region": [s["payload"] for s in sets],
           "oversize_tiles_per_region": [s["oversize"] for s in sets],
           "mh_decode_frames_shape": {"groups_per_frame": g, "waves_per_group": wv, "grid": g * N_FRAMES},
           "routes": {name: dict(_stats(us), decoded_MBps=round(px / (float(np.median(us)) * 1e-6) / 1e6, 1))
                      for name, us in times.items()}}
    med = {k: v["median_us"] for k, v in res["routes"].items()}
    res["a_over_c"] = round(med["a"] / med["c"], 4)
    if "b" in med:
        res["a_over_b"] = round(med["a"] / med["b"], 4)
    print(f"[{kind}] 64 x 2048x1536, cold regions, HIP events, median (min..max) us over {regions} regions "
          f"(tiles over the LDS window in the two sets: {[s['oversize'] for s in sets]} of {N_FRAMES * 768}):")
    label = {"a": "(a) mh_decode_frames, a table per frame, one launch",
             "b": "(b) mh_decode, one shared table, one launch (batch kernel)",
             "c": "(c) 64 x one-frame mh_decode, per-frame tables"}
    for name in sorted(times):
        v = res["routes"][name]
        print(f"  {label[name]:<62} {v['median_us']:9.2f} ({v['min_us']:.2f} .. {v['max_us']:.2f})  "
              f"{v['decoded_MBps']:.0f} MB/s decoded")
    print(f"  (a)/(c) = {res['a_over_c']:.3f}" + (f"   (a)/(b) = {res['a_over_b']:.3f}" if "b" in med else "")
          + f"   launch shape of (a): {g} workgroups x {wv} waves per frame, grid {g * N_FRAMES}")
    print(json.dumps(res))


def step_tables(regions):
    import numpy as np
    import torch
    from metalhuffman_amd import _native as N
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    efs = _frame_sets("distinct")[0][1]
    hdr = torch.from_numpy(np.stack([ef.canon for ef in efs])).to(dev)
    L = N.lib()
    stride = (int(L.mh_lut_bytes()) + 15) // 16 * 16
    luts = torch.empty((N_FRAMES, stride), dtype=torch.uint8, device=dev)
    luts1 = torch.empty_like(luts)
    t1 = torch.empty((N_FRAMES, 512), dtype=torch.uint8, device=dev)
    t2 = torch.empty((N_FRAMES, 2 * N.MH_TABLE2_MAX_ENTRIES), dtype=torch.uint8, device=dev)
    meta = torch.empty((N_FRAMES, 2), dtype=torch.int32, device=dev)
    status = torch.empty(N_FRAMES, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def batched():
        N.check(L.mh_build_luts_device(hdr.data_ptr(), N_FRAMES, luts.data_ptr(), stride, status.data_ptr(), stream),
                "mh_build_luts_device")

    def one_by_one():
        for i in range(N_FRAMES):
            N.check(L.mh_build_tables_device(hdr[i].data_ptr(), t1[i].data_ptr(), t2[i].data_ptr(),
                                             meta[i].data_ptr(), luts1[i].data_ptr(), meta[i].data_ptr() + 4, stream),
                    "mh_build_tables_device")

    batched()
    one_by_one()
    torch.cuda.synchronize(dev)
    lb = int(L.mh_lut_bytes())
    if not torch.equal(luts[:, :lb], luts1[:, :lb]) or status.any().item():
        raise SystemExit("bench_multitable: the batched table build differs from the single builds")
    times = {"batched": [], "one_by_one": []}
    for r in range(regions + 1):
        for name, fn in (("batched", batched), ("one_by_one", one_by_one)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize(dev)
            if r:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    res = {"step": "tables", "headers": N_FRAMES, "routes": {k: _stats(v) for k, v in times.items()}}
    res["batched_over_one_by_one"] = round(res["routes"]["batched"]["median_us"] /
                                           res["routes"]["one_by_one"]["median_us"], 4)
    print(f"[tables] 64 headers -> 64 prepared tables, HIP events, median (min..max) us over {regions} regions:")
    for name, text in (("batched", "mh_build_luts_device, one launch"),
                       ("one_by_one", "64 x mh_build_tables_device (T1/T2 + prepared table)")):
        v = res["routes"][name]
        print(f"  {text:<62} {v['median_us']:9.2f} ({v['min_us']:.2f} .. {v['max_us']:.2f})")
    print(f"  batched / one by one = {res['batched_over_one_by_one']:.3f}")
    print(json.dumps(res))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multitable_decode_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        step_tables(args.regions) if args.step == "tables" else step_decode(args.step, args.regions)
        return 0
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_multitable.py --regions {args.regions}   (library stamp "
            f"{B.library_stamp()[:16]})\n"]
    for step in ("shared", "distinct", "distinct_fit", "tables"):  # each under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--regions", str(args.regions)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)  # (stderr passes through)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"bench_multitable: step {step} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
        text.append(p.stdout)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
