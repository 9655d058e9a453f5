#!/usr/bin/env python3
"""The check of a batch with a table per frame (mh_check_frames) against what a caller could do before
it, on 64 frames of 2048x1536 per region (the method of bench_multitable.py):

  distinct -- 64 crops of a mirror-tiled BigBridge at 64 origins, 64 tables:
    (a) one mh_check_frames call, a prepared table per frame;
    (b) 64 one-frame mh_check calls, each with that frame's T1/T2: the only route before (a);
    (c) mh_decode_frames of the same batch. Not the same job: the yardstick for "a check costs no
        more than the decode it guards".
  shared -- 64 BigBridge block shuffles, one table:
    (a0) mh_check_frames with stride 0;
    (d)  one mh_check call over the batch: the same job, and the reports are compared before timing.

Regions are cold: two resident sets of 64 frames alternate, and bench.py's eviction copy runs before
every region, off the clock. A region's launches are enqueued behind bench.py's launch gate between
two HIP events; the routes alternate region by region; all tables and buffers are made outside the
clock. Median (min .. max) of --regions regions.

    python scripts/bench_check_frames.py [--out profiles/check_frames_ab.txt] [--regions 15]

Each step runs as a child process under its own `timeout`. Exit status 3 when (a)/(b) >= 0.96 (the
+-4 % box spread): the one-launch check must beat the per-frame calls. (a)/(c) and (a0)/(d) are
reported, not gated.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_FRAMES = 64
STEPS = {"distinct": 420, "shared": 300}  # step -> its time limit, seconds
GATE_RATIO = 0.96
CLEAN = [0, 0, 0, 0xFFFFFFFF]


def step_check(kind, regions):
    import numpy as np
    import torch
    import bench
    import bench_multitable as BM
    from metalhuffman_amd import _native as N
    from metalhuffman_amd import decoder as D
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if not bench.GATE.ok():
        raise SystemExit("bench_check_frames: the launch gate (scripts/micro/liblaunch_gate.so) is not built")
    L = N.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    sets = []
    for imgs, efs in BM._frame_sets(kind):
        batch = D.DeviceFrames.pack(efs, dev, shared_table=(kind == "shared"))
        s = {"batch": batch, "fr": D._frames_entry(batch)[0],
             "rep": torch.empty((N_FRAMES, 4), dtype=torch.int32, device=dev),
             "rep2": torch.empty((N_FRAMES, 4), dtype=torch.int32, device=dev),
             "verdict": torch.empty(N_FRAMES, dtype=torch.int32, device=dev)}
        if kind == "shared":
            s["tabs"] = D.DeviceTables.from_canonical_header(efs[0].canon, dev)
            s["tabs"].check_status()
            s["fr_d"] = D._frame_struct(batch, s["tabs"])
        else:
            s["tset"] = D.DeviceTableSet.from_canonical_headers(np.stack([ef.canon for ef in efs]), dev)
            s["tset"].check_status()
            s["singles"] = [D.DeviceFrames.pack([ef], dev) for ef in efs]
            s["tabs"] = [D.DeviceTables.from_canonical_header(ef.canon, dev, prepare_lut=False) for ef in efs]
            for t in s["tabs"]:
                t.check_status()
            s["fr_b"] = [D._frame_struct(f, t) for f, t in zip(s["singles"], s["tabs"])]
            s["ref"] = torch.from_numpy(np.stack(imgs)).to(dev)
            s["out"] = torch.empty((N_FRAMES, efs[0].height, efs[0].width), dtype=torch.uint8, device=dev)
        sets.append(s)

    def route_a(s):
        N.check(L.mh_check_frames(ctypes.byref(s["fr"]), s["tset"].luts.data_ptr(), s["tset"].stride,
                                  s["tset"].status.data_ptr(), s["rep"].data_ptr(), s["verdict"].data_ptr(), stream),
                "mh_check_frames")

    def route_a0(s):
        N.check(L.mh_check_frames(ctypes.byref(s["fr"]), s["tabs"].lut.data_ptr(), 0, None, s["rep"].data_ptr(),
                                  s["verdict"].data_ptr(), stream), "mh_check_frames")

    def route_b(s):
        for i, fr in enumerate(s["fr_b"]):
            N.check(L.mh_check(ctypes.byref(fr), s["rep2"][i].data_ptr(), stream), "mh_check")

    def route_c(s):
        D.decode_frames(s["batch"], s["tset"], out=s["out"])

    def route_d(s):
        N.check(L.mh_check(ctypes.byref(s["fr_d"]), s["rep2"].data_ptr(), stream), "mh_check")

    routes = {"a0": route_a0, "d": route_d} if kind == "shared" else {"a": route_a, "b": route_b, "c": route_c}
    for s in sets:  # the same answer first (and the warm-up of every kernel)
        for t in ("rep", "rep2", "verdict"):
            s[t].fill_(0x5A5A5A5A)
        for name in sorted(routes):
            routes[name](s)
        torch.cuda.synchronize(dev)
        rep = (s["rep"].to(torch.int64) & 0xFFFFFFFF).cpu().tolist()
        if rep != (s["rep2"].to(torch.int64) & 0xFFFFFFFF).cpu().tolist() or rep != [CLEAN] * N_FRAMES:
            raise SystemExit(f"bench_check_frames: mh_check_frames and mh_check disagree, or a frame is not clean ({kind})")
        if s["verdict"].any().item():
            raise SystemExit(f"bench_check_frames: a verdict is not MH_OK ({kind})")
        if "out" in s and not torch.equal(s["out"], s["ref"]):
            raise SystemExit("bench_check_frames: route (c) differs from the encoder inputs")
    times = {name: [] for name in routes}
    for r in range(regions + 1):  # region 0 of every route is a rehearsal, not recorded
        for name in sorted(routes):
            s = sets[r % 2]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            bench.FLUSH(dev)
            torch.cuda.synchronize(dev)
            bench.GATE.arm(stream)
            e0.record()
            routes[name](s)
            e1.record()
            bench.GATE.open()
            torch.cuda.synchronize(dev)
            if r:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    g, wv = ctypes.c_uint32(), ctypes.c_uint32()
    N.check(L.mh_check_frames_shape(ctypes.byref(sets[0]["fr"]), stream, ctypes.byref(g), ctypes.byref(wv)), "shape")
    res = {"step": kind, "device": torch.cuda.get_device_name(dev), "frames_per_region": N_FRAMES,
           "frame": [sets[0]["batch"].width, sets[0]["batch"].height],
           "mh_check_frames_shape": {"groups_per_frame": g.value, "waves_per_group": wv.value},
           "routes": {name: BM._stats(us) for name, us in times.items()}}
    med = {k: v["median_us"] for k, v in res["routes"].items()}
    pairs = (("a0", "d"),) if kind == "shared" else (("a", "b"), ("a", "c"))
    for x, y in pairs:
        res[f"{x}_over_{y}"] = round(med[x] / med[y], 4)
    label = {"a": "(a) mh_check_frames, a table per frame, one call",
             "b": "(b) 64 x one-frame mh_check with the frame's T1/T2",
             "c": "(c) mh_decode_frames of the same batch (not the same job)",
             "a0": "(a0) mh_check_frames, one table (stride 0)",
             "d": "(d) mh_check, one call over the batch"}
    print(f"[{kind}] 64 x 2048x1536, cold regions, HIP events, median (min..max) us over {regions} regions:")
    for name in sorted(times):
        v = res["routes"][name]
        print(f"  {label[name]:<62} {v['median_us']:9.2f} ({v['min_us']:.2f} .. {v['max_us']:.2f})")
    print("  " + "   ".join(f"({x})/({y}) = {res[f'{x}_over_{y}']:.3f}" for x, y in pairs)
          + f"   launch shape of the walk: {g.value} workgroups x {wv.value} waves per frame")
    print(json.dumps(res))
    if kind == "distinct" and res["a_over_b"] >= GATE_RATIO:
        print(f"bench_check_frames: (a)/(b) = {res['a_over_b']:.3f} >= {GATE_RATIO}: the gate fails", file=sys.stderr)
        raise SystemExit(3)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_frames_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        step_check(args.step, args.regions)
        return 0
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_check_frames.py --regions {args.regions}   (library stamp "
            f"{B.library_stamp()[:16]})\n"]
    status = 0
    for step in ("distinct", "shared"):  # each under its own time limit; stop at a failure that is not the gate's
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--regions", str(args.regions)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)  # (stderr passes through)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        text.append(p.stdout)
        if p.returncode == 3:
            status = 3
        elif p.returncode != 0:
            print(f"bench_check_frames: step {step} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return status


if __name__ == "__main__":
    sys.exit(main())
