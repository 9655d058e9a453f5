#!/usr/bin/env python3
"""Frames of DIFFERENT sizes into the frame-set layout in one call (mh_encode_set_device_async) against
what a caller had to do before, on 64 three-plane images (192 planar frames) per region whose sizes are
K = 1, 4 or 16 steps from 256x256 to 2048x1536 (image i has size i % K):

  (a) one set call over all 192 frames (three launches), the plan already uploaded;
  (b) one mh_encode_frames_device_async call per size present (3 K launches), over frames already
      grouped by size, each group into outputs of its own -- (b) does not even repack its K outputs
      into one frame set, which favours it;
  (c) K = 1 only: the frames entry on the same frames: what the map and record loads and the set's
      8-byte fetch (the frames entry takes 16-byte loads here) cost.

The gate: (a)/(b) < 0.96 at K >= 4 -- 0.96 is the margin for the +-4 % box-to-box spread recorded in
README.md -- against (b) measured in the same run. (a)/(c) is reported. The host planner's time (pure
host code, off the device's clock) is reported per step.

Every frame is a crop of a mirror-tiled BigBridge at its own origin. Regions are cold, as bench.py's:
two resident sets alternate, and a 1 GiB device copy evicts the Infinity Cache and the L2s before
every region (bench.FLUSH), off the clock. A region's launches are enqueued behind bench.py's launch
gate between two HIP events; the figure is the events' distance, the median (min..max) of --regions
regions. The arms alternate region by region. Before any timing, (a)'s outputs are compared with
(b)'s byte for byte, frame by frame. Every line carries the source stamp.

    python scripts/bench_encode_set.py [--out profiles/encode_set_ab.txt] [--regions 15]

runs each step as a child process under its own `timeout`, stops at the first failure and writes what
the steps printed, then the gate's verdict, to --out. `--step NAME` runs one step here.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_IMAGES, C = 64, 3
STEPS = {"k1": 420, "k4": 420, "k16": 420}  # step -> its time limit, seconds
GATED = ("k4", "k16")
GATE = 0.96


def _stamp() -> str:
    import metalhuffman_amd as mh
    import metalhuffman_amd.build as B
    s = B.source_stamps()
    return f"[lib {s['lib']} mh_encode.hip {s['mh_encode.hip']} loaded {mh.lib().mh_build_stamp().decode()[:16]}]"


def _stats(us):
    import numpy as np
    return {"median_us": round(float(np.median(us)), 2), "min_us": round(float(min(us)), 2),
            "max_us": round(float(max(us)), 2), "regions": len(us), "us": [round(float(u), 2) for u in us]}


def sizes_of(k):
    """K sizes from 256x256 to 2048x1536 in even steps, multiples of 64 (K = 1: the largest)."""
    if k == 1:
        return [(2048, 1536)]
    return [((256 + (2048 - 256) * i // (k - 1)) // 64 * 64, (256 + (1536 - 256) * i // (k - 1)) // 64 * 64)
            for i in range(k)]


def step(kind, regions):
    import numpy as np
    import torch
    import bench
    from metalhuffman_amd import _native as N
    from metalhuffman_amd import codec
    from metalhuffman_amd import frames as F
    from metalhuffman_amd.encoder import default_slot_bytes
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if not bench.GATE.ok():
        raise SystemExit("bench_encode_set: the launch gate (scripts/micro/liblaunch_gate.so) is not built")
    stamp = _stamp()
    L = N.lib()
    K = int(kind[1:])
    sizes = sizes_of(K)
    per = [len(range(i, N_IMAGES, K)) * C for i in range(K)]   # frames of each size
    n = sum(per)
    bb = F.bigbridge()
    src = F.mirror_tile(bb, 2 * bb.shape[0], 2 * bb.shape[1])
    stream = torch.cuda.current_stream(dev).cuda_stream
    flags = N.MH_ENCODE_WORKSPACE_ZEROED | N.MH_ENCODE_LIMIT_LENGTHS   # (a deep tree is limited, never rejected)

    def outputs(frames, slot_bytes, blocks):
        o = {"codes": torch.zeros(slot_bytes, dtype=torch.uint8, device=dev),
             "offs": torch.zeros(blocks, dtype=torch.int32, device=dev),
             "canon": torch.zeros((frames, 256), dtype=torch.uint8, device=dev),
             "lens": torch.zeros(frames, dtype=torch.int64, device=dev),
             "fco": torch.zeros(frames + 1, dtype=torch.int64, device=dev),
             "status": torch.zeros(frames, dtype=torch.int32, device=dev)}
        assert o["codes"].data_ptr() % 16 == 0
        return o

    def workspace(nbytes):
        t = torch.zeros(nbytes + 256, dtype=torch.uint8, device=dev)
        p = (t.data_ptr() + 255) // 256 * 256
        return t, p, t.numel() - (p - t.data_ptr())

    S = []
    plan_us = []
    for which in range(2):
        groups, records = [], []
        k0 = which * n
        for (w, h), cnt in zip(sizes, per):
            planes = np.stack([src[37 * (k0 + j) % bb.shape[0]:, 101 * (k0 + j) % bb.shape[1]:][:h, :w] for j in range(cnt)])
            k0 += cnt
            g = torch.from_numpy(np.ascontiguousarray(planes)).to(dev)
            slot = default_slot_bytes(w, h)
            nb = (w // 8) * (h // 8)
            groups.append({"gray": g, "w": w, "h": h, "n": cnt, "slot": slot, "nb": nb,
                           "out": outputs(cnt, cnt * slot, cnt * nb),
                           "ws": workspace(int(L.mh_encode_frames_workspace_bytes(w, h, cnt)))})
            records += [(g.data_ptr() + j * w * h, w, 1, w, h, slot) for j in range(cnt)]
        t0 = time.perf_counter()
        plan = codec.encode_set_plan(records, flags)
        plan_us.append((time.perf_counter() - t0) * 1e6)
        t = plan.totals
        S.append({"groups": groups, "plan": torch.from_numpy(plan.plan).to(dev), "totals": t,
                  "out": outputs(n, int(t.codes_bytes), int(t.total_blocks)), "ws": workspace(int(t.workspace_bytes))})
        assert S[-1]["plan"].data_ptr() % 16 == 0 and t.fetch_mode == 1

    def enc_a(s):
        o, t = s["out"], s["totals"]
        N.check(L.mh_encode_set_device_async(
            s["plan"].data_ptr(), ctypes.byref(t), flags, o["canon"].data_ptr(), o["codes"].data_ptr(), t.codes_bytes,
            o["lens"].data_ptr(), o["fco"].data_ptr(), o["offs"].data_ptr(), None, o["status"].data_ptr(), s["ws"][1],
            s["ws"][2], stream), "mh_encode_set_device_async")

    def enc_b(s):
        for g in s["groups"]:
            o = g["out"]
            N.check(L.mh_encode_frames_device_async(
                g["gray"].data_ptr(), g["w"] * g["h"], g["n"], g["w"], g["h"], flags, o["canon"].data_ptr(),
                o["codes"].data_ptr(), g["slot"], o["lens"].data_ptr(), o["fco"].data_ptr(), o["offs"].data_ptr(), None,
                o["status"].data_ptr(), g["ws"][1], g["ws"][2], stream), "mh_encode_frames_device_async")

    # byte identity of (a) and (b) first, frame by frame (and the warm-up of every kernel)
    for s in S:
        enc_a(s)
        enc_b(s)
        torch.cuda.synchronize(dev)
        a = s["out"]
        if a["status"].any().item() or any(g["out"]["status"].any().item() for g in s["groups"]):
            raise SystemExit(f"bench_encode_set: a frame was rejected ({kind})")
        f0, c0, b0 = 0, 0, 0
        fco = a["fco"].cpu().tolist()
        for g in s["groups"]:
            o, cnt = g["out"], g["n"]
            if fco[f0: f0 + cnt + 1] != [c0 + j * g["slot"] for j in range(cnt + 1)]:
                raise SystemExit(f"bench_encode_set: (a)'s frame code offsets are not the slots' ({kind})")
            for name, x, y in (("codes", a["codes"][c0: c0 + cnt * g["slot"]], o["codes"]),
                               ("offsets", a["offs"][b0: b0 + cnt * g["nb"]], o["offs"]),
                               ("headers", a["canon"][f0: f0 + cnt], o["canon"]),
                               ("lengths", a["lens"][f0: f0 + cnt], o["lens"])):
                if not torch.equal(x, y):
                    raise SystemExit(f"bench_encode_set: (a)'s {name} differ from (b)'s at {g['w']}x{g['h']} ({kind})")
            f0, c0, b0 = f0 + cnt, c0 + cnt * g["slot"], b0 + cnt * g["nb"]
    arms = {"a": enc_a, "b": enc_b}
    times = {name: [] for name in arms}
    for r in range(regions + 1):  # region 0 of every arm is a rehearsal, not recorded
        for name, fn in sorted(arms.items()):
            s = S[r % 2]
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
    res = {"step": kind, "device": torch.cuda.get_device_name(dev), "images_per_region": N_IMAGES, "planes": C,
           "sizes": sizes, "frames": n, "source_stamp": stamp, "planner_host_us": [round(u, 1) for u in plan_us],
           "arms": {k: _stats(v) for k, v in times.items()}}
    med = {k: v["median_us"] for k, v in res["arms"].items()}
    res["a_over_b"] = round(med["a"] / med["b"], 4)
    res["gated"] = kind in GATED
    label = {"a": "(a) one set call, 3 launches", "b": f"(b) {K} frames call(s), {3 * K} launches, no repacking"}
    lines = [f"[{kind}] 64 images x {C} planes in {K} size(s) {sizes[0][0]}x{sizes[0][1]} .. {sizes[-1][0]}x{sizes[-1][1]}; "
             f"cold regions, HIP events, median (min..max) us over {regions} regions; host planner "
             f"{min(plan_us):.0f} us"]
    for name in "ab":
        v = res["arms"][name]
        lines.append(f"  {label[name]:<56} {v['median_us']:9.2f} ({v['min_us']:.2f} .. {v['max_us']:.2f})   "
                     f"{v['median_us'] / n:.2f} us per frame")
    if K == 1:
        verdict = "(b) is (c) here: (a)/(c), reported, not gated"
    else:
        verdict = f"gate (a)/(b) < {GATE}: {'pass' if res['a_over_b'] < GATE else 'FAIL'}"
    lines.append(f"  (a)/(b) = {res['a_over_b']:.3f}   {verdict}")
    lines.append(json.dumps(res))
    for line in lines:
        print(f"{line}  {stamp}")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_set_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        step(args.step, args.regions)
        return 0
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_encode_set.py --regions {args.regions}   (library stamp "
            f"{B.library_stamp()[:16]})\n"]
    ratios = {}
    for name in ("k1", "k4", "k16"):  # each under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(STEPS[name]), sys.executable, os.path.abspath(__file__), "--step", name,
               "--regions", str(args.regions)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)  # (stderr passes through)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"bench_encode_set: step {name} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
        text.append(p.stdout)
        ratios[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1].rsplit("  [", 1)[0])["a_over_b"]
    failed = [k for k in GATED if not ratios[k] < GATE]
    verdict = (f"GATE (a)/(b) < {GATE} on {', '.join(GATED)}: " +
               ("pass" if not failed else f"FAIL on {', '.join(failed)}") +
               " -- " + ", ".join(f"{k} {ratios[k]:.3f}" for k in ratios) + " (k1: (a)/(c), reported)")
    print(verdict)
    text.append(verdict + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
