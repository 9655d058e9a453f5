#!/usr/bin/env python3
"""Every frame of a SET decoded whole in one launch (mh_decode_set_frames) against what a caller had to
do before, on 192 frames per region, a table per frame, whose sizes are K = 1, 4 or 16 steps from
256x256 to 2048x1536 (bench_encode_set.py's sets: size i holds the frames of images i, i + K, ...):

  (a) one mh_decode_set_frames launch over all 192 frames, the plan made by mh_decode_set_plan with
      the kernel's resident workgroups as the budget and uploaded beforehand;
  (b) one mh_decode_frames launch per size present (K launches), over batches already grouped by
      size -- views into the same device arrays, so (b) pays nothing for the regrouping.

At K = 1 (b) is the parent entry on the same frames, so (a)/(b) there is the price of the map word and
the three record loads: reported, not gated. The gate: (a)/(b) < 0.96 at K >= 4 -- 0.96 is the margin
for the +-4 % box-to-box spread recorded in README.md -- against (b) measured in the same run.
`skew`, reported and not gated: one 2048x1536 frame beside 191 of 256x256, to see what the planner's
proportional rule does when one frame holds a fifth of the work.

The frames are encoded on the device by mh_encode_set_device_async from crops of a mirror-tiled
BigBridge, each at its own origin. Regions are cold, as bench.py's: two resident sets alternate, and a
1 GiB device copy evicts the Infinity Cache and the L2s before every region (bench.FLUSH), off the
clock. A region's launches are enqueued behind bench.py's launch gate between two HIP events; the
figure is the events' distance, the median (min..max) of --regions regions. The arms alternate region
by region. Before any timing, (a)'s rasters are compared with (b)'s and with the source pixels bit for
bit, frame by frame. Every line carries the source stamp.

    python scripts/bench_decode_set.py [--out profiles/decode_set_ab.txt] [--regions 15]

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

N_FRAMES = 192
STEPS = {"k1": 420, "k4": 420, "k16": 420, "skew": 420}  # step -> its time limit, seconds
ORDER = ("k1", "k4", "k16", "skew")
GATED = ("k4", "k16")
GATE = 0.96


def _stamp() -> str:
    import metalhuffman_amd as mh
    import metalhuffman_amd.build as B
    s = B.source_stamps()
    return f"[lib {s['lib']} mh_decode.hip {s['mh_decode.hip']} loaded {mh.lib().mh_build_stamp().decode()[:16]}]"


def _stats(us):
    import numpy as np
    return {"median_us": round(float(np.median(us)), 2), "min_us": round(float(min(us)), 2),
            "max_us": round(float(max(us)), 2), "regions": len(us), "us": [round(float(u), 2) for u in us]}


def groups_of(kind):
    """[((W, H), frames)] of a step: K sizes from 256x256 to 2048x1536 in even steps, multiples of 64
    (K = 1: the largest), 64 images x 3 planes dealt over them; or the skewed set."""
    if kind == "skew":
        return [((2048, 1536), 1), ((256, 256), N_FRAMES - 1)]
    k = int(kind[1:])
    if k == 1:
        return [((2048, 1536), N_FRAMES)]
    sizes = [((256 + (2048 - 256) * i // (k - 1)) // 64 * 64, (256 + (1536 - 256) * i // (k - 1)) // 64 * 64)
             for i in range(k)]
    return [(s, len(range(i, 64, k)) * 3) for i, s in enumerate(sizes)]


def scan(kind):
    """CPU only: the tiles of a step's two resident sets whose code span exceeds the decoder's
    4352-byte staging window (hdr_resolve's span rule), frame by frame, from codec.encode_frame of the
    same crops -- the tiles a wave decodes unpipelined."""
    import numpy as np
    import metalhuffman_amd as mh
    from metalhuffman_amd import frames as F
    bb = F.bigbridge()
    src = F.mirror_tile(bb, 2 * bb.shape[0], 2 * bb.shape[1])
    for which in range(2):
        k0, f, found = which * N_FRAMES, 0, []
        for (w, h), cnt in groups_of(kind):
            for j in range(cnt):
                im = np.ascontiguousarray(src[37 * (k0 + j) % bb.shape[0]:, 101 * (k0 + j) % bb.shape[1]:][:h, :w])
                ef = mh.encode_frame(im, limit_lengths=True)
                offs = np.append(ef.block_offsets.astype(np.int64), 8 * ef.payload_bytes)
                tiles = -(-ef.n_blocks // 64)
                start = offs[0: ef.n_blocks: 64]
                end = offs[np.minimum(np.arange(1, tiles + 1) * 64, ef.n_blocks)]
                over = np.flatnonzero(((end >> 3) + 24) - ((start >> 3) & ~15) > 4352)
                if over.size:
                    found.append(f"frame {f} ({w}x{h}, {tiles} tiles): tiles {over.tolist()}")
                f += 1
            k0 += cnt
        print(f"[{kind}] set {which}: {len(found)} frame(s) with oversize tiles" + "".join("\n    " + x for x in found))


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
        raise SystemExit("bench_decode_set: the launch gate (scripts/micro/liblaunch_gate.so) is not built")
    stamp = _stamp()
    L = N.lib()
    groups = groups_of(kind)
    n = sum(c for _, c in groups)
    assert n == N_FRAMES
    bb = F.bigbridge()
    src = F.mirror_tile(bb, 2 * bb.shape[0], 2 * bb.shape[1])
    stream = torch.cuda.current_stream(dev).cuda_stream
    eflags = N.MH_ENCODE_WORKSPACE_ZEROED | N.MH_ENCODE_LIMIT_LENGTHS
    lut_stride = (int(L.mh_lut_bytes()) + 15) // 16 * 16
    fr0 = N.mh_frame()
    resident, waves = ctypes.c_uint32(0), ctypes.c_uint32(0)
    N.check(L.mh_decode_set_frames_shape(ctypes.byref(fr0), stream, ctypes.byref(resident), ctypes.byref(waves)),
            "mh_decode_set_frames_shape")

    S, plan_us = [], []
    for which in range(2):
        # ---- the set, encoded on the device: frames in group order, so a group is a run of the set ----
        gray, records, k0 = [], [], which * n
        for (w, h), cnt in groups:
            planes = np.stack([src[37 * (k0 + j) % bb.shape[0]:, 101 * (k0 + j) % bb.shape[1]:][:h, :w] for j in range(cnt)])
            k0 += cnt
            g = torch.from_numpy(np.ascontiguousarray(planes)).to(dev)
            gray.append(g)
            records += [(g.data_ptr() + j * w * h, w, 1, w, h, default_slot_bytes(w, h)) for j in range(cnt)]
        ep = codec.encode_set_plan(records, eflags)
        t = ep.totals
        d_eplan = torch.from_numpy(ep.plan).to(dev)
        codes = torch.zeros(int(t.codes_bytes), dtype=torch.uint8, device=dev)
        offs = torch.zeros(int(t.total_blocks), dtype=torch.int32, device=dev)
        canon = torch.zeros((n, 256), dtype=torch.uint8, device=dev)
        lens = torch.zeros(n, dtype=torch.int64, device=dev)
        fco = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        estatus = torch.zeros(n, dtype=torch.int32, device=dev)
        ws = torch.zeros(int(t.workspace_bytes) + 256, dtype=torch.uint8, device=dev)
        wp = (ws.data_ptr() + 255) // 256 * 256
        assert codes.data_ptr() % 16 == 0 and d_eplan.data_ptr() % 16 == 0
        N.check(L.mh_encode_set_device_async(d_eplan.data_ptr(), ctypes.byref(t), eflags, canon.data_ptr(),
                                             codes.data_ptr(), t.codes_bytes, lens.data_ptr(), fco.data_ptr(),
                                             offs.data_ptr(), None, estatus.data_ptr(), wp,
                                             ws.numel() - (wp - ws.data_ptr()), stream), "mh_encode_set_device_async")
        luts = torch.zeros((n, lut_stride), dtype=torch.uint8, device=dev)
        tstatus = torch.zeros(n, dtype=torch.int32, device=dev)
        N.check(L.mh_build_luts_device(canon.data_ptr(), n, luts.data_ptr(), lut_stride, tstatus.data_ptr(), stream),
                "mh_build_luts_device")
        torch.cuda.synchronize(dev)
        if estatus.any().item() or tstatus.any().item():
            raise SystemExit(f"bench_decode_set: a frame was rejected by the encoder or the table build ({kind})")
        del ws
        o = int(t.geoms_offset)
        d_geoms = d_eplan[o: o + 16 * n]
        geoms = ep.geoms.copy()
        # ---- (a): the plan, uploaded beforehand ----
        t0 = time.perf_counter()
        plan = codec.decode_set_plan(geoms, int(resident.value))
        plan_us.append((time.perf_counter() - t0) * 1e6)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev)
        a = {"fr": N.mh_frame(offs.data_ptr(), codes.data_ptr(), codes.numel(), fco.data_ptr(), None, None, 0, None, None,
                              N.mh_dims(int(t.max_width), int(t.max_height), 0, 0), n, 0),
             "rasters": up(plan.rasters), "shares": up(plan.shares), "map": up(plan.group_frame), "plan": plan,
             "out": torch.zeros(plan.out_bytes, dtype=torch.uint8, device=dev), "blocks": int(t.total_blocks)}
        assert a["out"].data_ptr() % 8 == 0 and d_geoms.data_ptr() % 16 == 0
        # ---- (b): a batch per size, views into the same arrays ----
        b, f0, b0 = [], 0, 0
        for ((w, h), cnt), g in zip(groups, gray):
            nb = (w // 8) * (h // 8)
            fr = N.mh_frame(offs.data_ptr() + 4 * b0, codes.data_ptr(), codes.numel(), fco.data_ptr() + 8 * f0, None,
                            None, 0, None, None, N.mh_dims(w, h, w // 8, h // 8), cnt, 0)
            b.append({"fr": fr, "luts": luts.data_ptr() + f0 * lut_stride, "w": w, "h": h, "n": cnt, "f0": f0,
                      "gray": g, "out": torch.zeros((cnt, h, w), dtype=torch.uint8, device=dev)})
            f0, b0 = f0 + cnt, b0 + cnt * nb
        S.append({"a": a, "b": b, "geoms": d_geoms, "luts": luts,
                  "keep": (d_eplan, codes, offs, canon, lens, fco, estatus, tstatus, gray)})

    def dec_a(s):
        a = s["a"]
        N.check(L.mh_decode_set_frames(ctypes.byref(a["fr"]), s["geoms"].data_ptr(), a["blocks"], a["rasters"].data_ptr(),
                                       a["shares"].data_ptr(), a["map"].data_ptr(), a["plan"].n_groups,
                                       s["luts"].data_ptr(), lut_stride, None, None, a["out"].data_ptr(),
                                       a["out"].numel(), stream), "mh_decode_set_frames")

    def dec_b(s):
        for g in s["b"]:
            N.check(L.mh_decode_frames(ctypes.byref(g["fr"]), g["luts"], lut_stride, None, g["out"].data_ptr(), g["w"],
                                       g["w"] * g["h"], stream), "mh_decode_frames")

    # bit identity of (a), (b) and the source pixels first, frame by frame (and every kernel's warm-up)
    for s in S:
        dec_a(s)
        dec_b(s)
        torch.cuda.synchronize(dev)
        p = s["a"]["plan"]
        for g in s["b"]:
            if not torch.equal(g["out"], g["gray"]):
                raise SystemExit(f"bench_decode_set: (b)'s rasters differ from the source at {g['w']}x{g['h']} ({kind})")
            for j in range(g["n"]):
                f = g["f0"] + j
                off, pitch = int(p.offsets[f]), int(p.pitches[f])
                view = s["a"]["out"].as_strided((g["h"], g["w"]), (pitch, 1), off)
                if not torch.equal(view, g["out"][j]):
                    raise SystemExit(f"bench_decode_set: (a)'s frame {f} differs from (b)'s ({kind})")
    arms = {"a": dec_a, "b": dec_b}
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
    plan = S[0]["a"]["plan"]
    res = {"step": kind, "device": torch.cuda.get_device_name(dev), "frames": n,
           "groups": [[list(s), c] for s, c in groups], "resident_groups": int(resident.value),
           "set_groups": plan.n_groups, "set_groups_per_size": [int(plan.shares[g["f0"], 1]) for g in S[0]["b"]],
           "source_stamp": stamp, "planner_host_us": [round(u, 1) for u in plan_us],
           "arms": {k: _stats(v) for k, v in times.items()}}
    med = {k: v["median_us"] for k, v in res["arms"].items()}
    res["a_over_b"] = round(med["a"] / med["b"], 4)
    res["gated"] = kind in GATED
    K = len(groups)
    label = {"a": f"(a) one set launch, {plan.n_groups} workgroups", "b": f"(b) {K} frames launch(es), grouped by size"}
    what = (f"1 frame of 2048x1536 and {N_FRAMES - 1} of 256x256" if kind == "skew" else
            f"{n} frames in {K} size(s) {groups[0][0][0]}x{groups[0][0][1]} .. {groups[-1][0][0]}x{groups[-1][0][1]}")
    lines = [f"[{kind}] {what}, a table per frame; cold regions, HIP events, median (min..max) us over {regions} "
             f"regions; budget {resident.value} resident workgroups; host planner {min(plan_us):.0f} us"]
    for name in "ab":
        v = res["arms"][name]
        lines.append(f"  {label[name]:<56} {v['median_us']:9.2f} ({v['min_us']:.2f} .. {v['max_us']:.2f})   "
                     f"{v['median_us'] / n:.2f} us per frame")
    if kind in GATED:
        verdict = f"gate (a)/(b) < {GATE}: {'pass' if res['a_over_b'] < GATE else 'FAIL'}"
    elif kind == "k1":
        verdict = "(b) is the parent entry on the same frames: the price of the map and record loads, reported, not gated"
    else:
        verdict = "reported, not gated"
    lines.append(f"  (a)/(b) = {res['a_over_b']:.3f}   {verdict}")
    lines.append(json.dumps(res))
    for line in lines:
        print(f"{line}  {stamp}")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--scan", choices=sorted(STEPS), help="CPU only: list a step's tiles above the staging window")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_set_ab.txt"))
    args = ap.parse_args(argv)
    if args.scan:
        scan(args.scan)
        return 0
    if args.step:
        step(args.step, args.regions)
        return 0
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_decode_set.py --regions {args.regions}   (library stamp "
            f"{B.library_stamp()[:16]})\n"]
    ratios = {}
    for name in ORDER:  # each under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(STEPS[name]), sys.executable, os.path.abspath(__file__), "--step", name,
               "--regions", str(args.regions)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)  # (stderr passes through)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"bench_decode_set: step {name} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
        text.append(p.stdout)
        ratios[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1].rsplit("  [", 1)[0])["a_over_b"]
    failed = [k for k in GATED if not ratios[k] < GATE]
    verdict = (f"GATE (a)/(b) < {GATE} on {', '.join(GATED)}: " +
               ("pass" if not failed else f"FAIL on {', '.join(failed)}") +
               " -- " + ", ".join(f"{k} {ratios[k]:.3f}" for k in ratios) + " (k1 and skew: reported)")
    print(verdict)
    text.append(verdict + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
