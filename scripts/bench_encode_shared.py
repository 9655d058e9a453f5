#!/usr/bin/env python3
"""Batch encode under ONE table (mh_encode_frames_shared_device_async) against the table-per-frame
batch encoder, on 64 frames of 2048x1536 per region:

  (a) built mode: one histogram over the batch, one tree, every frame packed with its codes;
  (b) supplied mode with (a)'s header (no histogram reduction, no tree);
  (c) mh_encode_frames_device_async on the same frames: a tree per frame.

Two frame sets: 64 crops of a mirror-tiled BigBridge at 64 different origins (64 different
histograms: the case a shared table is for) and 64 BigBridge block shuffles (one histogram: the
per-frame tables coincide, so (a) and (c) write the same bytes). Also reported: the payload bytes
of (a) over (c) -- what sharing a table costs in compression -- and the downstream decode of each
output on the same box: mh_build_tables_device + mh_decode for (a)'s, mh_build_luts_device +
mh_decode_frames for (c)'s.

Regions are cold, as bench.py's: two resident sets of 64 frames alternate, and a 1 GiB device copy
evicts the Infinity Cache and the L2s before every region (bench.FLUSH), off the clock. The
launches of a region are enqueued behind bench.py's launch gate between two HIP events; the figure
is the events' distance. The arms alternate region by region. Before timing, (a)'s and (c)'s
outputs are decoded and compared with the inputs, and (b)'s bytes with (a)'s. Every line carries
the source stamp (library, mh_encode.hip, the loaded library).

    python scripts/bench_encode_shared.py [--out profiles/encode_shared_ab.txt] [--regions 15]

runs each step (distinct, shuffles) as a child process under its own `timeout`, stops at the first
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

N_FRAMES = 64
STEPS = {"distinct": 420, "shuffles": 420}  # step -> its time limit, seconds


def _stamp() -> str:
    import metalhuffman_amd as mh
    import metalhuffman_amd.build as B
    s = B.source_stamps()
    return f"[lib {s['lib']} mh_encode.hip {s['mh_encode.hip']} loaded {mh.lib().mh_build_stamp().decode()[:16]}]"


def _stats(us):
    import numpy as np
    return {"median_us": round(float(np.median(us)), 2), "min_us": round(float(min(us)), 2),
            "max_us": round(float(max(us)), 2), "regions": len(us), "us": [round(float(u), 2) for u in us]}


def _images(kind):
    """Two sets of 64 images."""
    import numpy as np
    from metalhuffman_amd import frames as F
    bb = F.bigbridge()
    h, w = bb.shape
    if kind == "shuffles":
        imgs = [F.block_shuffle(bb, 20000 + k) for k in range(2 * N_FRAMES)]
    else:
        src = F.mirror_tile(bb, 2 * h, 2 * w)
        imgs = [np.ascontiguousarray(src[37 * k % h:, 101 * k % w:][:h, :w]) for k in range(2 * N_FRAMES)]
    return [imgs[i:i + N_FRAMES] for i in (0, N_FRAMES)]


class _Outputs:
    """One arm's preallocated outputs (nothing is allocated inside a timed region)."""

    def __init__(self, enc, dev, per_frame):
        import torch
        n = enc.n
        self.codes = torch.empty(n * enc.slot, dtype=torch.uint8, device=dev)
        assert self.codes.data_ptr() % 16 == 0
        self.offs = torch.empty(n * enc.nb, dtype=torch.int32, device=dev)
        self.canon = torch.empty((n, 256) if per_frame else (256,), dtype=torch.uint8, device=dev)
        self.lens = torch.empty(n, dtype=torch.int64, device=dev)
        self.fco = torch.empty(n + 1, dtype=torch.int64, device=dev)
        self.status = torch.empty(n + 1, dtype=torch.int32, device=dev)

    def frames(self, enc, payload):
        from metalhuffman_amd.decoder import DeviceFrames
        return DeviceFrames(enc.width, enc.height, enc.n, self.offs, self.codes, self.fco, None, 0, payload)


def step(kind, regions):
    import numpy as np
    import torch
    import bench
    from metalhuffman_amd import _native as N
    from metalhuffman_amd import decoder as D
    from metalhuffman_amd.encoder import BatchEncoder
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if not bench.GATE.ok():
        raise SystemExit("bench_encode_shared: the launch gate (scripts/micro/liblaunch_gate.so) is not built")
    stamp = _stamp()
    L = N.lib()
    sets = _images(kind)
    h, w = sets[0][0].shape
    enc = BatchEncoder(w, h, N_FRAMES, dev)
    base = enc.workspace.data_ptr()
    ws = (base + 255) // 256 * 256
    ws_bytes = enc.workspace.numel() - (ws - base)
    stream = torch.cuda.current_stream(dev).cuda_stream
    flags = N.MH_ENCODE_WORKSPACE_ZEROED | N.MH_ENCODE_LIMIT_LENGTHS   # (a deep tree is limited, never rejected)
    S = []
    for imgs in sets:
        S.append({"gray": torch.from_numpy(np.stack(imgs)).to(dev), "a": _Outputs(enc, dev, False),
                  "b": _Outputs(enc, dev, False), "c": _Outputs(enc, dev, True),
                  "out": torch.empty((N_FRAMES, h, w), dtype=torch.uint8, device=dev)})

    def shared(s, o, canon_in):
        N.check(L.mh_encode_frames_shared_device_async(
            s["gray"].data_ptr(), h * w, N_FRAMES, w, h, flags, canon_in, o.canon.data_ptr(), o.codes.data_ptr(), enc.slot,
            o.lens.data_ptr(), o.fco.data_ptr(), o.offs.data_ptr(), None, o.status.data_ptr(),
            o.status.data_ptr() + 4 * N_FRAMES, ws, ws_bytes, stream), "mh_encode_frames_shared_device_async")

    def enc_a(s):
        shared(s, s["a"], None)

    def enc_b(s):
        shared(s, s["b"], s["a"].canon.data_ptr())

    def enc_c(s):
        o = s["c"]
        N.check(L.mh_encode_frames_device_async(
            s["gray"].data_ptr(), h * w, N_FRAMES, w, h, flags, o.canon.data_ptr(), o.codes.data_ptr(), enc.slot,
            o.lens.data_ptr(), o.fco.data_ptr(), o.offs.data_ptr(), None, o.status.data_ptr(), ws, ws_bytes, stream),
            "mh_encode_frames_device_async")

    def dec_a(s):
        D.decode(s["fa"], D.DeviceTables.from_canonical_header(s["a"].canon, dev), out=s["out"])

    def dec_c(s):
        D.decode_frames(s["fc"], D.DeviceTableSet.from_canonical_headers(s["c"].canon, dev), out=s["out"])

    # parity first (and the warm-up of every kernel)
    for s in S:
        for fn in (enc_a, enc_b, enc_c):
            fn(s)
        torch.cuda.synchronize(dev)
        for arm in "abc":
            if s[arm].status.any().item():
                raise SystemExit(f"bench_encode_shared: arm ({arm}) rejected a frame or its header ({kind})")
        s["payload"] = {arm: int(s[arm].lens.sum().item()) - N_FRAMES * N.MH_CODES_PAD for arm in "abc"}
        s["tables"] = len({bytes(r) for r in s["c"].canon.cpu().numpy()})
        if not (torch.equal(s["a"].lens, s["b"].lens) and torch.equal(s["a"].offs, s["b"].offs)
                and torch.equal(s["a"].canon, s["b"].canon)):
            raise SystemExit(f"bench_encode_shared: (b) differs from (a) ({kind})")
        for f in range(N_FRAMES):
            n = int(s["a"].lens[f].item())
            if not torch.equal(s["a"].codes[f * enc.slot: f * enc.slot + n], s["b"].codes[f * enc.slot: f * enc.slot + n]):
                raise SystemExit(f"bench_encode_shared: (b)'s codes differ from (a)'s in frame {f} ({kind})")
        s["fa"] = s["a"].frames(enc, s["payload"]["a"])
        s["fc"] = s["c"].frames(enc, s["payload"]["c"])
        for name, fn in (("a", dec_a), ("c", dec_c)):
            s["out"].fill_(0xA5)
            fn(s)
            torch.cuda.synchronize(dev)
            if not torch.equal(s["out"], s["gray"]):
                raise SystemExit(f"bench_encode_shared: the decode of ({name})'s output differs from the inputs ({kind})")
    arms = {"a": enc_a, "b": enc_b, "c": enc_c, "dec_a": dec_a, "dec_c": dec_c}
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
    res = {"step": kind, "device": torch.cuda.get_device_name(dev), "frames_per_region": N_FRAMES, "frame": [w, h],
           "source_stamp": stamp, "distinct_per_frame_tables": [s["tables"] for s in S],
           "payload_bytes": [s["payload"] for s in S], "arms": {k: _stats(v) for k, v in times.items()}}
    med = {k: v["median_us"] for k, v in res["arms"].items()}
    res["a_over_c"] = round(med["a"] / med["c"], 4)
    res["b_over_c"] = round(med["b"] / med["c"], 4)
    res["payload_a_over_c"] = [round(s["payload"]["a"] / s["payload"]["c"], 5) for s in S]
    label = {"a": "(a) shared table, built from the batch (5 launches)",
             "b": "(b) shared table, supplied header (4 launches)",
             "c": "(c) mh_encode_frames_device_async, a table per frame (3 launches)",
             "dec_a": "decode of (a): mh_build_tables_device + mh_decode",
             "dec_c": "decode of (c): mh_build_luts_device + mh_decode_frames"}
    lines = [f"[{kind}] 64 x 2048x1536, cold regions, HIP events, median (min..max) us over {regions} regions; "
             f"distinct per-frame tables in the two sets: {[s['tables'] for s in S]}"]
    for name in ("a", "b", "c", "dec_a", "dec_c"):
        v = res["arms"][name]
        lines.append(f"  {label[name]:<68} {v['median_us']:9.2f} ({v['min_us']:.2f} .. {v['max_us']:.2f})")
    lines.append(f"  (a)/(c) = {res['a_over_c']:.3f}   (b)/(c) = {res['b_over_c']:.3f}   "
                 f"encode + decode: shared {med['a'] + med['dec_a']:.2f}, per frame {med['c'] + med['dec_c']:.2f} us")
    lines.append(f"  payload bytes (a)/(c) in the two sets: {res['payload_a_over_c']} "
                 f"({[s['payload']['a'] for s in S]} / {[s['payload']['c'] for s in S]})")
    lines.append(json.dumps(res))
    for line in lines:
        print(f"{line}  {stamp}")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_shared_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        step(args.step, args.regions)
        return 0
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_encode_shared.py --regions {args.regions}   (library stamp "
            f"{B.library_stamp()[:16]})\n"]
    for name in ("distinct", "shuffles"):  # each under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(STEPS[name]), sys.executable, os.path.abspath(__file__), "--step", name,
               "--regions", str(args.regions)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)  # (stderr passes through)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"bench_encode_shared: step {name} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
        text.append(p.stdout)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
