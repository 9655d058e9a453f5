#!/usr/bin/env python3
"""Interleaved images straight into C-plane frames (mh_encode_images_device_async) against what a
caller had to do before, on 64 images of 2048x1536 with three planes taken (192 frames) per region:

  (a) the images entry on the [64, H, W, K] buffer, in place;
  (b) one permute(0, 3, 1, 2) copy into a planar buffer (preallocated: no allocation on the clock),
      then mh_encode_frames_device_async on it;
  (c) mh_encode_frames_device_async alone on already-planar data: not the same job -- the yardstick
      for what the strided fetch costs.

Steps: `rgb` (K = 3), `rgba` (K = 4, three planes taken), `rgb_shared` (K = 3 through the shared-table
entries, built mode), all on 4-byte aligned layouts (the dword loads), and `rgb_odd` (K = 3 with a row
pitch of 3 W + 1: the byte loads; reported, not gated). The gate: (a)/(b) < 0.96 on the aligned steps
-- 0.96 is the margin for the +-4 % box-to-box spread recorded in README.md -- against (b) measured in
the same run. (a)/(c) is reported.

Every plane of every image is a crop of a mirror-tiled BigBridge at its own origin. Regions are
cold, as bench.py's: two resident sets alternate, and a 1 GiB device copy evicts the Infinity Cache
and the L2s before every region (bench.FLUSH), off the clock. A region's launches are enqueued behind
bench.py's launch gate between two HIP events; the figure is the events' distance, the median
(min..max) of --regions regions. The arms alternate region by region. Before any timing, (a)'s
outputs are compared with (b)'s byte for byte and decoded back to the planes. Every line carries the
source stamp.

    python scripts/bench_encode_images.py [--out profiles/encode_images_ab.txt] [--regions 15]

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_IMAGES, C = 64, 3
STEPS = {"rgb": 420, "rgba": 420, "rgb_shared": 420, "rgb_odd": 420}  # step -> its time limit, seconds
GATED = ("rgb", "rgba", "rgb_shared")
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


def _plane_sets():
    """Two sets of 64 x 3 planes [n, C, H, W]."""
    import numpy as np
    from metalhuffman_amd import frames as F
    bb = F.bigbridge()
    h, w = bb.shape
    src = F.mirror_tile(bb, 2 * h, 2 * w)
    planes = [np.ascontiguousarray(src[37 * k % h:, 101 * k % w:][:h, :w]) for k in range(2 * N_IMAGES * C)]
    return [np.stack(planes[i:i + N_IMAGES * C]).reshape(N_IMAGES, C, h, w) for i in (0, N_IMAGES * C)]


class _Outputs:
    """One arm's preallocated outputs (nothing is allocated inside a timed region)."""

    def __init__(self, enc, dev, per_frame):
        import torch
        n = enc.n
        self.codes = torch.zeros(n * enc.slot, dtype=torch.uint8, device=dev)
        assert self.codes.data_ptr() % 16 == 0
        self.offs = torch.zeros(n * enc.nb, dtype=torch.int32, device=dev)
        self.canon = torch.zeros((n, 256) if per_frame else (256,), dtype=torch.uint8, device=dev)
        self.lens = torch.zeros(n, dtype=torch.int64, device=dev)
        self.fco = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        self.status = torch.zeros(n + 1, dtype=torch.int32, device=dev)

    def tensors(self):
        return (self.codes, self.offs, self.canon, self.lens, self.fco, self.status)


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
        raise SystemExit("bench_encode_images: the launch gate (scripts/micro/liblaunch_gate.so) is not built")
    stamp = _stamp()
    L = N.lib()
    sets = _plane_sets()
    h, w = sets[0].shape[2:]
    K = 4 if kind == "rgba" else 3
    pitch = w * K + (1 if kind == "rgb_odd" else 0)
    shared = kind == "rgb_shared"
    n = N_IMAGES * C
    enc = BatchEncoder(w, h, n, dev)
    base = enc.workspace.data_ptr()
    ws = (base + 255) // 256 * 256
    ws_bytes = enc.workspace.numel() - (ws - base)
    stream = torch.cuda.current_stream(dev).cuda_stream
    flags = N.MH_ENCODE_WORKSPACE_ZEROED | N.MH_ENCODE_LIMIT_LENGTHS   # (a deep tree is limited, never rejected)
    lay = N.mh_image_layout(h * pitch, pitch, K, 0, C, 0)
    S = []
    for planes in sets:
        rows = torch.zeros((N_IMAGES, h, pitch), dtype=torch.uint8, device=dev)
        pix = rows[:, :, :w * K].view(N_IMAGES, h, w, K)             # the interleaved images, rows `pitch` apart
        pix[..., :C].copy_(torch.from_numpy(planes).to(dev).permute(0, 2, 3, 1))
        if K > C:
            pix[..., C:] = 0xFF                                       # alpha
        S.append({"pix": pix, "planar": torch.from_numpy(planes).to(dev).contiguous(),
                  "copy": torch.empty((N_IMAGES, C, h, w), dtype=torch.uint8, device=dev),
                  "a": _Outputs(enc, dev, not shared), "b": _Outputs(enc, dev, not shared),
                  "c": _Outputs(enc, dev, not shared),
                  "out": torch.empty((n, h, w), dtype=torch.uint8, device=dev)})
        assert pix.data_ptr() % 256 == 0 and pix.stride() == (h * pitch, pitch, K, 1)

    def frames_entry(gray, o):
        if shared:
            N.check(L.mh_encode_frames_shared_device_async(
                gray.data_ptr(), h * w, n, w, h, flags, None, o.canon.data_ptr(), o.codes.data_ptr(), enc.slot,
                o.lens.data_ptr(), o.fco.data_ptr(), o.offs.data_ptr(), None, o.status.data_ptr(),
                o.status.data_ptr() + 4 * n, ws, ws_bytes, stream), "mh_encode_frames_shared_device_async")
        else:
            N.check(L.mh_encode_frames_device_async(
                gray.data_ptr(), h * w, n, w, h, flags, o.canon.data_ptr(), o.codes.data_ptr(), enc.slot,
                o.lens.data_ptr(), o.fco.data_ptr(), o.offs.data_ptr(), None, o.status.data_ptr(), ws, ws_bytes, stream),
                "mh_encode_frames_device_async")

    def enc_a(s):
        o = s["a"]
        if shared:
            N.check(L.mh_encode_images_shared_device_async(
                s["pix"].data_ptr(), ctypes.byref(lay), N_IMAGES, w, h, flags, None, o.canon.data_ptr(),
                o.codes.data_ptr(), enc.slot, o.lens.data_ptr(), o.fco.data_ptr(), o.offs.data_ptr(), None,
                o.status.data_ptr(), o.status.data_ptr() + 4 * n, ws, ws_bytes, stream),
                "mh_encode_images_shared_device_async")
        else:
            N.check(L.mh_encode_images_device_async(
                s["pix"].data_ptr(), ctypes.byref(lay), N_IMAGES, w, h, flags, o.canon.data_ptr(), o.codes.data_ptr(),
                enc.slot, o.lens.data_ptr(), o.fco.data_ptr(), o.offs.data_ptr(), None, o.status.data_ptr(), ws,
                ws_bytes, stream), "mh_encode_images_device_async")

    def enc_b(s):
        s["copy"].copy_(s["pix"][..., :C].permute(0, 3, 1, 2))        # what .contiguous() launches
        frames_entry(s["copy"], s["b"])

    def enc_c(s):
        frames_entry(s["planar"], s["c"])

    # byte identity of (a) and (b) first (and the warm-up of every kernel), then a decode of (a)
    for s in S:
        for fn in (enc_a, enc_b, enc_c):
            fn(s)
        torch.cuda.synchronize(dev)
        for arm in "abc":
            if s[arm].status.any().item():
                raise SystemExit(f"bench_encode_images: arm ({arm}) rejected a frame or its header ({kind})")
        if not torch.equal(s["copy"], s["planar"]):
            raise SystemExit(f"bench_encode_images: the interleaved buffer does not hold the planes ({kind})")
        for name, x, y in zip(("codes", "offsets", "headers", "lengths", "frame offsets", "status"),
                              s["a"].tensors(), s["b"].tensors()):
            if not torch.equal(x, y):
                raise SystemExit(f"bench_encode_images: (a)'s {name} differ from (b)'s ({kind})")
        payload = int(s["a"].lens.sum().item()) - n * N.MH_CODES_PAD
        fr = D.DeviceFrames(w, h, n, s["a"].offs, s["a"].codes, s["a"].fco, None, 0, payload)
        s["out"].fill_(0xA5)
        if shared:
            D.decode(fr, D.DeviceTables.from_canonical_header(s["a"].canon, dev), out=s["out"])
        else:
            D.decode_frames(fr, D.DeviceTableSet.from_canonical_headers(s["a"].canon, dev), out=s["out"])
        torch.cuda.synchronize(dev)
        if not torch.equal(s["out"].view(N_IMAGES, C, h, w), s["planar"]):
            raise SystemExit(f"bench_encode_images: the decode of (a)'s output differs from the planes ({kind})")
    arms = {"a": enc_a, "b": enc_b, "c": enc_c}
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
           "pixel_stride": K, "row_pitch": pitch, "frame": [w, h], "entry": "shared, built" if shared else "per-frame tables",
           "loads": "bytes" if kind == "rgb_odd" else "dwords", "source_stamp": stamp,
           "arms": {k: _stats(v) for k, v in times.items()}}
    med = {k: v["median_us"] for k, v in res["arms"].items()}
    res["a_over_b"] = round(med["a"] / med["b"], 4)
    res["a_over_c"] = round(med["a"] / med["c"], 4)
    res["gated"] = kind in GATED
    label = {"a": "(a) images entry, in place", "b": "(b) permute copy + frames entry",
             "c": "(c) frames entry on planar data (not the same job)"}
    lines = [f"[{kind}] 64 x 2048x1536 x {C} planes of {K}-byte pixels, pitch {pitch} ({res['loads']}), {res['entry']}; "
             f"cold regions, HIP events, median (min..max) us over {regions} regions"]
    for name in "abc":
        v = res["arms"][name]
        lines.append(f"  {label[name]:<56} {v['median_us']:9.2f} ({v['min_us']:.2f} .. {v['max_us']:.2f})   "
                     f"{v['median_us'] / n:.2f} us per frame")
    verdict = "reported, not gated" if kind not in GATED else \
        f"gate (a)/(b) < {GATE}: {'pass' if res['a_over_b'] < GATE else 'FAIL'}"
    lines.append(f"  (a)/(b) = {res['a_over_b']:.3f}   (a)/(c) = {res['a_over_c']:.3f}   {verdict}")
    lines.append(json.dumps(res))
    for line in lines:
        print(f"{line}  {stamp}")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_images_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        step(args.step, args.regions)
        return 0
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_encode_images.py --regions {args.regions}   (library stamp "
            f"{B.library_stamp()[:16]})\n"]
    ratios = {}
    for name in ("rgb", "rgba", "rgb_shared", "rgb_odd"):  # each under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(STEPS[name]), sys.executable, os.path.abspath(__file__), "--step", name,
               "--regions", str(args.regions)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)  # (stderr passes through)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"bench_encode_images: step {name} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
        text.append(p.stdout)
        ratios[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1].rsplit("  [", 1)[0])["a_over_b"]
    failed = [k for k in GATED if not ratios[k] < GATE]
    verdict = (f"GATE (a)/(b) < {GATE} on {', '.join(GATED)}: " +
               ("pass" if not failed else f"FAIL on {', '.join(failed)}") +
               " -- " + ", ".join(f"{k} {ratios[k]:.3f}" for k in ratios))
    print(verdict)
    text.append(verdict + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
