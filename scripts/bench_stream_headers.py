#!/usr/bin/env python3
"""Frames with a Huffman table each, streamed from pinned host memory (2 slots), by bench.py's
stream_h2d method -- a sustained phase (frames back to back, frames/s) and a paced phase (one
frame in flight, device latency H2D start -> decode end from the slot's events, p50 / p99):

  (a) the header-mode stream (mh_stream_create_headers): one DMA (header | offsets | codes) and one
      mh_decode_headers launch per frame, direct (its default);
  (b) the route a user had before it, assembled here from public entries: per frame, on the slot's
      stream, one DMA of offsets | codes plus a 256-byte header copy, then
      mh_build_luts_device(n = 1) and mh_decode_frames(n = 1), direct launches;
  (c) the shared-table stream (mh_stream_create) on block shuffles of one image: the floor;
  (g) (a) created under MH_STREAM_GRAPHS=1: the same launch replayed from the slot's graph;
  (h) (a)'s copies and launch assembled here from public entries, as a cross-check of (a).
The stream keeps mh_decode_headers unless (a)'s paced device latency p50 is worse than (b)'s by more
than the +-4 % box-to-box spread. (Earlier libraries whose slot replayed a graph of one launch, and
of (b)'s two launches: profiles/stream_headers_ab_one_launch.txt, stream_headers_ab_two_launch.txt.)

(a) and (b) stream 2048x1536 crops of a mirror-tiled BigBridge with distinct headers (crops with a
tile over the kernels' LDS window are passed over, as bench_multitable.py's distinct_fit); (c)
streams block shuffles of BigBridge. The routes alternate region by region; a figure is the
median (min .. max) over the regions. Every route's output is compared with the encoder inputs
before timing.

Step `resident`, by bench_multitable.py's method (cold regions, launch gate, HIP events, 64 crops
resident in HBM): mh_decode_headers against mh_build_luts_device + mh_decode_frames (both launches
between the events) and against mh_decode_frames alone (tables prepared beforehand).

    python scripts/bench_stream_headers.py [--out profiles/stream_headers_ab.txt] [--regions 15]

runs each step as a child process under its own `timeout`, stops at the first failure and writes
what the steps printed to --out. `--step NAME` runs one step here.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

STEPS = {"stream": 420, "resident": 300}  # step -> its time limit, seconds
N_HOST = 32        # distinct frames in pinned host memory per route
N_SUSTAINED = 512  # frames per region, back to back
N_PACED = 128      # frames per region, one in flight


def _stats(v, nd=2):
    import numpy as np
    return {"median": round(float(np.median(v)), nd), "min": round(float(min(v)), nd), "max": round(float(max(v)), nd),
            "regions": len(v), "all": [round(float(x), nd) for x in v]}


class _Hip:
    """The few HIP runtime calls route (b) needs, through ctypes, from the HIP runtime this
    process already runs on (the one torch and the decoder library loaded)."""

    def __init__(self):
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64.so" in line:
                    path = line.split()[-1]
                    break
        if path is None:
            raise SystemExit("bench_stream_headers: no HIP runtime is loaded in this process")
        L = ctypes.CDLL(path)
        vp = ctypes.c_void_p
        L.hipMemcpyAsync.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
        L.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(vp), ctypes.c_uint]
        L.hipStreamSynchronize.argtypes = [vp]
        L.hipStreamDestroy.argtypes = [vp]
        L.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
        L.hipEventRecord.argtypes = [vp, vp]
        L.hipEventSynchronize.argtypes = [vp]
        L.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
        L.hipEventDestroy.argtypes = [vp]
        self.L = L

    def ok(self, rc, what):
        if rc != 0:
            raise SystemExit(f"bench_stream_headers: {what} failed (hipError {rc})")


class TwoLaunchStream:
    """Routes (b) and (h): 2 slots, each with its own stream, events and buffers. (b): a submit is
    two copies, mh_build_luts_device(n = 1) and mh_decode_frames(n = 1) on the slot's stream; (h),
    `headers`: one copy (the slot buffer is header | offsets | codes) and mh_decode_headers."""

    def __init__(self, width, height, cap, device, slots=2, headers=False):
        self.headers = headers
        import torch
        from metalhuffman_amd import _native as N
        self.hip, self.N, self.L = _Hip(), N, N.lib()
        self.w, self.h, self.pitch = width, height, (width + 7) // 8 * 8
        nb = ((width + 7) // 8) * ((height + 7) // 8)
        self.ob = (nb * 4 + 15) // 16 * 16
        self.cap = (cap + 15) // 16 * 16
        self.stride = (int(self.L.mh_lut_bytes()) + 15) // 16 * 16
        self.slots = []
        for _ in range(slots):
            whole = torch.zeros(256 + self.ob + self.cap, dtype=torch.uint8, device=device)
            s = {"whole": whole, "base": whole[256:], "hdr": whole[:256],
                 "lut": torch.zeros(self.stride, dtype=torch.uint8, device=device),
                 "status": torch.zeros(1, dtype=torch.int32, device=device),
                 "out": torch.zeros((height, self.pitch), dtype=torch.uint8, device=device)}
            st, e0, e1 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
            self.hip.ok(self.hip.L.hipStreamCreateWithFlags(ctypes.byref(st), 1), "hipStreamCreateWithFlags")
            self.hip.ok(self.hip.L.hipEventCreate(ctypes.byref(e0)), "hipEventCreate")
            self.hip.ok(self.hip.L.hipEventCreate(ctypes.byref(e1)), "hipEventCreate")
            fr = N.mh_frame()
            fr.d_block_offsets = s["base"].data_ptr()
            fr.d_codes = s["base"].data_ptr() + self.ob
            fr.codes_bytes = self.cap
            fr.dims = N.mh_dims(width, height, (width + 7) // 8, (height + 7) // 8)
            fr.n_frames = 1
            s.update(stream=st, start=e0, done=e1, frame=fr)
            self.slots.append(s)
        torch.cuda.synchronize(device)
        self.next = 0

    def submit(self, header, codes, offsets):
        """header u8[256] pinned; codes / offsets: pinned_frame's views (one buffer, offsets | codes)."""
        k = self.next
        s, H, L = self.slots[k], self.hip.L, self.L
        st = s["stream"]
        H.hipEventRecord(s["start"], st)
        if self.headers:  # header | offsets | codes: pinned_frame_with_header's buffer
            self.hip.ok(H.hipMemcpyAsync(s["whole"].data_ptr(), header.data_ptr(), 256 + self.ob + codes.numel(), 1,
                                         st), "hipMemcpyAsync")
            self.N.check(L.mh_decode_headers(ctypes.byref(s["frame"]), s["hdr"].data_ptr(), None,
                                             s["status"].data_ptr(), s["out"].data_ptr(), self.pitch,
                                             self.h * self.pitch, st), "mh_decode_headers")
            H.hipEventRecord(s["done"], st)
            self.next = (k + 1) % len(self.slots)
            return k
        rc = H.hipMemcpyAsync(s["base"].data_ptr(), offsets.data_ptr(), self.ob + codes.numel(), 1, st)
        rc |= H.hipMemcpyAsync(s["hdr"].data_ptr(), header.data_ptr(), 256, 1, st)
        self.hip.ok(rc, "hipMemcpyAsync")
        self.N.check(L.mh_build_luts_device(s["hdr"].data_ptr(), 1, s["lut"].data_ptr(), self.stride,
                                            s["status"].data_ptr(), st), "mh_build_luts_device")
        self.N.check(L.mh_decode_frames(ctypes.byref(s["frame"]), s["lut"].data_ptr(), self.stride,
                                        s["status"].data_ptr(), s["out"].data_ptr(), self.pitch,
                                        self.h * self.pitch, st), "mh_decode_frames")
        H.hipEventRecord(s["done"], st)
        self.next = (k + 1) % len(self.slots)
        return k

    def wait(self, k):
        self.hip.ok(self.hip.L.hipEventSynchronize(self.slots[k]["done"]), "hipEventSynchronize")

    def slot_time_ms(self, k):
        ms = ctypes.c_float(0)
        self.wait(k)
        self.hip.ok(self.hip.L.hipEventElapsedTime(ctypes.byref(ms), self.slots[k]["start"], self.slots[k]["done"]),
                    "hipEventElapsedTime")
        return float(ms.value)

    def output(self, k):
        return self.slots[k]["out"]

    def synchronize(self):
        for s in self.slots:
            self.hip.ok(self.hip.L.hipStreamSynchronize(s["stream"]), "hipStreamSynchronize")

    def close(self):
        self.synchronize()
        for s in self.slots:
            self.hip.L.hipEventDestroy(s["start"])
            self.hip.L.hipEventDestroy(s["done"])
            self.hip.L.hipStreamDestroy(s["stream"])
        self.slots = []


def _distinct_crops(n):
    import numpy as np
    import metalhuffman_amd as mh
    from metalhuffman_amd import frames as F
    from bench_multitable import _oversize_tiles
    bb = F.bigbridge()
    h, w = bb.shape
    src = F.mirror_tile(bb, 2 * h, 2 * w)
    imgs, efs, k = [], [], 0
    while len(imgs) < n:
        im = np.ascontiguousarray(src[37 * k % h:, 101 * k % w:][:h, :w])
        k += 1
        try:
            ef = mh.encode_frame(im)
        except mh.MHError:
            continue
        if _oversize_tiles(ef):
            continue
        efs.append(ef)
        imgs.append(im)
    assert len({ef.canon.tobytes() for ef in efs}) == n
    return imgs, efs


def step_stream(regions):
    import numpy as np
    import torch
    import bench
    from metalhuffman_amd import decoder as D
    from metalhuffman_amd import frames as F
    from metalhuffman_amd.stream import FrameStream, HeaderFrameStream, pinned_frame, pinned_frame_with_header
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    imgs, efs = _distinct_crops(N_HOST)
    bb = F.bigbridge()
    H, W = bb.shape
    sh_imgs = [F.block_shuffle(bb, 30000 + k) for k in range(N_HOST)]
    sh_efs = bench.encode_many(sh_imgs)
    assert all(np.array_equal(ef.canon, sh_efs[0].canon) for ef in sh_efs)
    tabs = D.DeviceTables.upload(*sh_efs[0].tables(), dev)
    cap = max(ef.codes.size for ef in efs + sh_efs)
    a = HeaderFrameStream(W, H, cap, slots=2, device=dev)
    os.environ["MH_STREAM_GRAPHS"] = "1"  # read when a stream is created
    g = HeaderFrameStream(W, H, cap, slots=2, device=dev)
    del os.environ["MH_STREAM_GRAPHS"]
    b = TwoLaunchStream(W, H, cap, dev)
    c = FrameStream(tabs, W, H, cap, slots=2, device=dev)
    hh = TwoLaunchStream(W, H, cap, dev, headers=True)
    host_a = [pinned_frame_with_header(ef) for ef in efs]
    host_b = [(torch.from_numpy(np.ascontiguousarray(ef.canon)).pin_memory(),) + pinned_frame(ef) for ef in efs]
    host_c = [pinned_frame(ef) for ef in sh_efs]
    routes = {"a": (a, host_a, imgs), "b": (b, host_b, imgs), "c": (c, host_c, sh_imgs), "h": (hh, host_a, imgs),
              "g": (g, host_a, imgs)}
    for name, (s, hosts, ref) in routes.items():  # parity first (and the warm-up)
        for i, hst in enumerate(hosts):
            k = s.submit(*hst)
            s.wait(k)
            if not np.array_equal(s.output(k)[:, :W].cpu().numpy(), ref[i]):
                raise SystemExit(f"bench_stream_headers: route ({name}) frame {i} differs from the encoder input")
    fps = {n: [] for n in routes}
    p50 = {n: [] for n in routes}
    p99 = {n: [] for n in routes}
    host50 = {n: [] for n in routes}
    for r in range(regions + 1):  # region 0 of every route is a rehearsal, not recorded
        for name in sorted(routes):
            s, hosts, _ = routes[name]
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(N_SUSTAINED):
                s.submit(*hosts[i % N_HOST])
            s.synchronize()
            wall = time.perf_counter() - t0
            dl, hl = [], []
            for i in range(N_PACED):
                t = time.perf_counter()
                k = s.submit(*hosts[i % N_HOST])
                s.wait(k)
                hl.append((time.perf_counter() - t) * 1e6)
                dl.append(s.slot_time_ms(k) * 1e3)
            if r:
                fps[name].append(N_SUSTAINED / wall)
                p50[name].append(float(np.percentile(dl, 50)))
                p99[name].append(float(np.percentile(dl, 99)))
                host50[name].append(float(np.percentile(hl, 50)))
    for s, _, _ in routes.values():
        s.close()
    res = {"step": "stream", "device": torch.cuda.get_device_name(dev), "frame": [W, H], "slots": 2,
           "host_frames": N_HOST, "sustained_frames_per_region": N_SUSTAINED, "paced_frames_per_region": N_PACED,
           "h2d_bytes_per_frame": {"a_b": int(np.mean([ef.codes.size + 4 * ef.n_blocks + 256 for ef in efs])),
                                   "c": int(np.mean([ef.codes.size + 4 * ef.n_blocks for ef in sh_efs]))},
           "routes": {n: {"sustained_fps": _stats(fps[n], 1), "device_latency_us_p50": _stats(p50[n]),
                          "device_latency_us_p99": _stats(p99[n]), "host_latency_us_p50": _stats(host50[n])}
                      for n in sorted(routes)}}
    ma, mb, mh1 = (res["routes"][n]["device_latency_us_p50"]["median"] for n in "abh")
    res["a_over_b_device_p50"] = round(ma / mb, 4)
    res["h_over_b_device_p50"] = round(mh1 / mb, 4)
    res["stream_keeps_mh_decode_headers"] = bool(ma <= mb * 1.04)
    label = {"a": "(a) header-mode stream: 1 DMA + mh_decode_headers, direct",
             "g": "(g) ... the same launch replayed from the slot's graph",
             "b": "(b) 2 copies + mh_build_luts_device + mh_decode_frames",
             "c": "(c) shared-table stream on block shuffles (floor)",
             "h": "(h) (a) assembled in this script"}
    print(f"[stream] 2048x1536, 2 slots, median (min .. max) over {regions} regions; sustained: {N_SUSTAINED} "
          f"frames back to back; paced: {N_PACED} frames, one in flight")
    for n in sorted(routes):
        v = res["routes"][n]
        f, d, q, hh = (v[k] for k in ("sustained_fps", "device_latency_us_p50", "device_latency_us_p99",
                                      "host_latency_us_p50"))
        print(f"  {label[n]:<60} {f['median']:8.1f} ({f['min']:.1f} .. {f['max']:.1f}) frames/s   device p50 "
              f"{d['median']:7.2f} ({d['min']:.2f} .. {d['max']:.2f}) us   p99 {q['median']:7.2f} "
              f"({q['min']:.2f} .. {q['max']:.2f}) us   host p50 {hh['median']:7.2f} us")
    print(f"  paced device latency p50: (a)/(b) = {res['a_over_b_device_p50']:.3f}   (h)/(b) = "
          f"{res['h_over_b_device_p50']:.3f} -> the stream "
          f"{'keeps mh_decode_headers' if res['stream_keeps_mh_decode_headers'] else 'should replay two launches'}"
          f" (rule: (a) no worse than (b) by more than 4 %)")
    print(json.dumps(res))


def step_resident(regions):
    import numpy as np
    import torch
    import bench
    from bench_multitable import N_FRAMES, _frame_sets
    from metalhuffman_amd import _native as N
    from metalhuffman_amd import decoder as D
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if not bench.GATE.ok():
        raise SystemExit("bench_stream_headers: the launch gate (scripts/micro/liblaunch_gate.so) is not built")
    L = N.lib()
    stride = (int(L.mh_lut_bytes()) + 15) // 16 * 16
    sets = []
    for imgs, efs in _frame_sets("distinct_fit"):
        s = {"ref": torch.from_numpy(np.stack(imgs)).to(dev),
             "batch": D.DeviceFrames.pack(efs, dev, shared_table=False),
             "hdr": torch.from_numpy(np.stack([ef.canon for ef in efs])).to(dev),
             "tset": D.DeviceTableSet.from_canonical_headers(np.stack([ef.canon for ef in efs]), dev),
             "luts": torch.empty((N_FRAMES, stride), dtype=torch.uint8, device=dev),
             "status": torch.empty(N_FRAMES, dtype=torch.int32, device=dev),
             "out": torch.empty((N_FRAMES, efs[0].height, efs[0].width), dtype=torch.uint8, device=dev)}
        s["tset"].check_status()
        s["tset2"] = D.DeviceTableSet(s["luts"], s["status"])
        sets.append(s)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def route_h(s):
        D.decode_headers(s["batch"], s["hdr"], out=s["out"])

    def route_lf(s):
        N.check(L.mh_build_luts_device(s["hdr"].data_ptr(), N_FRAMES, s["luts"].data_ptr(), stride,
                                       s["status"].data_ptr(), stream), "mh_build_luts_device")
        D.decode_frames(s["batch"], s["tset2"], out=s["out"])

    def route_f(s):
        D.decode_frames(s["batch"], s["tset"], out=s["out"])

    routes = {"h": route_h, "lf": route_lf, "f": route_f}
    for name, fn in sorted(routes.items()):
        for s in sets:
            s["out"].fill_(0xA5)
            fn(s)
            torch.cuda.synchronize(dev)
            if not torch.equal(s["out"], s["ref"]):
                raise SystemExit(f"bench_stream_headers: resident route ({name}) differs from the encoder inputs")
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
    gh = D.decode_headers_shape(sets[0]["batch"])
    gf = D.decode_frames_shape(sets[0]["batch"])
    res = {"step": "resident", "device": torch.cuda.get_device_name(dev), "frames_per_region": N_FRAMES,
           "frame": [sets[0]["batch"].width, sets[0]["batch"].height],
           "shape_headers": list(gh), "shape_frames": list(gf),
           "routes_us": {name: _stats(us) for name, us in times.items()}}
    med = {k: v["median"] for k, v in res["routes_us"].items()}
    res["h_over_lf"] = round(med["h"] / med["lf"], 4)
    res["h_over_f"] = round(med["h"] / med["f"], 4)
    print(f"[resident] 64 x 2048x1536 distinct-header crops without an oversize tile, cold regions, launch gate, "
          f"HIP events, median (min .. max) us over {regions} regions:")
    label = {"h": "mh_decode_headers (one launch, tables built in LDS)",
             "lf": "mh_build_luts_device + mh_decode_frames (both launches)",
             "f": "mh_decode_frames alone (tables prepared beforehand)"}
    for name in ("h", "lf", "f"):
        v = res["routes_us"][name]
        print(f"  {label[name]:<62} {v['median']:9.2f} ({v['min']:.2f} .. {v['max']:.2f})")
    print(f"  headers / (luts + frames) = {res['h_over_lf']:.3f}   headers / frames alone = {res['h_over_f']:.3f}   "
          f"workgroups per frame: headers {gh[0]}, frames {gf[0]}")
    print(json.dumps(res))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_headers_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        step_stream(args.regions) if args.step == "stream" else step_resident(args.regions)
        return 0
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_stream_headers.py --regions {args.regions}   (library stamp "
            f"{B.library_stamp()[:16]})\n"]
    for step in ("stream", "resident"):  # each under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--regions", str(args.regions)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)  # (stderr passes through)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"bench_stream_headers: step {step} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
        text.append(p.stdout)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
