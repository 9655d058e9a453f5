#!/usr/bin/env python3
"""What MH_ENCODE_LIMIT_LENGTHS costs, on 2048x1536 frames: the batched encode of 64 frames
(mh_encode_frames_device_async, one region = one call) and the single-frame encode
(mh_encode_frame_device_async, one region = one frame, the fused two-launch path).

  step `ordinary`: frames that need no limiting (64 BigBridge block shuffles per set), three routes:
      (p) the parent commit's library, which has no such flag (--parent, skipped when absent);
      (0) this library, flag off;  (1) this library, flag on.
      The limiter is behind a workgroup-uniform branch, so (1) adds one counting barrier to
      the tree workgroup and (0) nothing.
  step `deep`: frames that all need it (64 block shuffles per set of a frame holding 30 Fibonacci
      symbols, 2.18 M of its 3.1 M symbols; its Huffman tree is 29 deep) against the ordinary
      frames, both with the flag, in the same run. The difference also holds what the other
      data costs in the split and the packing, so it is an upper bound of the limiter's cost;
      per frame it is the batched difference / 64 (the 64 tree workgroups run side by side), per
      tree workgroup the single-frame difference (one tree on the critical path).

Method, as scripts/bench_multitable.py: cold regions (two resident sets alternate, bench.FLUSH
evicts the Infinity Cache and the L2s before every region, off the clock), the region's launches
enqueued behind bench.py's launch gate between two HIP events, the routes alternating region by
region, median (min .. max) of --regions regions after one rehearsal. Before timing, every route's
output is compared: the routes of `ordinary` with each other, frame 0 of `deep` with the host codec.

    python scripts/bench_limit_lengths.py [--out profiles/limit_lengths_ab.txt] [--regions 15]
                                          [--parent ab/lib_parent.so]

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_FRAMES = 64
W, H = 2048, 1536
STEPS = {"ordinary": 400, "deep": 400}  # step -> its time limit, seconds
LIMIT = 0x200
ZEROED = 0x100


def _stats(us):
    import numpy as np
    return {"median_us": round(float(np.median(us)), 2), "min_us": round(float(min(us)), 2),
            "max_us": round(float(max(us)), 2), "regions": len(us), "us": [round(float(u), 2) for u in us]}


def _bind(L):
    vp, u32, u64, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
    L.mh_encode_workspace_bytes.argtypes = [u32, u32]
    L.mh_encode_workspace_bytes.restype = sz
    L.mh_encode_frames_workspace_bytes.argtypes = [u32, u32, u32]
    L.mh_encode_frames_workspace_bytes.restype = sz
    L.mh_encode_frame_device_async.argtypes = [vp, u32, u32, u32, vp, vp, u64, vp, vp, vp, vp, vp, sz, vp]
    L.mh_encode_frames_device_async.argtypes = [vp, u64, u32, u32, u32, u32, vp, vp, u64, vp, vp, vp, vp, vp, vp, sz,
                                                vp]
    return L


class Enc:
    """One library's encoders for W x H with their own workspaces and outputs (reused region after region)."""

    def __init__(self, L, dev):
        import torch
        self.L, self.dev = L, dev
        nb = (W // 8) * (H // 8)
        self.nb = nb
        self.slot = (nb * 64 * 2 + 4 + 15) // 16 * 16 + 16
        z = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device=dev)
        self.bws = z(int(L.mh_encode_frames_workspace_bytes(W, H, N_FRAMES)) + 256)
        self.sws = z(int(L.mh_encode_workspace_bytes(W, H)) + 256)
        self.codes = z(N_FRAMES * self.slot + 16)
        self.offs = z(N_FRAMES * nb, torch.int32)
        self.canon = z(N_FRAMES * 256)
        self.lens = z(N_FRAMES, torch.int64)
        self.fco = z(N_FRAMES + 1, torch.int64)
        self.status = z(N_FRAMES, torch.int32)

    @staticmethod
    def _al(t, a):
        return (t.data_ptr() + a - 1) // a * a

    def batch(self, grays, flags, stream):
        ws = self._al(self.bws, 256)
        rc = self.L.mh_encode_frames_device_async(
            grays.data_ptr(), W * H, N_FRAMES, W, H, flags | ZEROED, self.canon.data_ptr(), self._al(self.codes, 16),
            self.slot, self.lens.data_ptr(), self.fco.data_ptr(), self.offs.data_ptr(), None, self.status.data_ptr(),
            ws, self.bws.numel() - (ws - self.bws.data_ptr()), stream)
        assert rc == 0, rc

    def single(self, gray, flags, stream):
        ws = self._al(self.sws, 256)
        rc = self.L.mh_encode_frame_device_async(
            gray.data_ptr(), W, H, flags | ZEROED, self.canon.data_ptr(), self._al(self.codes, 16), self.slot,
            self.lens.data_ptr(), self.offs.data_ptr(), None, self.status.data_ptr(), ws,
            self.sws.numel() - (ws - self.sws.data_ptr()), stream)
        assert rc == 0, rc

    def snapshot(self, n):
        """(status, byte counts, headers, code bytes, offsets) of the first n frames, on the host."""
        import torch
        torch.cuda.synchronize(self.dev)
        base = self._al(self.codes, 16) - self.codes.data_ptr()
        lens = self.lens[:n].cpu().numpy()
        codes = [self.codes[base + f * self.slot: base + f * self.slot + int(lens[f])].cpu().numpy() for f in range(n)]
        return (self.status[:n].cpu().numpy(), lens, self.canon[: n * 256].cpu().numpy(), codes,
                self.offs[: n * self.nb].cpu().numpy())


def _same(a, b) -> bool:
    import numpy as np
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            and all(np.array_equal(x, y) for x, y in zip(a[3], b[3])) and np.array_equal(a[4], b[4]))


def deep_frame(seed=30):
    """A 2048 x 1536 frame whose deltas hold 30 symbols with Fibonacci counts (2,178,308 symbols, the
    largest count on symbol 0, which also takes the rest of the frame and opens every block)."""
    import numpy as np
    counts, a, b = [], 1, 1
    for _ in range(30):
        counts.append(a)
        a, b = b, a + b
    r = np.random.default_rng(seed)
    syms = np.concatenate([[0], 1 + r.permutation(255)[:29]])
    f = np.zeros(256, np.int64)
    f[syms] = counts[::-1]
    nb = (W // 8) * (H // 8)
    f[0] += nb * 64 - int(f.sum()) - nb
    body = np.repeat(np.arange(256, dtype=np.uint8), f)
    r.shuffle(body)
    sym = np.zeros((nb, 64), np.uint16)
    sym[:, 1:] = body.reshape(nb, 63)
    vals = (np.cumsum(sym, axis=1) & 0xFF).astype(np.uint8)
    return np.ascontiguousarray(vals.reshape(H // 8, W // 8, 8, 8).transpose(0, 2, 1, 3).reshape(H, W))


def _sets(kind, dev):
    """Two resident sets of 64 frames [64, H, W] on the device (block shuffles: one histogram each kind)."""
    import numpy as np
    import torch
    from metalhuffman_amd import frames as F
    src = F.bigbridge() if kind == "ordinary" else deep_frame()
    assert src.shape == (H, W)
    imgs = [F.block_shuffle(src, 31000 + k) for k in range(2 * N_FRAMES)]
    return imgs, [torch.from_numpy(np.stack(imgs[i:i + N_FRAMES])).to(dev) for i in (0, N_FRAMES)]


def _time(routes, regions, dev):
    import torch
    import bench
    stream = torch.cuda.current_stream(dev).cuda_stream
    times = {name: [] for name in routes}
    for r in range(regions + 1):  # region 0 of every route is a rehearsal, not recorded
        for name in sorted(routes):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            bench.FLUSH(dev)
            torch.cuda.synchronize(dev)
            bench.GATE.arm(stream)
            e0.record()
            routes[name](r, stream)
            e1.record()
            bench.GATE.open()
            torch.cuda.synchronize(dev)
            if r:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    return {name: _stats(us) for name, us in times.items()}


def _setup(parent):
    import torch
    import bench
    import metalhuffman_amd as mh
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if not bench.GATE.ok():
        raise SystemExit("bench_limit_lengths: the launch gate (scripts/micro/liblaunch_gate.so) is not built")
    new = Enc(_bind(ctypes.CDLL(mh.LIB_PATH)), dev)
    old = Enc(_bind(ctypes.CDLL(os.path.abspath(parent))), dev) if parent and os.path.exists(parent) else None
    return dev, new, old


def _print(title, res, labels):
    print(title)
    for mode in ("batch", "single"):
        for name in sorted(res[mode]):
            v = res[mode][name]
            print(f"  {mode:<6} {labels[name]:<58} {v['median_us']:9.2f} ({v['min_us']:.2f} .. {v['max_us']:.2f})")


def step_ordinary(regions, parent):
    import torch
    dev, new, old = _setup(parent)
    imgs, sets = _sets("ordinary", dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    encs = {"0": (new, 0), "1": (new, LIMIT)}
    if old is not None:
        encs["p"] = (old, 0)
    snaps = {}
    for name, (e, fl) in encs.items():  # parity first (and the warm-up of every kernel)
        e.batch(sets[0], fl, stream)
        snaps[name] = e.snapshot(N_FRAMES)
        assert not snaps[name][0].any(), (name, snaps[name][0])
        e.single(sets[1][3], fl, stream)
        snaps[name + "s"] = e.snapshot(1)
    for name in encs:
        if not (_same(snaps[name], snaps["0"]) and _same(snaps[name + "s"], snaps["0s"])):
            raise SystemExit(f"bench_limit_lengths: route ({name}) differs from route (0) on ordinary frames")
    res = {"step": "ordinary", "device": torch.cuda.get_device_name(dev), "frame": [W, H], "frames_per_batch": N_FRAMES,
           "parent": bool(old)}
    res["batch"] = _time({n: (lambda r, s, e=e, fl=fl: e.batch(sets[r % 2], fl, s)) for n, (e, fl) in encs.items()},
                         regions, dev)
    res["single"] = _time({n: (lambda r, s, e=e, fl=fl: e.single(sets[r % 2][r % N_FRAMES], fl, s))
                           for n, (e, fl) in encs.items()}, regions, dev)
    for mode in ("batch", "single"):
        m = {k: v["median_us"] for k, v in res[mode].items()}
        res[mode + "_ratios"] = {"1_over_0": round(m["1"] / m["0"], 4)}
        if "p" in m:
            res[mode + "_ratios"].update({"0_over_p": round(m["0"] / m["p"], 4), "1_over_p": round(m["1"] / m["p"], 4)})
    _print(f"[ordinary] frames that need no limiting, 2048x1536, cold regions, HIP events, median (min..max) us over "
           f"{regions} regions (batch: 64 frames per call; single: one frame):", res,
           {"p": "(p) parent commit's library", "0": "(0) this library, flag off",
            "1": "(1) this library, MH_ENCODE_LIMIT_LENGTHS"})
    print(f"  ratios of medians: batch {res['batch_ratios']}  single {res['single_ratios']}"
          + ("" if old else "   (no parent library given: route (p) skipped)"))
    print(json.dumps(res))


def step_deep(regions, parent):
    import numpy as np
    import torch
    import metalhuffman_amd as mh
    dev, new, _ = _setup(None)
    imgs_d, deep = _sets("deep", dev)
    _, plain = _sets("ordinary", dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    try:
        mh.encode_frame(imgs_d[0])
        raise SystemExit("bench_limit_lengths: the deep frame's tree fits 16 bits")
    except mh.MHError as e:
        assert e.status == -3
    host = mh.encode_frame(imgs_d[0], limit_lengths=True)
    new.batch(deep[0], 0, stream)
    st = new.snapshot(N_FRAMES)[0]
    assert (st == -3).all(), st  # without the flag: rejected, as before
    for call in (lambda: new.batch(deep[0], LIMIT, stream), lambda: new.single(deep[0][0], LIMIT, stream)):
        call()
        s = new.snapshot(1)
        if s[0][0] != 0 or not (np.array_equal(s[2], host.canon) and np.array_equal(s[3][0], host.codes)
                                and np.array_equal(s[4].view(np.uint32), host.block_offsets)):
            raise SystemExit("bench_limit_lengths: the device's limited frame differs from the host codec's")
    new.batch(deep[0], LIMIT, stream)
    assert not new.snapshot(N_FRAMES)[0].any()
    new.batch(plain[0], LIMIT, stream)  # warm-up of the ordinary route
    new.single(plain[0][0], LIMIT, stream)
    torch.cuda.synchronize(dev)
    res = {"step": "deep", "device": torch.cuda.get_device_name(dev), "frame": [W, H], "frames_per_batch": N_FRAMES,
           "deep_symbols": 30, "deep_tree_depth": 29,
           "cost_bits": _cost_bits(imgs_d[0], host.canon)}
    res["batch"] = _time({"d": lambda r, s: new.batch(deep[r % 2], LIMIT, s),
                          "o": lambda r, s: new.batch(plain[r % 2], LIMIT, s)}, regions, dev)
    res["single"] = _time({"d": lambda r, s: new.single(deep[r % 2][r % N_FRAMES], LIMIT, s),
                           "o": lambda r, s: new.single(plain[r % 2][r % N_FRAMES], LIMIT, s)}, regions, dev)
    db = res["batch"]["d"]["median_us"] - res["batch"]["o"]["median_us"]
    ds = res["single"]["d"]["median_us"] - res["single"]["o"]["median_us"]
    res["delta_us"] = {"batch_call": round(db, 2), "per_frame_of_the_batch": round(db / N_FRAMES, 3),
                       "per_tree_workgroup_single_frame": round(ds, 2)}
    _print(f"[deep] 64 frames that all need limiting against ordinary frames, both with the flag, 2048x1536, cold "
           f"regions, HIP events, median (min..max) us over {regions} regions:", res,
           {"d": "(d) deep frames (30 Fibonacci symbols, tree depth 29)", "o": "(o) ordinary frames (BigBridge shuffles)"})
    print(f"  (d) - (o): batch call {db:+.2f} us = {db / N_FRAMES:+.3f} us per frame; single frame (one tree workgroup "
          f"on the critical path) {ds:+.2f} us. The difference holds the other data's split and packing cost too.")
    c = res["cost_bits"]
    print(f"  cost of limiting on a deep frame: {c['limited']} bits against {c['huffman_unlimited']} of the depth-"
          f"{c['huffman_depth']} Huffman tree (x {c['ratio']:.6f})")
    print(json.dumps(res))


def _cost_bits(img, limited):
    """Sum of count x length of a frame under its limited code and under its (too deep) Huffman tree."""
    import numpy as np
    from metalhuffman_amd import _native as N
    f = np.ascontiguousarray(_hist(img), np.uint64)
    huff = np.zeros(256, np.uint8)
    assert N.lib().mh_code_lengths(f.ctypes.data_as(N._u64p), huff.ctypes.data_as(N._u8p)) == -3
    cost = lambda lens: int(sum(int(c) * int(l) for c, l in zip(f, lens)))
    out = {"limited": cost(limited), "huffman_unlimited": cost(huff), "huffman_depth": int(huff.max())}
    out["ratio"] = round(out["limited"] / out["huffman_unlimited"], 8)
    return out


def _hist(img):
    import numpy as np
    b = img.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64).astype(np.int16)
    d = np.diff(np.concatenate([np.zeros((b.shape[0], 1), np.int16), b], axis=1), axis=1).astype(np.uint8)
    return np.bincount(d.reshape(-1), minlength=256)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per route")
    ap.add_argument("--parent", default=os.path.join(ROOT, "ab", "lib_parent.so"),
                    help="libmetalhuffman_amd.so built from the parent commit (route (p); skipped when absent)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "limit_lengths_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        {"ordinary": step_ordinary, "deep": step_deep}[args.step](args.regions, args.parent)
        return 0
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_limit_lengths.py --regions {args.regions}   (library stamp "
            f"{B.library_stamp()[:16]})\n"]
    for step in ("ordinary", "deep"):  # each under its own time limit; stop at the first failure
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--regions", str(args.regions), "--parent", args.parent]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)  # (stderr passes through)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f"bench_limit_lengths: step {step} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
        text.append(p.stdout)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
