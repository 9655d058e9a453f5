#!/usr/bin/env python3
"""Samples of three-plane images (three 8192^2 mirror-tile frames per image, config 3) decoded into
a normalised [n, 3, h, w] tensor, every second sample mirrored, the three ImageNet (mean, std) pairs:

  (a) one mh_decode_crops_norm_planes launch;
  (b) today's route: three mh_decode_crops_norm launches, each with its own descriptor array (the
      plane's frame) and its own pair, into the planes of the same [n, 3, h, w] tensor; the three
      arrays are prepared outside the clock;
  (c) one mh_decode_crops_norm launch over 3 n descriptors with ONE common pair: the same decode work
      and store bytes in one launch of the older kernel. It does not produce the batch; (a)/(c) is
      the price of the plane trip at the head of a workgroup, reported and not gated.

Samples of 224 x 224 at seeded random pixel origins, N = 1, 16, 64 and 256, and 64 samples of
1024 x 768, as float16 and float32. scripts/bench_region.py's method, as scripts/bench_crops_norm.py:
two resident image sets of one table alternate region by region; every region is cold -- a 1 GiB
device copy evicts the Infinity Cache and the L2s first (bench.FLUSH), off the clock -- the launches
of a region are enqueued behind bench.py's launch gate between two HIP events, the figure is the
events' distance, the routes alternate region by region, and the table gives the median (min .. max)
over the timed regions. Before timing, route (a) is compared BIT FOR BIT with codec.norm_table's 256
elements of the plane's pair looked up by the encoder's input (reversed where mirrored), and route
(b) with route (a).

Gate: (a)/(b) < 0.96 -- faster by more than the +-4 % box spread -- at every row with N >= 16; the exit
status is 3 when a row misses it (the record is written all the same).

    python scripts/bench_crops_planes.py [--out profiles/crops_planes_ab.txt] [--regions 15]

runs the step as a child process under its own `timeout` and writes what it printed to --out.
`--step lists` runs it here.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SIDE = 8192
C = 3
ROWS = [((224, 224), 1), ((224, 224), 16), ((224, 224), 64), ((224, 224), 256), ((1024, 768), 64)]
SEED = 20264
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
GATE = 0.96  # (a)/(b) below it: faster by more than the box spread
STEPS = {"lists": 1100}  # step -> its time limit, seconds
GATE_MISSED = 3  # the step's exit status when a gated row misses the gate


def _setup():
    """Two resident images of three planes each (six frames of one table, plane after plane), their
    inputs on the device, one prepared table."""
    import numpy as np
    import torch
    import bench
    from metalhuffman_amd import decoder as D
    from metalhuffman_amd import frames as F
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if not bench.GATE.ok():
        raise SystemExit("bench_crops_planes: the launch gate (scripts/micro/liblaunch_gate.so) is not built")
    base = F.mirror_tile(F.bigbridge(), SIDE, SIDE)
    imgs = [base] + [F.block_shuffle(base, 100 + i) for i in range(2 * C - 1)]
    efs = bench.encode_many(imgs, threads=2 * C)
    assert all(np.array_equal(ef.canon, efs[0].canon) for ef in efs)
    t1, t2 = efs[0].tables()
    tabs = D.DeviceTables.upload(t1, t2, dev)
    sets = [{"ref": [torch.from_numpy(im).to(dev) for im in imgs[C * i: C * i + C]],
             "fr": D.DeviceFrames.pack(efs[C * i: C * i + C], dev)} for i in range(2)]
    return dev, tabs, sets


def step_lists(regions):
    import numpy as np
    import torch
    from bench_region import _fmt, _timed
    from metalhuffman_amd import _native as N, codec, decoder as D
    dev, tabs, sets = _setup()
    scale, bias = codec.norm_coefficients(MEAN, STD)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = N.lib()
    print(f"[lists] N samples of one 3-plane image ({C} {SIDE}x{SIDE} mirror-tile frames) at seeded random PIXEL "
          f"origins, every second one mirrored, the ImageNet pairs, one prepared table, cold regions, HIP events, "
          f"median (min .. max) us over {regions} regions")
    print(f"  {'dtype':<9} {'sample':<12} {'N':>4} {'grid':>10}   {'(a) mh_decode_crops_norm_planes':<34} "
          f"{'(b) 3 x mh_decode_crops_norm':<34} {'(c) 1 x mh_decode_crops_norm, 3N':<34} (a)/(b)  (a)/(c)")
    rows, missed = [], []
    rng = np.random.default_rng(SEED)
    for (w, h), n in ROWS:
        assert w % 8 == 0
        x0 = rng.integers(0, SIDE - w + 1, n)
        y0 = rng.integers(0, SIDE - h + 1, n)
        flags = (np.arange(n) & 1).astype(np.int64)          # every second sample mirrored
        plane_desc = [np.stack([np.full(n, c, np.int64), x0, y0, flags], axis=1).astype(np.int32) for c in range(C)]
        desc = torch.from_numpy(plane_desc[0]).to(dev)                        # (a): the sample's first frame
        desc_b = [torch.from_numpy(d).to(dev) for d in plane_desc]            # (b): one array per plane
        desc_c = torch.from_numpy(np.concatenate(plane_desc)).to(dev)         # (c): 3 n crops
        midx = torch.from_numpy(np.flatnonzero(flags)).to(dev)
        for dtype in (torch.float16, torch.float32):
            name = str(dtype).rsplit(".", 1)[-1]
            fmt, esize = codec.norm_format(dtype), (4 if dtype is torch.float32 else 2)
            ibits, nbits = (torch.int32, np.int32) if dtype is torch.float32 else (torch.int16, np.int16)
            T = [torch.from_numpy(codec.norm_table(name, scale[c], bias[c]).view(nbits).copy()).to(dev)
                 for c in range(C)]
            out_a = torch.empty((n, C, h, w), dtype=dtype, device=dev)
            out_b = torch.empty((n, C, h, w), dtype=dtype, device=dev)
            out_c = torch.empty((C * n, h, w), dtype=dtype, device=dev)
            pitch = w * esize

            def route_a(s):
                D.decode_crops_normalized_planes(s["fr"], tabs, desc, (w, h), dtype, scale, bias, out=out_a)

            def route_b(s):
                st, _ = D._frames_entry(s["fr"])
                for c in range(C):
                    rc = L.mh_decode_crops_norm(ctypes.byref(st), desc_b[c].data_ptr(), n, w, h, fmt, scale[c], bias[c],
                                                tabs.lut.data_ptr(), 0, None, None,
                                                out_b.data_ptr() + c * h * pitch, pitch, C * h * pitch, stream)
                    if rc:
                        N.check(rc, "mh_decode_crops_norm")

            def route_c(s):
                D.decode_crops_normalized(s["fr"], tabs, desc_c, (w, h), dtype, scale[0], bias[0], out=out_c)

            for s in sets:  # parity first (and the warm-up of every kernel)
                out_a.fill_(-7.0)
                out_b.fill_(-9.0)
                route_a(s)
                route_b(s)
                route_c(s)
                torch.cuda.synchronize(dev)
                for c in range(C):
                    want = torch.stack([s["ref"][c][int(y): int(y) + h, int(x): int(x) + w] for x, y in zip(x0, y0)])
                    want = T[c][want.long()]
                    if midx.numel():
                        want[midx] = torch.flip(want[midx], dims=[-1])
                    if not torch.equal(out_a[:, c].view(ibits), want):
                        raise SystemExit(f"bench_crops_planes: route (a) differs from the table lookup "
                                         f"({name}, {n} x {w}x{h}, plane {c})")
                    del want
                if not torch.equal(out_b.view(ibits), out_a.view(ibits)):
                    raise SystemExit(f"bench_crops_planes: route (b) is not route (a)'s batch ({name}, {n} x {w}x{h})")
            g, wv = D.decode_crops_normalized_planes_shape(sets[0]["fr"], n, (w, h), dtype, C)
            res = _timed(dev, {"a": route_a, "b": route_b, "c": route_c}, sets, regions)
            ab = round(res["a"]["median_us"] / res["b"]["median_us"], 4)
            ac = round(res["a"]["median_us"] / res["c"]["median_us"], 4)
            gated = n >= 16
            if gated and not ab < GATE:
                missed.append((name, w, h, n, ab))
            rows.append({"dtype": name, "sample": [w, h, C], "n_samples": n,
                         "origins": np.stack([x0, y0], axis=1).tolist(), "mirrored": int(flags.sum()),
                         "shape": {"groups_per_plane": g, "waves_per_group": wv}, "routes": res, "a_over_b": ab,
                         "a_over_c": ac, "gated": gated})
            print(f"  {name:<9} {f'{w}x{h}x{C}':<12} {n:>4} {f'{n * C}x{g}x{wv}':>10}   {_fmt(res['a']):<34} "
                  f"{_fmt(res['b']):<34} {_fmt(res['c']):<34} {ab:.3f}    {ac:.3f}", flush=True)
            del out_a, out_b, out_c
    print(json.dumps({"step": "lists", "device": torch.cuda.get_device_name(dev), "seed": SEED, "scale": scale,
                      "bias": bias, "gate_a_over_b": GATE, "rows": rows}))
    for m in missed:
        print(f"bench_crops_planes: GATE MISSED: {m[0]} {m[3]} x {m[1]}x{m[2]}x{C}: (a)/(b) = {m[4]:.3f}, not below {GATE}")
    print("gate: (a)/(b) < %.2f at every row with N >= 16: %s" % (GATE, "MISSED" if missed else "held"))
    return GATE_MISSED if missed else 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crops_planes_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        return step_lists(args.regions)
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_crops_planes.py --regions {args.regions}   (library stamp {B.library_stamp()[:16]})\n"]
    rc = 0
    for step in ("lists",):  # under its own time limit
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--regions", str(args.regions)]
        p = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)  # (stderr passes through)
        lines = []
        for line in p.stdout:  # shown as it comes: the step takes minutes
            sys.stdout.write(line)
            sys.stdout.flush()
            lines.append(line)
        p.wait()
        text.append("".join(lines))
        if p.returncode not in (0, GATE_MISSED):
            print(f"bench_crops_planes: step {step} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
        rc = rc or p.returncode  # GATE_MISSED; the record is written all the same
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return rc


if __name__ == "__main__":
    sys.exit(main())
