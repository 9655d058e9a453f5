#!/usr/bin/env python3
"""Crops of the 8192^2 mirror tile (config 3) decoded straight into normalised float16, bfloat16 or
float32 elements, half of them mirrored, in one launch (mh_decode_crops_norm) against what a caller
does without it, with one prepared table:

  (a) one mh_decode_crops_norm launch: conversion, (x * scale + bias) and the mirror in the decoder;
  (b) what a caller does today: mh_decode_crops into a uint8 batch, then .to(dtype), * scale + bias
      and torch.flip of the mirrored half -- all inside the clocked region;
  (c) mh_decode_crops alone: the same crops as bytes. It does not produce the batch; (a)/(c) is the
      price of storing 2 or 4 times the bytes, reported and not gated.

Crops of 224 x 224 pixels at seeded random pixel origins, N = 1, 16, 64 and 256, and 64 crops of
1024 x 768, for each of the three formats; scale = 1 / (255 * 0.229), bias = -0.485 / 0.229.
scripts/bench_region.py's frame and method, as scripts/bench_crops.py: two resident 8192^2 frames of
one table alternate region by region; every region is cold -- a 1 GiB device copy evicts the Infinity
Cache and the L2s first (bench.FLUSH), off the clock -- the launches of a region are enqueued behind
bench.py's launch gate between two HIP events, the figure is the events' distance, the routes
alternate region by region, and the table gives the median (min .. max) over the timed regions.
Before timing, route (a) is compared BIT FOR BIT with codec.norm_table's 256 elements looked up by
the encoder's input (reversed where mirrored), and route (c) with the encoder's input.

Gate: (a) < (b) by more than the +-4 % box spread, i.e. (a)/(b) < 0.96, at every row with N >= 16 and
every format; the exit status is 3 when a row misses it (the record is written all the same).

    python scripts/bench_crops_norm.py [--out profiles/crops_norm_ab.txt] [--regions 15]

runs the step as a child process under its own `timeout` and writes what it printed to --out.
`--step lists` runs it here.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SIDE = 8192
ROWS = [((224, 224), 1), ((224, 224), 16), ((224, 224), 64), ((224, 224), 256), ((1024, 768), 64)]
SEED = 20263
SCALE, BIAS = 1.0 / (255.0 * 0.229), -0.485 / 0.229
GATE = 0.96  # (a)/(b) below it: faster by more than the box spread
STEPS = {"lists": 1100}  # step -> its time limit, seconds
GATE_MISSED = 3  # the step's exit status when a gated row misses the gate


def step_lists(regions):
    import numpy as np
    import torch
    from bench_region import _fmt, _setup, _timed
    from metalhuffman_amd import codec, decoder as D
    dev, tabs, sets = _setup()
    print(f"[lists] N crops of one {SIDE}x{SIDE} mirror-tile frame at seeded random PIXEL origins, every second one "
          f"mirrored, scale = 1/(255*0.229), bias = -0.485/0.229, one prepared table, cold regions, HIP events, "
          f"median (min .. max) us over {regions} regions")
    print(f"  {'dtype':<9} {'crop':<10} {'N':>4} {'grid':>9}   {'(a) mh_decode_crops_norm':<34} "
          f"{'(b) crops + to + fma + flip':<34} {'(c) mh_decode_crops, bytes':<34} (a)/(b)  (a)/(c)")
    rows, missed = [], []
    rng = np.random.default_rng(SEED)
    for (w, h), n in ROWS:
        x0 = rng.integers(0, SIDE - w + 1, n)
        y0 = rng.integers(0, SIDE - h + 1, n)
        f = np.zeros(n, np.int64)
        flags = (np.arange(n) & 1).astype(np.int64)          # half of them mirrored
        desc = torch.from_numpy(np.stack([f, x0, y0, flags], axis=1).astype(np.int32)).to(dev)
        plain = torch.from_numpy(np.stack([f, x0, y0, f], axis=1).astype(np.int32)).to(dev)
        midx = torch.from_numpy(np.flatnonzero(flags)).to(dev)
        bytes_bc = torch.empty((n, h, w), dtype=torch.uint8, device=dev)   # (w is a multiple of 8)
        assert w % 8 == 0
        for dtype in (torch.float16, torch.bfloat16, torch.float32):
            name = str(dtype).rsplit(".", 1)[-1]
            ibits = torch.int32 if dtype is torch.float32 else torch.int16
            T = torch.from_numpy(codec.norm_table(name, SCALE, BIAS).view(np.int32 if dtype is torch.float32
                                                                          else np.int16).copy()).to(dev)
            out_a = torch.empty((n, h, w), dtype=dtype, device=dev)
            res_b = {}

            def route_a(s):
                D.decode_crops_normalized(s["fr"], tabs, desc, (w, h), dtype, SCALE, BIAS, out=out_a)

            def route_b(s):
                D.decode_crops(s["fr"], tabs, plain, (w, h), out=bytes_bc)
                y = bytes_bc.to(dtype) * SCALE + BIAS
                if midx.numel():
                    y[midx] = torch.flip(y[midx], dims=[-1])
                res_b["out"] = y

            def route_c(s):
                D.decode_crops(s["fr"], tabs, plain, (w, h), out=bytes_bc)

            for s in sets:  # parity first (and the warm-up of every kernel)
                want = torch.stack([s["ref"][int(y): int(y) + h, int(x): int(x) + w] for x, y in zip(x0, y0)])
                want_a = T[want.long()]
                if midx.numel():
                    want_a[midx] = torch.flip(want_a[midx], dims=[-1])
                out_a.fill_(-7.0)
                route_a(s)
                route_b(s)
                torch.cuda.synchronize(dev)
                if not torch.equal(out_a.view(ibits), want_a):
                    raise SystemExit(f"bench_crops_norm: route (a) differs from the table lookup ({name}, {n} x {w}x{h})")
                # (b) multiplies and adds in `dtype`, unfused: close to (a), not equal to it
                if not torch.allclose(res_b["out"].float(), out_a.float(), rtol=2e-2, atol=2e-2):
                    raise SystemExit(f"bench_crops_norm: route (b) is not the same batch ({name}, {n} x {w}x{h})")
                bytes_bc.fill_(0xA5)
                route_c(s)
                torch.cuda.synchronize(dev)
                if not torch.equal(bytes_bc, want):
                    raise SystemExit(f"bench_crops_norm: route (c) differs from the encoder's input ({n} x {w}x{h})")
            g, wv = D.decode_crops_normalized_shape(sets[0]["fr"], n, (w, h), dtype)
            res = _timed(dev, {"a": route_a, "b": route_b, "c": route_c}, sets, regions)
            ab = round(res["a"]["median_us"] / res["b"]["median_us"], 4)
            ac = round(res["a"]["median_us"] / res["c"]["median_us"], 4)
            gated = n >= 16
            if gated and not ab < GATE:
                missed.append((name, w, h, n, ab))
            rows.append({"dtype": name, "crop": [w, h], "n_crops": n, "origins": np.stack([x0, y0], axis=1).tolist(),
                         "mirrored": int(flags.sum()), "shape": {"groups_per_crop": g, "waves_per_group": wv},
                         "routes": res, "a_over_b": ab, "a_over_c": ac, "gated": gated})
            print(f"  {name:<9} {f'{w}x{h}':<10} {n:>4} {f'{n}x{g}x{wv}':>9}   {_fmt(res['a']):<34} {_fmt(res['b']):<34} "
                  f"{_fmt(res['c']):<34} {ab:.3f}    {ac:.3f}")
    print(json.dumps({"step": "lists", "device": torch.cuda.get_device_name(dev), "seed": SEED, "scale": SCALE,
                      "bias": BIAS, "gate_a_over_b": GATE, "rows": rows}))
    for m in missed:
        print(f"bench_crops_norm: GATE MISSED: {m[0]} {m[3]} x {m[1]}x{m[2]}: (a)/(b) = {m[4]:.3f}, not below {GATE}")
    print("gate: (a)/(b) < %.2f at every row with N >= 16: %s" % (GATE, "MISSED" if missed else "held"))
    return GATE_MISSED if missed else 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crops_norm_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        return step_lists(args.regions)
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_crops_norm.py --regions {args.regions}   (library stamp {B.library_stamp()[:16]})\n"]
    rc = 0
    for step in ("lists",):  # under its own time limit
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--regions", str(args.regions)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)  # (stderr passes through)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        text.append(p.stdout)
        if p.returncode not in (0, GATE_MISSED):
            print(f"bench_crops_norm: step {step} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
        rc = rc or p.returncode  # GATE_MISSED; the record is written all the same
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return rc


if __name__ == "__main__":
    sys.exit(main())
