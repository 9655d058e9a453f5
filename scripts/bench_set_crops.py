#!/usr/bin/env python3
"""A loader's batch over images of K distinct sizes: N samples of 224 x 224, three planes, float16, drawn
uniformly from 16 three-plane images in K = 1, 4 or 16 sizes between 256 x 256 and 2048 x 1536, every
second sample mirrored, the three ImageNet (mean, std) pairs, a table per frame:

  (a) one mh_decode_set_crops_norm_planes launch over the frame set;
  (b) what a caller did before the set entries: the batch sorted by image size, one
      mh_decode_crops_norm_planes launch per size present, each over that size's own DeviceFrames and
      table set, into its run of slots of the same [n, 3, h, w] tensor. The per-size descriptor arrays
      are prepared outside the clock;
  (c) K = 1 only: the parent entry on the same frames packed as one DeviceFrames -- the yardstick
      for the set entry's second dependent load (the geometry record). At K = 1 it is route (b).

(a) runs over the same size-sorted descriptors, so its tensor is compared BIT FOR BIT with (b)'s
before timing, and both with codec.norm_table's elements looked up by the source pixels.
scripts/bench_crops_planes.py's method: two resident image sets alternate region by region; every
region is cold (bench.FLUSH, off the clock); the launches of a region are enqueued behind bench.py's
launch gate between two HIP events; the routes alternate region by region; median (min .. max) over the
timed regions.

Gate: (a)/(b) < 0.96 -- faster by more than the +-4 % box spread -- at every row with K >= 4 and
N >= 16; the exit status is 3 when a row misses it (the record is written all the same). (a)/(c) is
reported, not gated.

    python scripts/bench_set_crops.py [--out profiles/set_crops_ab.txt] [--regions 15]

runs the step as a child process under its own `timeout` and writes what it printed to --out.
`--step sets` runs it here.
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

C = 3
IMAGES = 16
W, H = 224, 224
NS = (16, 64, 256)
WIDTHS, HEIGHTS = (256, 640, 1280, 2048), (256, 512, 1024, 1536)
SIZES = {1: [(1280, 1024)],
         4: list(zip(WIDTHS, HEIGHTS)),
         16: [(w, h) for h in HEIGHTS for w in WIDTHS]}
SEED = 20266
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
GATE = 0.96
STEPS = {"sets": 1100}
GATE_MISSED = 3


def _image_set(K, which, dev, base):
    """16 images, image i of size SIZES[K][i % K], three planes each (plane after plane): the frame set,
    and per size the same frames as a DeviceFrames with its own table set and its images' indices."""
    import numpy as np
    import torch
    import concurrent.futures as cf
    import metalhuffman_amd as mh
    from metalhuffman_amd import decoder as D
    rng = np.random.default_rng(SEED + 100 * K + which)
    planes, sizes = [], []
    for i in range(IMAGES):
        w, h = SIZES[K][i % K]
        x, y = int(rng.integers(0, base.shape[1] - w + 1)), int(rng.integers(0, base.shape[0] - h + 1))
        img = base[y: y + h, x: x + w]
        planes += [np.ascontiguousarray(np.roll(img, 61 * c, axis=1)) for c in range(C)]
        sizes.append((w, h))
    with cf.ThreadPoolExecutor(16) as ex:  # ctypes releases the GIL
        efs = list(ex.map(lambda p: mh.encode_frame(p, limit_lengths=True), planes))
    canon = np.stack([ef.canon for ef in efs])
    groups = []
    for size in SIZES[K]:
        members = [i for i in range(IMAGES) if sizes[i] == size]
        idx = [C * i + c for i in members for c in range(C)]
        groups.append({"size": size, "images": members,
                       "fr": D.DeviceFrames.pack([efs[j] for j in idx], dev, shared_table=False),
                       "tabs": D.DeviceTableSet.from_canonical_headers(canon[idx], dev)})
    return {"fs": D.DeviceFrameSet.pack(efs, dev), "tabs": D.DeviceTableSet.from_canonical_headers(canon, dev),
            "groups": groups, "sizes": sizes, "ref": [torch.from_numpy(p).to(dev) for p in planes]}


def step_sets(regions):
    import numpy as np
    import torch
    import bench
    from bench_region import _fmt, _timed
    from metalhuffman_amd import codec, decoder as D
    from metalhuffman_amd import frames as F
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if not bench.GATE.ok():
        raise SystemExit("bench_set_crops: the launch gate (scripts/micro/liblaunch_gate.so) is not built")
    base = F.bigbridge()
    scale, bias = codec.norm_coefficients(MEAN, STD)
    dtype, name = torch.float16, "float16"
    T = [torch.from_numpy(codec.norm_table(name, scale[c], bias[c]).view(np.int16).copy()).to(dev) for c in range(C)]
    print(f"[sets] N samples of {W}x{H}x{C} {name}, drawn uniformly from {IMAGES} three-plane images in K distinct "
          f"sizes between 256x256 and 2048x1536, every second one mirrored, the ImageNet pairs, a table per frame, "
          f"cold regions, HIP events, median (min .. max) us over {regions} regions")
    print(f"  {'K':>3} {'N':>4} {'sizes hit':>9} {'grid':>10}   {'(a) 1 x mh_decode_set_crops_norm_planes':<40} "
          f"{'(b) mh_decode_crops_norm_planes per size':<40} {'(c) parent entry, K = 1':<34} (a)/(b)  (a)/(c)")
    rows, missed = [], []
    for K in (1, 4, 16):
        sets = [_image_set(K, which, dev, base) for which in range(2)]
        assert sets[0]["sizes"] == sets[1]["sizes"]
        sizes = sets[0]["sizes"]
        rng = np.random.default_rng(SEED + K)
        for n in NS:
            img = rng.integers(0, IMAGES, n)
            img = img[np.argsort([SIZES[K].index(sizes[i]) for i in img], kind="stable")]   # the batch sorted by size
            x0 = np.array([rng.integers(0, sizes[i][0] - W + 1) for i in img])
            y0 = np.array([rng.integers(0, sizes[i][1] - H + 1) for i in img])
            flags = (np.arange(n) & 1).astype(np.int64)
            desc = torch.from_numpy(np.stack([C * img, x0, y0, flags], axis=1).astype(np.int32)).to(dev)
            runs = []    # (b): per size present, its run of slots and its descriptors in the group's own frame numbers
            for g, grp in enumerate(sets[0]["groups"]):
                sel = np.flatnonzero([sizes[i] == grp["size"] for i in img])
                if sel.size:
                    assert sel[-1] - sel[0] + 1 == sel.size
                    local = np.array([grp["images"].index(i) for i in img[sel]])
                    d = np.stack([C * local, x0[sel], y0[sel], flags[sel]], axis=1).astype(np.int32)
                    runs.append((g, int(sel[0]), int(sel[-1]) + 1, torch.from_numpy(d).to(dev)))
            out_a = torch.empty((n, C, H, W), dtype=dtype, device=dev)
            out_b = torch.empty((n, C, H, W), dtype=dtype, device=dev)

            def route_a(s):
                D.decode_set_crops_normalized_planes(s["fs"], s["tabs"], desc, (W, H), dtype, scale, bias, out=out_a)

            def route_b(s):
                for g, lo, hi, d in runs:
                    grp = s["groups"][g]
                    D.decode_crops_normalized_planes(grp["fr"], grp["tabs"], d, (W, H), dtype, scale, bias,
                                                     out=out_b[lo:hi])

            for s in sets:  # parity first (and the warm-up of every kernel)
                out_a.fill_(-7.0)
                out_b.fill_(-9.0)
                route_a(s)
                route_b(s)
                torch.cuda.synchronize(dev)
                for c in range(C):
                    want = torch.stack([s["ref"][C * int(i) + c][int(y): int(y) + H, int(x): int(x) + W]
                                        for i, x, y in zip(img, x0, y0)])
                    want = T[c][want.long()]
                    midx = torch.from_numpy(np.flatnonzero(flags)).to(dev)
                    want[midx] = torch.flip(want[midx], dims=[-1])
                    if not torch.equal(out_a[:, c].view(torch.int16), want):
                        raise SystemExit(f"bench_set_crops: route (a) differs from the table lookup (K {K}, N {n}, "
                                         f"plane {c})")
                    del want
                if not torch.equal(out_b.view(torch.int16), out_a.view(torch.int16)):
                    raise SystemExit(f"bench_set_crops: route (b) is not route (a)'s batch (K {K}, N {n})")
            g, wv = D.decode_set_crops_normalized_planes_shape(sets[0]["fs"], n, (W, H), dtype, C)
            res = _timed(dev, {"a": route_a, "b": route_b}, sets, regions)
            ab = round(res["a"]["median_us"] / res["b"]["median_us"], 4)
            gated = K >= 4 and n >= 16
            if gated and not ab < GATE:
                missed.append((K, n, ab))
            rows.append({"K": K, "n_samples": n, "sizes_hit": len(runs), "shape": {"groups_per_plane": g,
                         "waves_per_group": wv}, "routes": res, "a_over_b": ab, "a_over_c": ab if K == 1 else None,
                         "gated": gated})
            c_col = _fmt(res["b"]) if K == 1 else "-"
            ac = f"{ab:.3f}" if K == 1 else "-"
            print(f"  {K:>3} {n:>4} {len(runs):>9} {f'{n * C}x{g}x{wv}':>10}   {_fmt(res['a']):<40} "
                  f"{_fmt(res['b']):<40} {c_col:<34} {ab:.3f}    {ac}", flush=True)
            del out_a, out_b
        del sets
    print(json.dumps({"step": "sets", "device": torch.cuda.get_device_name(dev), "seed": SEED, "scale": scale,
                      "bias": bias, "gate_a_over_b": GATE, "rows": rows}))
    for m in missed:
        print(f"bench_set_crops: GATE MISSED: K {m[0]}, N {m[1]}: (a)/(b) = {m[2]:.3f}, not below {GATE}")
    print("gate: (a)/(b) < %.2f at every row with K >= 4 and N >= 16: %s" % (GATE, "MISSED" if missed else "held"))
    return GATE_MISSED if missed else 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process")
    ap.add_argument("--regions", type=int, default=15, help="timed regions per route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_crops_ab.txt"))
    args = ap.parse_args(argv)
    if args.step:
        return step_sets(args.regions)
    import metalhuffman_amd.build as B
    B.build()
    B.build_probe()
    text = [f"# python scripts/bench_set_crops.py --regions {args.regions}   (library stamp {B.library_stamp()[:16]})\n"]
    rc = 0
    for step in ("sets",):  # under its own time limit
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
            print(f"bench_set_crops: step {step} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode
        rc = rc or p.returncode  # GATE_MISSED; the record is written all the same
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))
    return rc


if __name__ == "__main__":
    sys.exit(main())
