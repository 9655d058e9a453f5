"""LDS bank-conflict model of the single-frame chain on real bitstreams (CPU simulation,
diagnostic): the 14-bit table lookup of every step and the stage read of the even steps,
on the natural BigBridge frame and on block-shuffled ones (bench.py's frames).

The method of scripts/sim_lds_banks.py: for every tile (64 blocks = 64 lanes) and decode
step, the lanes' addresses are banked per MI355X_MICROARCH.md (two 32-lane groups, bank =
(byte_addr / 4) % 32, one LDS cycle per distinct dword on the busiest bank, identical
dwords broadcast; 2 cycles per 64-lane access = conflict-free).
  lookup: u16 entry at index (16-bit window >> 2) of the 2^14-entry table
  stage read: the dword two words behind the cursor's word in the tile's staged span
    (the lazy step's next-word read; its one-step lag behind the cursor is not modelled)

    python scripts/sim_lds_banks14.py [--tiles N] [--seeds 0 5]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import metalhuffman_amd as mh  # noqa: E402
from metalhuffman_amd import frames as F  # noqa: E402


def access_cycles(dw):
    """dw: (64,) dword addresses of one wave access -> LDS cycles (2 = conflict-free)."""
    c = 0
    for g in (0, 1):
        u = np.unique(dw[g * 32:(g + 1) * 32])
        c += np.bincount(u % 32, minlength=32).max()
    return c


def frame_model(img, ntiles, seed=0):
    ef = mh.encode_frame(img)
    assert ef.canon.max() <= 14, "the 14-bit table needs a longest code of <= 14 bits"
    bits = np.unpackbits(ef.codes)
    offs = ef.block_offsets.astype(np.int64)
    t1, t2 = ef.tables()
    t1 = t1.view(np.uint8).reshape(-1, 2)
    t2 = t2.view(np.uint8).reshape(-1, 2)
    nt = ef.n_blocks // 64
    tiles = np.random.default_rng(seed).choice(nt, size=min(ntiles, nt), replace=False)
    look, stage = [], []
    for t in tiles:
        pos = offs[t * 64:(t + 1) * 64].copy()
        start = (int(pos[0]) >> 3) & ~15  # the staged span's first byte (16-aligned)
        for j in range(64):
            w = np.zeros(64, np.int64)
            for b in range(16):
                w = (w << 1) | bits[pos + b]
            e = t1[w >> 8]
            sym, ln = e[:, 0].astype(np.int64), e[:, 1].astype(np.int64)
            esc = ln == 0
            if esc.any():
                ln[esc] = t2[sym[esc] * 256 + (w[esc] & 0xFF)][:, 1]
            look.append(access_cycles((w >> 2) >> 1))  # u16 entries, two per dword
            if j % 2 == 0:
                stage.append(access_cycles(((pos - 8 * start) >> 5) + 2))
            pos += ln
    return float(np.mean(look)), float(np.mean(stage)), len(tiles)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=128)
    ap.add_argument("--seeds", type=int, nargs="*", default=[0, 5], help="block_shuffle seeds")
    args = ap.parse_args()
    bb = F.bigbridge()
    rows = [("natural BigBridge", bb)] + [(f"block-shuffled, seed {s}", F.block_shuffle(bb, s)) for s in args.seeds]
    print("LDS cycles per 64-lane access (2 = conflict-free), mean over tiles x steps")
    for name, img in rows:
        lk, st, n = frame_model(img, args.tiles)
        print(f"  {name:26s} ({n} tiles): 14-bit lookup {lk:5.2f}   stage read (even steps) {st:5.2f}")


if __name__ == "__main__":
    main()
