"""mh_decode_set_crops (and, in the seeded sweep, mh_decode_set_crops_norm_planes with one plane): crops
of frames of DIFFERENT sizes in one launch. Every launch goes through the C-ABI into a guarded buffer
(set_helpers.py) and every byte of it is compared: an accepted crop's pixels against the source image's
own [y0: y0 + h, x0: x0 + w] (which set_helpers cross-checks with codec.decode_frame_cpu), everything
else -- guards, gaps, the slots of rejected and skipped crops -- against the fill. No tolerance."""
from __future__ import annotations

import numpy as np
import pytest

import norm_helpers as NH
import set_helpers as S
from set_helpers import MH_ERR_DIMS

pytestmark = pytest.mark.gpu

SIZES = ((8, 8), (9, 17), (64, 40), (131, 77), (520, 24))   # one block ... 65 blocks wide
FMTS = pytest.mark.parametrize("fmt", S.FORMATS)
TABS = pytest.mark.parametrize("tables", S.TABLES)


def _set(mh, device, fmt="delta", tables="set", sizes=SIZES, seed=0):
    pairs = S.encoded(mh, sizes, fmt, tables == "shared", seed)
    fs, tabs = S.upload(device, [p[0] for p in pairs], tables == "shared")
    assert fs.sizes == tuple(sizes) and fs.n_frames == len(sizes)
    return fs, tabs, [p[1] for p in pairs]


def _expect(imgs, sizes, desc, size):
    return [[S.pixels(imgs, d, size)] if S.fits(sizes, d, size) else None for d in desc]


def _statuses(sizes, desc, size):
    return [0 if S.fits(sizes, d, size) else MH_ERR_DIMS for d in desc]


# ---- 1. mixed sizes ----------------------------------------------------------------------------------------

def _mixed(size, seed):
    """Crops of `size` at the four corners and at seeded interior origins of every frame large enough,
    shuffled (frames in any order, with repeats)."""
    w, h = size
    rng = np.random.default_rng(seed)
    desc = []
    for f, (W, H) in enumerate(SIZES):
        if w > W or h > H:
            continue
        desc += [(f, 0, 0, 0), (f, W - w, 0, 0), (f, 0, H - h, 0), (f, W - w, H - h, 0)]
        desc += [(f, int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), 0) for _ in range(6)]
    order = rng.permutation(len(desc))
    return [desc[i] for i in order]


@FMTS
@TABS
def test_mixed_sizes(mh, device, fmt, tables):
    fs, tabs, imgs = _set(mh, device, fmt, tables)
    seen = set()
    for k, size in enumerate(((5, 3), (8, 8), (24, 16))):
        desc = _mixed(size, 11 + k)
        if size == (24, 16):  # every (dx, dy) of the block grid, in the frames that leave room for it
            desc += [(3 + (i & 1), 8 * (i % 5) + (i & 7), (i >> 3), 0) for i in range(64)]
        assert len({d[0] for d in desc}) == sum(size[0] <= W and size[1] <= H for W, H in SIZES) >= 3
        assert all(S.fits(SIZES, d, size) for d in desc)
        seen |= {(d[1] & 7, d[2] & 7) for d in desc}
        lay = S.run_crops(device, fs, tabs, desc, size)
        assert lay.rc == 0
        S.check(lay, _expect(imgs, SIZES, desc, size))
        assert lay.status == [0] * len(desc)
    assert {dx for dx, _ in seen} == set(range(8)) and {dy for _, dy in seen} == set(range(8))
    assert len(seen) == 64


# ---- 2. two tiles per row, and frames too small for the crop --------------------------------------------------

@FMTS
def test_two_tiles_per_row(mh, device, fmt):
    """A 512 x 8 crop is 64 output words: S = 2 tiles per block row, and at x0 = 3 it touches 65
    blocks. The same launch names the smaller frames, which cannot hold it."""
    fs, tabs, imgs = _set(mh, device, fmt)
    size = (512, 8)
    desc = [(4, 0, 0, 0), (0, 0, 0, 0), (4, 3, 16, 0), (2, 0, 0, 0), (4, 8, 9, 0), (3, 0, 0, 0), (1, 0, 0, 0),
            (4, 3, 0, 0), (4, 9, 0, 0)]
    assert [S.fits(SIZES, d, size) for d in desc] == [True, False, True, False, True, False, False, True, False]
    lay = S.run_crops(device, fs, tabs, desc, size)
    assert lay.rc == 0
    S.check(lay, _expect(imgs, SIZES, desc, size))
    assert lay.status == _statuses(SIZES, desc, size)


# ---- 3. a set of one size is mh_decode_crops -----------------------------------------------------------------

@FMTS
@TABS
def test_same_size_set_equals_decode_crops(mh, device, fmt, tables):
    import torch
    from metalhuffman_amd import decoder as D
    sizes = ((64, 40),) * 4
    pairs = S.encoded(mh, sizes, fmt, tables == "shared", seed=3)
    efs = [p[0] for p in pairs]
    fs, tabs = S.upload(device, efs, tables == "shared")
    fr = D.DeviceFrames.pack(efs, device, shared_table=tables == "shared")
    rng = np.random.default_rng(5)
    size = (19, 11)
    crops = [(int(rng.integers(0, 4)), int(rng.integers(0, 64 - 19 + 1)), int(rng.integers(0, 40 - 11 + 1)))
             for _ in range(40)]
    dev = torch.tensor([list(c) + [0] for c in crops] + [[4, 0, 0, 0], [0, 46, 0, 0], [1, 0, 30, 0], [2, 0, 0, 7]],
                       dtype=torch.int32, device=device)
    outs = []
    for f, frames in ((D.decode_set_crops, fs), (D.decode_crops, fr)):
        out = torch.full((dev.shape[0], 11, 24), S.FILL, dtype=torch.uint8, device=device)
        got, st = f(frames, tabs, dev, size, out=out, status=True)
        torch.cuda.synchronize(device)
        assert got is out
        outs.append((out.cpu().numpy(), st.cpu().tolist()))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert outs[0][1] == outs[1][1] == [0] * 40 + [MH_ERR_DIMS] * 4
    for p, c in enumerate(crops):
        assert np.array_equal(outs[0][0][p, :, :19], S.pixels([q[1] for q in pairs], c, size))
    # ... and a host list through the Python entry: validated against each crop's own frame
    got = D.decode_set_crops(fs, tabs, crops, size)
    torch.cuda.synchronize(device)
    assert np.array_equal(got.cpu().numpy()[:, :, :19], outs[0][0][:40, :, :19])


# ---- 4. rejections ---------------------------------------------------------------------------------------------

def test_rejected_descriptors(mh, device):
    fs, tabs, imgs = _set(mh, device)
    size = (8, 8)
    desc = [(2, 5, 3, 0),
            (5, 0, 0, 0),                       # frame >= n_frames
            (3, 0xFFFFFFFF, 0, 0),              # no sum of descriptor words is formed
            (1, 1, 9, 0),
            (2, 0, 0, 1),                       # reserved != 0
            (0xFFFFFFFF, 0, 0, 0),
            (0, 0, 0, 0),
            (2, 57, 0, 0),                      # x0 = W_f - w + 1
            (1, 0, 17 - 8 + 1, 0),              # y0 = H_f - h + 1
            (0, 1, 0, 0),
            (4, 512, 16, 0),
            (3, 0, 0xFFFFFFFF, 0)]
    want = [True, False, False, True, False, False, True, False, False, False, True, False]
    assert [S.fits(SIZES, [np.int64(v) for v in d], size) for d in desc] == want
    lay = S.run_crops(device, fs, tabs, desc, size)
    assert lay.rc == 0
    S.check(lay, [[S.pixels(imgs, d, size)] if ok else None for d, ok in zip(desc, want)])
    assert lay.status == [0 if ok else MH_ERR_DIMS for ok in want]
    # w > W_f, h > H_f: a crop wider (taller) than its own frame, though not than the set's largest
    for size, small in (((65, 8), (0, 1, 2)), ((8, 41), (0, 1, 2, 4))):
        desc = [(f, 0, 0, 0) for f in range(5)]
        lay = S.run_crops(device, fs, tabs, desc, size)
        S.check(lay, _expect(imgs, SIZES, desc, size))
        assert lay.status == [MH_ERR_DIMS if f in small else 0 for f in range(5)]


@pytest.mark.parametrize("what", ["reserved", "width0", "height65536", "first_block", "total_blocks_40"])
def test_rejected_geometry_records(mh, device, what):
    """A stale or corrupt record rejects its frame's crops and nothing else: the crops of the other
    frames are exact, and no byte outside them changes."""
    fs, tabs, imgs = _set(mh, device)
    lay0 = S.encoded(mh, SIZES)
    geoms = mh.frame_set_layout([p[0] for p in lay0]).geoms.astype(np.int64)
    total = fs.total_blocks
    victim, tb = 2, None
    nb = 8 * 5
    if what == "reserved":
        geoms[victim, 3] = 1
    elif what == "width0":
        geoms[victim, 1] = 0
    elif what == "height65536":
        geoms[victim, 2] = 65536
    elif what == "first_block":
        geoms[victim, 0] = total - nb + 1
    else:  # the declared blocks end before the victim's do: NB > total_blocks for the largest frame too
        victim, tb = None, 40
    size = (8, 8)
    desc = [(f, x, y, 0) for f, (W, H) in enumerate(SIZES) for x, y in ((0, 0), (W - 8, H - 8))]
    if tb is None:
        bad = {victim}
    else:   # total_blocks = 40: frames 0 (1 block at 0) and 1 (6 blocks at 1) still lie inside; 2, 3, 4 do not
        bad = {2, 3, 4}
        assert all(int(geoms[f, 0]) + (-(-W // 8)) * (-(-H // 8)) <= 40 for f, (W, H) in enumerate(SIZES[:2]))
        assert int(geoms[2, 0]) + nb > 40
    lay = S.run_crops(device, fs, tabs, desc, size, geoms=geoms, total_blocks=tb)
    assert lay.rc == 0
    S.check(lay, [None if d[0] in bad else [S.pixels(imgs, d, size)] for d in desc])
    assert lay.status == [MH_ERR_DIMS if d[0] in bad else 0 for d in desc]


def test_first_block_at_the_last_place_that_fits(mh, device):
    """first_block = total_blocks - NB is accepted: the frame is then the array's tail."""
    fs, tabs, imgs = _set(mh, device)
    geoms = mh.frame_set_layout([p[0] for p in S.encoded(mh, SIZES)]).geoms.astype(np.int64)
    assert int(geoms[4, 0]) == fs.total_blocks - 65 * 3
    desc = [(4, 3, 5, 0), (4, 512, 16, 0)]
    lay = S.run_crops(device, fs, tabs, desc, (8, 8), geoms=geoms)
    S.check(lay, _expect(imgs, SIZES, desc, (8, 8)))
    assert lay.status == [0, 0]


# ---- 5. status words ----------------------------------------------------------------------------------------------

def test_frame_status_skips_a_frames_crops(mh, device):
    import torch
    fs, tabs, imgs = _set(mh, device)
    fstatus = torch.tensor([0, 0, -9, 0, 0], dtype=torch.int32, device=device)
    size = (8, 8)
    desc = [(2, 0, 0, 0), (3, 1, 1, 0), (2, 56, 32, 0), (0, 0, 0, 0), (2, 57, 0, 0), (4, 100, 7, 0)]
    lay = S.run_crops(device, fs, tabs, desc, size, frame_status=fstatus)
    assert lay.rc == 0
    S.check(lay, [None if d[0] == 2 else [S.pixels(imgs, d, size)] for d in desc])
    assert lay.status == [-9, 0, -9, 0, MH_ERR_DIMS, 0]     # a rejected crop reports MH_ERR_DIMS first
    # the two status arrays must not alias
    lay = S.run_crops(device, fs, tabs, desc[:5], size, frame_status=fstatus, crop_status=fstatus)
    assert lay.rc == S.MH_ERR_INVALID_ARG
    S.check(lay, [None] * 5)
    assert lay.status == [0, 0, -9, 0, 0]


# ---- 6. isolation ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("victim", [0, 2, 4])
def test_a_noisy_frame_harms_only_its_own_crops(mh, device, victim):
    import torch
    fs, tabs, imgs = _set(mh, device)
    lay0 = mh.frame_set_layout([p[0] for p in S.encoded(mh, SIZES)])
    a, b = int(lay0.code_offsets[victim]), int(lay0.code_offsets[victim + 1])
    noise = np.random.default_rng(90 + victim).integers(0, 256, b - a, dtype=np.uint8)
    fs.codes[a:b] = torch.from_numpy(noise).to(device)
    size = (8, 8)
    desc = [(f, x, y, 0) for f, (W, H) in enumerate(SIZES) for x, y in ((0, 0), (W - 8, H - 8), ((W - 8) // 2, 0))]
    lay = S.run_crops(device, fs, tabs, desc, size)
    assert lay.rc == 0
    # the victim's slots may hold anything (its pixels are undecodable), but only inside their rows
    exp = [[S.pixels(imgs, d, size)] for d in desc]
    for p, d in enumerate(desc):
        if d[0] == victim:
            for y in range(8):
                o = lay.offset(p, 0, y)
                lay.buf[o: o + 8] = np.frombuffer(exp[p][0][y].tobytes(), np.uint8)
    S.check(lay, exp)
    assert lay.status == [0] * len(desc)


# ---- 7. seeded sweep, both entries ------------------------------------------------------------------------------------

def sweep_case(i):
    """Case i: 2..6 frames of seeded sizes in 1..200 x 1..200 with one 1 x 1 frame always present, a
    crop size that fits at least half the frames, and descriptors over all frames -- those of frames
    the crop does not fit are the launch's rejected ones."""
    rng = np.random.default_rng(4000 + i)
    n = int(rng.integers(2, 7))
    sizes = [(int(rng.integers(1, 201)), int(rng.integers(1, 201))) for _ in range(n - 1)]
    sizes.insert(int(rng.integers(0, n)), (1, 1))
    ws, hs = sorted(s[0] for s in sizes), sorted(s[1] for s in sizes)
    # at most the ceil(n / 2)-th largest width and height ... then shrunk until half the frames hold both
    w = int(rng.integers(1, ws[n // 2] + 1))
    h = int(rng.integers(1, hs[n // 2] + 1))
    while 2 * sum(w <= W and h <= H for W, H in sizes) < n:
        w, h = max(1, w // 2), max(1, h // 2)
    desc = []
    for f, (W, H) in enumerate(sizes):
        for _ in range(4):
            if w <= W and h <= H:
                desc.append((f, int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), 0))
            else:
                desc.append((f, 0, 0, 0))
    desc = [desc[j] for j in rng.permutation(len(desc))]
    return tuple(sizes), (w, h), desc


SWEEP = range(24)
PAIR = (1.0 / (255.0 * 0.229), -0.485 / 0.229)


def test_sweep_cases_are_mostly_accepted():
    for i in SWEEP:
        sizes, size, desc = sweep_case(i)
        assert 2 <= len(sizes) <= 6 and (1, 1) in sizes
        assert 2 * sum(size[0] <= W and size[1] <= H for W, H in sizes) >= len(sizes)
        assert 3 * sum(S.fits(sizes, d, size) for d in desc) >= len(desc), i


@pytest.mark.parametrize("i", SWEEP)
def test_seeded_sweep(mh, device, i):
    sizes, size, desc = sweep_case(i)
    fmt, tables = S.FORMATS[i % 4], S.TABLES[(i // 4) % 2]
    fs, tabs, imgs = _set(mh, device, fmt, tables, sizes, seed=100 + i)
    assert 3 * sum(S.fits(sizes, d, size) for d in desc) >= len(desc)
    lay = S.run_crops(device, fs, tabs, desc, size)
    assert lay.rc == 0
    S.check(lay, _expect(imgs, sizes, desc, size))
    assert lay.status == _statuses(sizes, desc, size)
    # ... and the normalised entry with one plane, the same descriptors (flags 0)
    nf = NH.FORMATS[i % 3]
    T = NH.table_bits(nf, *PAIR)
    lay = S.run_planes(device, fs, tabs, desc, size, nf, [PAIR])
    assert lay.rc == 0
    S.check(lay, [[T[S.pixels(imgs, d, size)]] if S.fits(sizes, d, size) else None for d in desc])
    assert lay.status == _statuses(sizes, desc, size)
