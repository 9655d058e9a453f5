"""mh_decode_set_crops_norm_planes: samples of three-plane images of DIFFERENT sizes into a normalised
[n, C, h, w] batch in one launch. Every launch goes through the C-ABI into a guarded buffer
(set_helpers.py): the gaps between rows, planes and slots and the zones around them are compared with
the fill, and every element with norm_helpers.table_bits of its plane's (scale, bias) -- libm's fmaf,
numpy's float16 cast, integer rounding for bfloat16, never the code under test -- indexed by the source
image's own slice, reversed along x where the sample is mirrored. Bit patterns, no tolerance."""
from __future__ import annotations

import numpy as np
import pytest

import norm_helpers as NH
import set_helpers as S
from norm_helpers import MIRROR
from set_helpers import MH_ERR_DIMS

pytestmark = pytest.mark.gpu

IMAGES = ((24, 16), (40, 40), (72, 33))          # three images, three planes each
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FMTS = pytest.mark.parametrize("fmt", NH.FORMATS, ids=[NH.NAMES[f] for f in NH.FORMATS])
LAYOUTS = pytest.mark.parametrize("layout", ["plane_after_plane", "plane_major"])

_T: dict = {}


def pairs(mh):
    s, b = mh.norm_coefficients(MEAN, STD)
    return [(float(x), float(y)) for x, y in zip(s, b)]


def table(mh, fmt, c):
    if (fmt, c) not in _T:
        _T[fmt, c] = NH.table_bits(fmt, *pairs(mh)[c])
        _T[fmt, c].setflags(write=False)
    return _T[fmt, c]


def _sizes(layout):
    """The frames' sizes and (first frame of image i, frame stride of its planes)."""
    n = len(IMAGES)
    if layout == "plane_after_plane":
        return tuple(s for s in IMAGES for _ in range(3)), [3 * i for i in range(n)], 1
    return tuple(IMAGES) * 3, list(range(n)), n


def _set(mh, device, layout, fmt="delta", tables="set"):
    sizes, first, ps = _sizes(layout)
    enc = S.encoded(mh, sizes, fmt, tables == "shared", seed=7)
    fs, tabs = S.upload(device, [p[0] for p in enc], tables == "shared")
    return fs, tabs, [p[1] for p in enc], sizes, first, ps


def _expected(mh, imgs, d, size, fmt, ps, C=3):
    f0, flags = int(d[0]), int(d[3])
    return [NH.expected_crop(table(mh, fmt, c), imgs[f0 + c * ps], (f0 + c * ps, d[1], d[2], flags), size)
            for c in range(C)]


def _samples(first, size, flags, rng):
    w, h = size
    out = []
    for i, (W, H) in enumerate(IMAGES):
        if w > W or h > H:
            continue
        out += [(first[i], 0, 0, flags), (first[i], W - w, H - h, flags),
                (first[i], int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), flags)]
    return out


@FMTS
@LAYOUTS
@pytest.mark.parametrize("tables", S.TABLES)
def test_three_plane_images_of_three_sizes(mh, device, layout, fmt, tables):
    """Mirrored 16 x 16 samples and plain 13 x 9 ones, over all three images, a pair per plane."""
    fs, tabs, imgs, sizes, first, ps = _set(mh, device, layout, "delta", tables)
    rng = np.random.default_rng(21)
    for size, flags in (((16, 16), MIRROR), ((13, 9), 0)):
        desc = _samples(first, size, flags, rng)
        assert len(desc) == 9
        desc = [desc[j] for j in rng.permutation(9)]
        lay = S.run_planes(device, fs, tabs, desc, size, fmt, pairs(mh), ps)
        assert lay.rc == 0
        S.check(lay, [_expected(mh, imgs, d, size, fmt, ps) for d in desc])
        assert lay.status == [0] * 9


@pytest.mark.parametrize("fmt_name", ["raw", "delta_init"])
def test_raw_and_block_init_frames(mh, device, fmt_name):
    fs, tabs, imgs, sizes, first, ps = _set(mh, device, "plane_after_plane", fmt_name)
    desc = _samples(first, (13, 9), 0, np.random.default_rng(22))
    lay = S.run_planes(device, fs, tabs, desc, (13, 9), NH.F16, pairs(mh), ps)
    assert lay.rc == 0
    S.check(lay, [_expected(mh, imgs, d, (13, 9), NH.F16, ps) for d in desc])


@FMTS
@LAYOUTS
def test_planes_of_different_sizes_reject_the_sample(mh, device, layout, fmt):
    """A descriptor whose `frame` is off by one runs into the next image: its planes differ in size,
    so the sample gets MH_ERR_DIMS and no plane of it is written -- not even plane 0, whose own
    frame could hold the crop. Its neighbours are exact."""
    fs, tabs, imgs, sizes, first, ps = _set(mh, device, layout)
    size = (16, 16)
    if layout == "plane_after_plane":   # frames 1, 2, 3 = image 0's planes 1, 2 and image 1's plane 0
        off = [(1, 0, 0, 0), (5, 3, 3, MIRROR), (2, 0, 0, 0)]
    else:                                # plane-major, stride 3: frame 0 under stride 2 mixes the images
        off = []
    good = [(first[0], 8, 0, 0), (first[1], 5, 7, MIRROR), (first[2], 56, 17, 0)]
    desc = [good[0]] + off[:1] + [good[1]] + off[1:] + [good[2]]
    lay = S.run_planes(device, fs, tabs, desc, size, fmt, pairs(mh), ps)
    assert lay.rc == 0
    S.check(lay, [None if d in off else _expected(mh, imgs, d, size, fmt, ps) for d in desc])
    assert lay.status == [MH_ERR_DIMS if d in off else 0 for d in desc]
    if layout == "plane_major":          # the right frames under the wrong stride: planes of images 0, 2, 1
        lay = S.run_planes(device, fs, tabs, good, size, fmt, pairs(mh), 2)
        S.check(lay, [None] * 3)
        assert lay.status == [MH_ERR_DIMS] * 3


def test_rejected_samples_and_records(mh, device):
    fs, tabs, imgs, sizes, first, ps = _set(mh, device, "plane_after_plane")
    size = (16, 16)
    desc = [(0, 8, 0, 0),
            (7, 0, 0, 0),                    # frame > n_frames - 1 - 2: plane 2 would be frame 9
            (3, 25, 0, 0),                   # x0 > 40 - 16
            (3, 24, 24, MIRROR),
            (6, 0, 18, 0),                   # y0 > 33 - 16
            (3, 0, 0, 2),                    # a flag bit other than MH_CROP_MIRROR
            (0xFFFFFFFF, 0, 0, 0),
            (6, 56, 17, MIRROR)]
    ok = [True, False, False, True, False, False, False, True]
    lay = S.run_planes(device, fs, tabs, desc, size, NH.F16, pairs(mh), ps)
    assert lay.rc == 0
    S.check(lay, [_expected(mh, imgs, d, size, NH.F16, ps) if k else None for d, k in zip(desc, ok)])
    assert lay.status == [0 if k else MH_ERR_DIMS for k in ok]
    # the crop does not fit the 24 x 16 image at all (w > W_f is judged before W_f - w is formed)
    lay = S.run_planes(device, fs, tabs, [(0, 0, 0, 0), (3, 0, 0, 0)], (25, 16), NH.F32, pairs(mh), ps)
    S.check(lay, [None, _expected(mh, imgs, (3, 0, 0, 0), (25, 16), NH.F32, ps)])
    assert lay.status == [MH_ERR_DIMS, 0]
    # MH_CROP_MIRROR on a width that is no multiple of 8
    lay = S.run_planes(device, fs, tabs, [(3, 0, 0, MIRROR), (3, 0, 0, 0)], (13, 9), NH.BF16, pairs(mh), ps)
    S.check(lay, [None, _expected(mh, imgs, (3, 0, 0, 0), (13, 9), NH.BF16, ps)])
    assert lay.status == [MH_ERR_DIMS, 0]
    # a corrupt record on plane 2 of image 1 rejects the whole sample, in every one of its workgroups
    geoms = mh.frame_set_layout([p[0] for p in S.encoded(mh, sizes, "delta", False, 7)]).geoms.astype(np.int64)
    geoms[5, 3] = 1
    desc = [(3, 0, 0, 0), (0, 0, 0, 0), (6, 1, 1, 0)]
    lay = S.run_planes(device, fs, tabs, desc, size, NH.F16, pairs(mh), ps, geoms=geoms)
    S.check(lay, [None] + [_expected(mh, imgs, d, size, NH.F16, ps) for d in desc[1:]])
    assert lay.status == [MH_ERR_DIMS, 0, 0]


@FMTS
def test_one_plane_equals_decode_crops_normalized(mh, device, fmt):
    """n_planes == 1 over a set of one size is byte-identical, raster and statuses, to
    decode_crops_normalized on the same frames packed as DeviceFrames."""
    import torch
    from metalhuffman_amd import decoder as D
    sizes = ((64, 40),) * 4
    enc = S.encoded(mh, sizes, "delta", False, seed=3)
    efs = [p[0] for p in enc]
    fs, tabs = S.upload(device, efs)
    fr = D.DeviceFrames.pack(efs, device, shared_table=False)
    rng = np.random.default_rng(6)
    size = (16, 11)
    rows = [[int(rng.integers(0, 4)), int(rng.integers(0, 49)), int(rng.integers(0, 30)), int(rng.integers(0, 2))]
            for _ in range(30)] + [[4, 0, 0, 0], [0, 49, 0, 0], [1, 0, 0, 2]]
    dev = torch.tensor(rows, dtype=torch.int32, device=device)
    scale, bias = pairs(mh)[1]
    dt = NH.torch_dtype(fmt)
    fill = lambda: torch.full((33 * 11 * 16 * NH.ESIZE[fmt],), S.FILL, dtype=torch.uint8,
                              device=device).view(dt).view(33, 1, 11, 16)
    a, sa = D.decode_set_crops_normalized_planes(fs, tabs, dev, size, dt, [scale], [bias], n_planes=1, out=fill(),
                                                 status=True)
    b, sb = D.decode_crops_normalized(fr, tabs, dev, size, dt, scale, bias, out=fill().view(33, 11, 16), status=True)
    torch.cuda.synchronize(device)
    assert np.array_equal(NH.bits_of(a, fmt).reshape(33, 11, 16), NH.bits_of(b, fmt))
    assert sa.cpu().tolist() == sb.cpu().tolist() == [0] * 30 + [MH_ERR_DIMS] * 3
    T = NH.table_bits(fmt, scale, bias)
    for p, r in enumerate(rows[:30]):
        assert np.array_equal(NH.bits_of(a, fmt)[p, 0], NH.expected_crop(T, enc[r[0]][1], r, size))


def test_stride_zero_replicates_one_gray_frame(mh, device):
    fs, tabs, imgs, sizes, first, ps = _set(mh, device, "plane_after_plane")
    size = (16, 16)
    desc = [(8, 56, 17, 0), (0, 8, 0, MIRROR), (4, 3, 3, 0)]      # the last frame included
    lay = S.run_planes(device, fs, tabs, desc, size, NH.F16, pairs(mh), 0)
    assert lay.rc == 0
    S.check(lay, [_expected(mh, imgs, d, size, NH.F16, 0) for d in desc])
    assert lay.status == [0, 0, 0]
    assert all((lay.buf[lay.offset(0, c, 0): lay.offset(0, c, 0) + 32] !=
                lay.buf[lay.offset(0, 0, 0): lay.offset(0, 0, 0) + 32]).any() for c in (1, 2))


def test_a_status_word_on_plane_2_skips_the_sample(mh, device):
    import torch
    fs, tabs, imgs, sizes, first, ps = _set(mh, device, "plane_after_plane")
    fstatus = torch.zeros(9, dtype=torch.int32, device=device)
    fstatus[5] = -5
    size = (16, 16)
    desc = [(3, 0, 0, 0), (0, 0, 0, 0), (3, 24, 24, MIRROR), (6, 0, 0, 0), (3, 25, 0, 0)]
    lay = S.run_planes(device, fs, tabs, desc, size, NH.BF16, pairs(mh), ps, frame_status=fstatus)
    assert lay.rc == 0
    S.check(lay, [None if d[0] == 3 else _expected(mh, imgs, d, size, NH.BF16, ps) for d in desc])
    assert lay.status == [-5, 0, -5, 0, MH_ERR_DIMS]
    lay = S.run_planes(device, fs, tabs, desc, size, NH.BF16, pairs(mh), ps, frame_status=fstatus,
                       crop_status=fstatus[:5])
    assert lay.rc == S.MH_ERR_INVALID_ARG
    S.check(lay, [None] * 5)
