"""mh_decode_crops_norm_planes: samples of C planes -- the same crop of C frames, each under its own
(scale, bias) -- decoded into a normalised [n, C, h, round_up(w, 8)] tensor in one launch. Every slot
is prefilled with 0xA5 bytes; the expected elements are norm_helpers.table_bits of the plane's pair
(libm's fmaf, numpy's float16 cast, integer rounding for bfloat16 -- never the code under test) indexed
by the numpy slice of the oracle's decode_frame_shader of the plane's FULL frame
(region_helpers.frame_set), reversed along x where the sample is mirrored. Every comparison is on bit
patterns; there is no tolerance. Columns >= w of a written row are the only elements not compared.

The frames are region_helpers' 597 x 67 ones (75 x 9 blocks, partial right and bottom blocks), six per
flavour: two images of three planes. A sample is (frame, x0, y0, flags); plane c is frame + c *
plane_stride. The whole slot -- every plane -- of a rejected or skipped sample must keep the fill."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import norm_helpers as NH
import region_helpers as R
from norm_helpers import MIRROR, up8
from region_helpers import FILL, H, W

pytestmark = pytest.mark.gpu

MH_ERR_DIMS = -2
NFR = 6
# four distinct pairs, one scale negative: a swapped or shared pair shows in every element
PAIRS = [(1.0 / (255.0 * 0.229), -0.485 / 0.229), (-1.5, 3.0), (1.0 / 255.0, 0.25), (0.125, -7.0)]
FMTS = pytest.mark.parametrize("fmt", NH.FORMATS, ids=[NH.NAMES[f] for f in NH.FORMATS])

_TABLES: dict = {}


def table(fmt, c):
    """T_c of the format, computed once and left unchanged."""
    if (fmt, c) not in _TABLES:
        _TABLES[fmt, c] = NH.table_bits(fmt, *PAIRS[c])
        _TABLES[fmt, c].setflags(write=False)
    return _TABLES[fmt, c]


def _frames(mh, oracle, flavour="general"):
    return R.frame_set(mh, oracle, flavour, n=NFR)


def _efs(frames):
    return [f[0] for f in frames]


def _wants(frames):
    return [f[1] for f in frames]


def _filled(device, shape, fmt):
    """A tensor of the format's dtype whose every BYTE is FILL."""
    import torch
    raw = torch.full((int(np.prod(shape)) * NH.ESIZE[fmt],), FILL, dtype=torch.uint8, device=device)
    return raw.view(NH.torch_dtype(fmt)).view(*shape)


def _fill_bits(fmt):
    return NH.BITS[fmt](int.from_bytes(bytes([FILL]) * NH.ESIZE[fmt], "little"))


def _coeffs(C):
    return [p[0] for p in PAIRS[:C]], [p[1] for p in PAIRS[:C]]


def decode_host(device, fr, tabs, crops, size, fmt, C=3, ps=1, **kw):
    """decode_crops_normalized_planes into slots prefilled with FILL bytes -> the bit patterns
    [n, C, h, round_up(w, 8)] on the host (and the per-sample status list when status=True is passed)."""
    import torch
    from metalhuffman_amd import decoder as D
    n = len(crops)
    out = _filled(device, (n, C, size[1], up8(size[0])), fmt)
    got = D.decode_crops_normalized_planes(fr, tabs, crops, size, NH.torch_dtype(fmt), *_coeffs(C), plane_stride=ps,
                                           out=out, **kw)
    torch.cuda.synchronize(device)
    if kw.get("status") is True:
        assert got[0] is out
        return NH.bits_of(out, fmt), got[1].cpu().tolist()
    assert got is out
    return NH.bits_of(out, fmt)


def check(got, crops, size, wants, fmt, C=3, ps=1):
    """Plane c of slot p holds T_c[the numpy slice of frame + c * ps's expected raster], mirrored where
    the sample is flagged, in its first w columns."""
    w, h = size
    assert got.shape == (len(crops), C, h, up8(w)) and got.dtype == NH.BITS[fmt], (got.shape, got.dtype)
    for p, s in enumerate(crops):
        for c in range(C):
            exp = NH.expected_crop(table(fmt, c), wants[int(s[0]) + c * ps], s, size)
            if not np.array_equal(got[p, c, :, :w], exp):
                ys, xs = np.nonzero(got[p, c, :, :w] != exp)
                raise AssertionError(
                    f"sample {p} = {tuple(int(v) for v in s)} of {size}, plane {c}: {ys.size} wrong element(s), first "
                    f"at row {int(ys[0])}, column {int(xs[0])}: {int(got[p, c, ys[0], xs[0]]):#x}, expected "
                    f"{int(exp[ys[0], xs[0]]):#x}")


def test_the_pairs_tell_the_planes_apart():
    assert len({p for p in PAIRS}) == 4 and sum(p[0] < 0 for p in PAIRS[:3]) == 1
    for fmt in NH.FORMATS:
        for a in range(4):
            for b in range(a):
                assert (table(fmt, a) != table(fmt, b)).sum() >= 250, (fmt, a, b)


# ---- 1. every sub-block origin -------------------------------------------------------------------------

def _all_origins(w, h, mirror_alternate, first_frames):
    """64 samples of w x h, (x0 & 7, y0 & 7) every pair, over the frames a sample may start at."""
    crops = []
    for dy in range(8):
        for dx in range(8):
            i = 8 * dy + dx
            bx = (i * 7) % ((W - w - 7) // 8 + 1)
            by = min((i * 5) % 7, (H - h - dy) // 8)
            crops.append((i % first_frames, 8 * bx + dx, 8 * by + dy, (i & 1) if mirror_alternate else 0))
    return crops


@FMTS
@pytest.mark.parametrize("tables", ["shared", "set"])
@pytest.mark.parametrize("ps", [1, 2])
@pytest.mark.parametrize("w,mirrored", [(19, False), (24, True)])
def test_all_sub_block_origins(mh, oracle, device, tables, fmt, ps, w, mirrored):
    frames = _frames(mh, oracle)
    fr, tabs = R.upload(device, _efs(frames), tables)
    crops = _all_origins(w, 13, mirrored, NFR - 2 * ps)
    assert {(c[1] & 7, c[2] & 7) for c in crops} == {(dx, dy) for dx in range(8) for dy in range(8)}
    assert {c[0] for c in crops} == set(range(NFR - 2 * ps)) and max(c[0] for c in crops) + 2 * ps == NFR - 1
    assert sum(c[3] for c in crops) == (32 if mirrored else 0)
    got, st = decode_host(device, fr, tabs, crops, (w, 13), fmt, 3, ps, status=True)
    check(got, crops, (w, 13), _wants(frames), fmt, 3, ps)
    assert st == [0] * 64


# ---- 2. plane counts and strides -----------------------------------------------------------------------

@FMTS
@pytest.mark.parametrize("size", [(1, 1), (9, 9), (17, 8), (W, H)])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_plane_counts_and_strides(mh, oracle, device, C, size, fmt):
    """C = 1..4 at every frame stride that fits six frames, 0 included (C differently normalised
    tables of ONE frame); each list holds a sample whose last plane is the batch's last frame and one
    that starts at frame 0, at the frame's corners and at odd origins."""
    frames = _frames(mh, oracle)
    fr, ts = R.upload(device, _efs(frames), "set")
    w, h = size
    for ps in (0, 1, 2, 5):
        if (C - 1) * ps >= NFR:
            continue
        last = NFR - 1 - (C - 1) * ps
        crops = [(last, W - w, H - h, 0), (0, 0, 0, 0), (last, 0, H - h, 0), (last // 2, W - w, 0, 0),
                 (0, min(5, W - w), min(3, H - h), 0)]
        assert max(c[0] for c in crops) + (C - 1) * ps == NFR - 1
        got, st = decode_host(device, fr, ts, crops, size, fmt, C, ps, status=True)
        check(got, crops, size, _wants(frames), fmt, C, ps)
        assert st == [0] * len(crops)
        if ps == 0 and C > 1:      # the planes of a sample are one picture under different maps
            assert all((got[:, c] != got[:, 0]).any() for c in range(1, C))


# ---- 3. planes under different Huffman tables -------------------------------------------------------------

@FMTS
def test_planes_under_different_tables(mh, oracle, device, fmt):
    """One batch of nine frames, plane-major: three `general` (13-bit table with escapes), three
    `noesc` (escape-free step) and three `flat8` (byte loop), a table per frame. Plane c of a sample
    takes another decode loop than plane c - 1, in one launch."""
    from metalhuffman_amd import decoder as D
    sets = [R.frame_set(mh, oracle, f) for f in ("general", "noesc", "flat8")]
    frames = [f for s in sets for f in s]
    assert len(frames) == 9 and [R.lens(s[0][0])[:2] for s in sets] == [(1, 16), (1, 13), (8, 8)]
    efs = _efs(frames)
    fr = D.DeviceFrames.pack(efs, device, shared_table=False)
    ts = D.DeviceTableSet.from_canonical_headers(np.stack([ef.canon for ef in efs]), device)
    for size, crops in (((40, 20), [(0, 3, 5, 0), (1, 3, 47, MIRROR), (2, 3, 0, 0), (1, 297, 30, MIRROR),
                                    (2, 557, 12, MIRROR), (0, 0, 0, MIRROR), (1, 557, 47, 0), (2, 251, 29, 0)]),
                        ((304, 20), [(0, 3, 5, 0), (1, 3, 47, MIRROR), (2, 293, 30, 0)])):
        got, st = decode_host(device, fr, ts, crops, size, fmt, 3, 3, status=True)
        check(got, crops, size, _wants(frames), fmt, 3, 3)
        assert st == [0] * len(crops)
    # ... and the planes in the other order, by a list that starts at the flat8 frames with stride 0
    got = decode_host(device, fr, ts, [(6, 1, 1, 0), (3, 2, 2, 0), (0, 3, 3, 0)], (24, 9), fmt, 2, 0)
    check(got, [(6, 1, 1, 0), (3, 2, 2, 0), (0, 3, 3, 0)], (24, 9), _wants(frames), fmt, 2, 0)


# ---- 4. samples the kernel rejects ---------------------------------------------------------------------------

@FMTS
@pytest.mark.parametrize("ps", [1, 2])
def test_rejected_samples(mh, oracle, device, ps, fmt):
    """One launch of valid samples and one of each rejected kind. The descriptors are a device tensor,
    so only the kernel sees them. A rejected sample reports MH_ERR_DIMS and EVERY plane of its slot
    keeps the fill bytewise; its neighbours are exact, status 0."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = _frames(mh, oracle)
    fr, ts = R.upload(device, _efs(frames), "set")
    w, h, C = 19, 21, 3
    last = NFR - 1 - (C - 1) * ps                 # the last frame a sample may start at
    desc = [(0, 3, 5, 0), (last + 1, 0, 0, 0), (last, W - w, H - h, 0), (0xFFFFFFFF, 0, 0, 0), (NFR - 1, 1, 1, 0),
            (1, 9, 9, 0), (0, W - w + 1, 0, 0), (last, 0, H - h + 1, 0), (0, 0xFFFFFFFF, 0, 0), (0, 0, 0xFFFFFFFF, 0),
            (last, 0, H - h, 0), (1, 5, 2, 2), (0, 7, 7, 0x80000001), (0, 9, 9, MIRROR), (NFR, 0, 0, 0),
            (0x80000000, 0, 0, 0), (0, W - w, 0, 0)]
    valid = [0, 2, 5, 10, 16]
    crops = torch.from_numpy(np.array(desc, np.uint32).view(np.int32)).to(device)
    n = len(desc)
    out = _filled(device, (n, C, h, up8(w)), fmt)
    status = torch.full((n,), 77, dtype=torch.int32, device=device)
    assert D.decode_crops_normalized_planes(fr, ts, crops, (w, h), NH.torch_dtype(fmt), *_coeffs(C), plane_stride=ps,
                                            out=out, status=status) is out
    torch.cuda.synchronize(device)
    got, st = NH.bits_of(out, fmt), status.cpu().tolist()
    assert st == [0 if p in valid else MH_ERR_DIMS for p in range(n)], st
    for p in range(n):
        if p not in valid:
            assert (got[p] == _fill_bits(fmt)).all(), f"sample {p} = {desc[p]}: its slot was written"
    check(got[valid], [desc[p] for p in valid], (w, h), _wants(frames), fmt, C, ps)
    # a width that is a multiple of 8 accepts the same mirrored descriptor
    got8 = decode_host(device, fr, ts, [desc[13], desc[0]], (24, h), fmt, C, ps)
    check(got8, [desc[13], desc[0]], (24, h), _wants(frames), fmt, C, ps)


# ---- 5. skipped samples: written whole or not at all -------------------------------------------------------------

@FMTS
def test_skipped_samples(mh, oracle, device, fmt):
    """Frame status words [0, -3, 0, -9, 0, -5], three planes. A sample is skipped when ANY of its
    frames has a non-zero word, its status is the first such word in plane order, and then no plane
    of it is written, the planes of healthy frames included. Under plane stride 1: frame 0 meets -3 on
    plane 1 only; frame 1 meets -3 on plane 0 and -9 on plane 2 (plane 0's word); frames 2 and 3 meet
    -9. Under stride 2 the sample of frames (0, 2, 4) uses no marked frame and is MH_OK beside its
    skipped neighbour. A rejected sample never reads the words; without the status array everything
    decodes."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = _frames(mh, oracle)
    fr, ts = R.upload(device, _efs(frames), "set")
    words = [0, -3, 0, -9, 0, -5]
    marked = D.DeviceTableSet(ts.luts, torch.tensor(words, dtype=torch.int32, device=device))
    size, C = (24, 13), 3
    crops = [(0, 3, 5, 0), (1, 100, 9, MIRROR), (2, 7, 7, 0), (3, 0, 0, 0), (0, 301, 33, MIRROR), (4, 0, 0, 0),
             (2, 250, 50, MIRROR)]
    on_device = torch.tensor(crops, dtype=torch.int32, device=device)   # (a host list with sample 5 is a ValueError)
    got, st = decode_host(device, fr, marked, on_device, size, fmt, C, 1, status=True, skip_rejected=True)
    assert st == [-3, -3, -9, -9, -3, MH_ERR_DIMS, -9], st
    assert (got == _fill_bits(fmt)).all(), "a skipped sample's plane was written"
    # planes two frames apart: (0, 2, 4) is healthy; (1, 3, 5) meets -3, -9, -5 and reports the first
    two = [(1, 9, 9, 0), (0, 3, 5, MIRROR), (1, 0, 0, 0)]
    got, st = decode_host(device, fr, marked, two, size, fmt, C, 2, status=True)
    assert st == [-3, 0, -3], st
    assert (got[[0, 2]] == _fill_bits(fmt)).all()
    check(got[[1]], [two[1]], size, _wants(frames), fmt, C, 2)
    # two planes, two frames apart: (2, 4) and (0, 2) are healthy, (1, 3) and (3, 5) are not
    mix = [(1, 3, 5, 0), (2, 9, 9, MIRROR), (0, 1, 1, 0), (3, 40, 40, 0)]
    got, st = decode_host(device, fr, marked, mix, size, fmt, 2, 2, status=True)
    assert st == [-3, 0, 0, -9], st
    assert (got[[0, 3]] == _fill_bits(fmt)).all()
    check(got[[1, 2]], [mix[1], mix[2]], size, _wants(frames), fmt, 2, 2)
    # one frame under three maps: its own word decides
    one = [(0, 1, 1, 0), (3, 5, 5, MIRROR), (2, 2, 2, 0), (5, 9, 9, 0), (4, 5, 5, MIRROR)]
    got, st = decode_host(device, fr, marked, one, size, fmt, 3, 0, status=True)
    assert st == [0, -9, 0, -5, 0], st
    assert (got[[1, 3]] == _fill_bits(fmt)).all()
    check(got[[0, 2, 4]], [one[0], one[2], one[4]], size, _wants(frames), fmt, 3, 0)
    # the words ignored on request: the tables are good, so every sample decodes
    got, st = decode_host(device, fr, marked, crops[:5], size, fmt, C, 1, status=True, skip_rejected=False)
    assert st == [0] * 5
    check(got, crops[:5], size, _wants(frames), fmt, C, 1)


# ---- 6. write containment ----------------------------------------------------------------------------------

@FMTS
@pytest.mark.parametrize("w,flags", [(19, 0), (24, MIRROR)])
@pytest.mark.parametrize("flavour", ["general", "flat8"])
def test_write_containment(mh, oracle, device, flavour, w, flags, fmt):
    """One launch through the C-ABI into slots laid out inside a buffer of seeded random bytes: d_out
    at 16 mod 32, pitch = the row's bytes + 48, plane stride = h * pitch + 32, sample stride = C * plane
    stride + 80 -- every level leaves a gap -- the first sample at the buffer's first byte and the last
    sample's last row ending at its last byte. The round_up(w, 8) * E bytes of each of the h rows of
    each plane may change -- the first w elements to their exact values -- and EVERY other byte of the
    buffer must be as it was: the rows above a crop, the row padding, the gaps between planes and
    between slots, and the whole slot of the rejected sample in the middle of the list."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    E = NH.ESIZE[fmt]
    h, C, ps = 13, 3, 1
    crops = [(0, 5, 1, flags), (3, 251, 54, flags), (2, W - w - 1, 3, flags), (4, 13, 9, flags), (1, 1, 47, flags),
             (3, 339, 30, flags)]
    rejected = 3                                         # frame 4 + 2 planes: no frame 6
    assert all(c[1] & 7 and c[2] & 7 for c in crops)
    frames = _frames(mh, oracle, flavour)
    fr, tabs = R.upload(device, _efs(frames))
    n, row = len(crops), up8(w) * E
    pitch = row + 48
    plane = h * pitch + 32
    stride = C * plane + 80
    assert pitch % 16 == 0 and plane % 16 == 0 and stride % 16 == 0 and plane > h * pitch and stride > C * plane
    size = (n - 1) * stride + (C - 1) * plane + (h - 1) * pitch + row
    pattern = np.random.default_rng(w * 8 + fmt).integers(0, 256, 16 + size, dtype=np.uint8)
    buf = torch.from_numpy(pattern.copy()).to(device)
    assert buf.data_ptr() % 32 == 0
    d_out = buf.data_ptr() + 16                                   # 16 mod 32; the slots end with the buffer
    desc = torch.tensor([list(c) for c in crops], dtype=torch.int32, device=device)
    status = torch.full((n,), 77, dtype=torch.int32, device=device)
    st, _ = D._frames_entry(fr)
    scale, bias = _coeffs(C)
    arr = ctypes.c_float * C
    N.check(N.lib().mh_decode_crops_norm_planes(ctypes.byref(st), desc.data_ptr(), n, w, h, fmt, C, ps, arr(*scale),
                                                arr(*bias), tabs.lut.data_ptr(), 0, None, status.data_ptr(), d_out,
                                                pitch, plane, stride,
                                                torch.cuda.current_stream(device).cuda_stream),
            "mh_decode_crops_norm_planes")
    torch.cuda.synchronize(device)
    assert status.cpu().tolist() == [MH_ERR_DIMS if p == rejected else 0 for p in range(n)]
    after = buf.cpu().numpy()
    may = np.zeros(after.size, bool)
    for p, s in enumerate(crops):
        if p == rejected:
            continue
        for c in range(C):
            exp = NH.expected_crop(table(fmt, c), _wants(frames)[s[0] + c * ps], s, (w, h))
            for y in range(h):
                o = 16 + p * stride + c * plane + y * pitch
                may[o: o + row] = True
                got = after[o: o + w * E].view(NH.BITS[fmt])
                assert np.array_equal(got, exp[y]), (p, c, y)
    changed = np.flatnonzero((after != pattern) & ~may)
    assert changed.size == 0, f"{changed.size} byte(s) written outside the rows, first at {int(changed[0])}"


# ---- 7. flags, block_init, descriptors -----------------------------------------------------------------------

@FMTS
@pytest.mark.parametrize("flavour", ["no_delta", "block_init"])
def test_no_delta_and_block_init(mh, oracle, device, flavour, fmt):
    frames = _frames(mh, oracle, flavour)
    assert bool(frames[0][0].flags & 1) == (flavour == "no_delta")
    assert (frames[0][0].block_init is not None) == (flavour == "block_init")
    fr, ts = R.upload(device, _efs(frames), "set")
    size = (72, 21)
    crops = [(0, 0, 0, MIRROR), (3, 520, 0, 0), (1, 243, 46, MIRROR), (2, 517, 41, 0), (3, 1, 1, MIRROR)]
    got = decode_host(device, fr, ts, crops, size, fmt)
    check(got, crops, size, _wants(frames), fmt)


@FMTS
def test_any_order(mh, oracle, device, fmt):
    """MH_FLAG_ANY_ORDER: the launch may start while earlier work on the stream drains; the stream is
    idle here, and the picture is the same."""
    import torch
    from metalhuffman_amd import _native as N
    frames = _frames(mh, oracle)
    fr, ts = R.upload(device, _efs(frames), "set")
    size = (72, 21)
    crops = [(0, 0, 0, MIRROR), (1, 520, 0, 0), (0, 243, 46, MIRROR)]
    torch.cuda.synchronize(device)
    got = decode_host(device, fr, ts, crops, size, fmt, 3, 2, extra_flags=N.MH_FLAG_ANY_ORDER)
    check(got, crops, size, _wants(frames), fmt, 3, 2)


@FMTS
def test_device_descriptors_in_place(mh, oracle, device, fmt):
    """An int32 [n, 4] device tensor is used where it lies: rewritten in place between two calls, the
    second call sees the new samples, and the tensor is not changed. [n, 3] and host lists give the
    same picture; out = None is zero-filled, typed and [n, C, h, round_up(w, 8)]."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = _frames(mh, oracle)
    fr, tabs = R.upload(device, _efs(frames))
    size = (80, 21)
    a = [(0, 0, 0, 0), (2, 517, 0, MIRROR), (1, 243, 46, 0), (3, 517, 41, MIRROR), (2, 1, 1, 0)]
    b = [(1, 5, 3, MIRROR), (3, 100, 20, 0), (2, 9, 9, MIRROR), (1, 0, 46, 0), (0, 517, 0, MIRROR)]
    c4 = torch.tensor(a, dtype=torch.int32, device=device)
    assert c4.is_contiguous() and c4.data_ptr() % 16 == 0
    ptr = c4.data_ptr()
    got = decode_host(device, fr, tabs, c4, size, fmt)
    check(got, a, size, _wants(frames), fmt)
    c4.copy_(torch.tensor(b, dtype=torch.int32, device=device))
    got = decode_host(device, fr, tabs, c4, size, fmt)
    check(got, b, size, _wants(frames), fmt)
    assert c4.data_ptr() == ptr and c4.cpu().tolist() == [list(x) for x in b]
    plain = [x[:3] for x in a]
    c3 = torch.tensor(plain, dtype=torch.int32, device=device)
    for form, want in ((c3, plain), (plain, plain), (np.asarray(plain), plain), (np.asarray(a), a)):
        got = decode_host(device, fr, tabs, form, size, fmt)
        check(got, [tuple(x) + (0,) * (4 - len(x)) for x in want], size, _wants(frames), fmt)
    out, st = D.decode_crops_normalized_planes(fr, tabs, [(3, 0, 0)], size, NH.torch_dtype(fmt), *_coeffs(3),
                                               status=True)
    torch.cuda.synchronize(device)
    assert out.dtype is NH.torch_dtype(fmt) and tuple(out.shape) == (1, 3, 21, 80) and st.cpu().tolist() == [0]
    check(NH.bits_of(out, fmt), [(3, 0, 0, 0)], size, _wants(frames), fmt)


# ---- 8. one plane is decode_crops_normalized -----------------------------------------------------------------------

@FMTS
def test_one_plane_equals_the_normalised_crops(mh, oracle, device, fmt):
    """C = 1: the first w columns are decode_crops_normalized's on the same crops, whatever plane_stride
    says -- and both are the expectation."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = _frames(mh, oracle)
    fr, ts = R.upload(device, _efs(frames), "set")
    for size, flags in (((19, 13), 0), ((24, 13), MIRROR), ((W, H), 0)):
        w, h = size
        crops = [(5, W - w, H - h, flags), (0, 0, 0, 0), (3, min(5, W - w), min(3, H - h), flags),
                 (4, (W - w) // 2, (H - h) // 2, 0)]
        ref = _filled(device, (len(crops), h, up8(w)), fmt)
        D.decode_crops_normalized(fr, ts, crops, size, NH.torch_dtype(fmt), *PAIRS[0], out=ref)
        torch.cuda.synchronize(device)
        ref = NH.bits_of(ref, fmt)
        for ps in (1, 0, 1000):
            got = decode_host(device, fr, ts, crops, size, fmt, 1, ps)
            assert np.array_equal(got[:, 0, :, :w], ref[:, :, :w]), (size, ps)
            check(got, crops, size, _wants(frames), fmt, 1, 0)


# ---- 9. the launch shape and the persistent loop -------------------------------------------------------------------

def _tiles(size):
    ow = (size[0] + 7) // 8
    return ((size[1] + 14) // 8) * ((ow + 62) // 63)


@FMTS
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("size,tiles", [((19, 13), 3), ((W, H), 20), ((512, 10), 6)])
def test_shape_rule(mh, oracle, device, size, tiles, C, fmt):
    """mh_decode_crops' rule over n_crops * n_planes units with this kernel's occupancy: G =
    clamp(ceil(R / (n C)), 1, ceil(CBH S / 8)), R = CUs x 1, 2 or 3 workgroups per CU (53,280 B of LDS
    admit no more)."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = _frames(mh, oracle)
    fr, _ = R.upload(device, _efs(frames))
    assert _tiles(size) == tiles
    most = -(-tiles // 8)
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    dt = NH.torch_dtype(fmt)
    occs = set()
    for n in (1, 2, 100, cus, 2 * cus, 3 * cus, 3 * cus + 1, 65536):
        G, waves = D.decode_crops_normalized_planes_shape(fr, n, size, dt, C)
        assert waves == 8
        fit = [o for o in (1, 2, 3) if G == min(max(-(-cus * o // (n * C)), 1), most)]
        assert fit, (n, C, G, cus, most)
        occs.add(tuple(fit))
    assert D.decode_crops_normalized_planes_shape(fr, 65536, size, dt, C)[0] == 1
    assert set.intersection(*(set(f) for f in occs)), occs    # one occupancy explains every answer
    if C == 1:
        assert D.decode_crops_normalized_planes_shape(fr, 1, size, dt, 1)[0] == most


@FMTS
def test_persistent_loop_many_units(mh, oracle, device, fmt):
    """200 samples x 3 planes of 40 x 20: 600 units of four tiles, a workgroup each, so the grid's
    unit -> (sample, plane) split runs far past the first samples and workgroups queue behind the
    resident ones. Seeded origins, half of the samples mirrored, both plane strides."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = _frames(mh, oracle)
    fr, ts = R.upload(device, _efs(frames), "set")
    size, n, C = (40, 20), 200, 3
    G, waves = D.decode_crops_normalized_planes_shape(fr, n, size, NH.torch_dtype(fmt), C)
    assert waves == 8 and 1 <= G <= -(-_tiles(size) // 8)
    for ps in (1, 2):
        rng = np.random.default_rng(2027 + ps)
        crops = np.stack([rng.integers(0, NFR - 2 * ps, n), rng.integers(0, W - size[0] + 1, n),
                          rng.integers(0, H - size[1] + 1, n), rng.integers(0, 2, n)], axis=1)
        assert len({int(v) & 7 for v in crops[:, 1]}) == 8 and len({int(v) & 7 for v in crops[:, 2]}) == 8
        got, st = decode_host(device, fr, ts, crops, size, fmt, C, ps, status=True)
        check(got, crops.tolist(), size, _wants(frames), fmt, C, ps)
        assert st == [0] * n
