"""The C-ABI of the frame-set entries (include/metalhuffman.h: mh_frame_geom, mh_decode_set_crops,
mh_decode_set_crops_norm_planes and their *_shape twins): exported, the record's layout, and every
host check made before any HIP call, with fake pointers -- the parents' checks in the parents' order
(tests/test_crops_abi.py, tests/test_crops_planes_abi.py), the set's own beside a NULL or misaligned
d_crops, and dims read as the set's maxima with the block counts ignored. CPU only."""
from __future__ import annotations

import ctypes

import pytest

INVALID, DIMS, CAPACITY, ALIGN, HIP = -1, -2, -4, -6, -7
LUTS, OUT, CROPS, FSTATUS, CSTATUS, GEOMS = 0x60000, 0x50000, 0x90000, 0xA0000, 0xB0000, 0xC0000
CW, CH = 250, 190
PITCH, CSTRIDE = 256, 256 * CH
NPITCH = 256 * 2                       # fp16 rows of round_up(250, 8) elements
NPLANE = NPITCH * CH
NSTRIDE = 3 * NPLANE
F16 = 0


def _frame(**kw):
    """A set the entries accept: maxima 2045 x 1531, four frames; the block counts are deliberately
    NOT those of the maxima (they are ignored), and the table fields are NULL / 0."""
    from metalhuffman_amd import _native as N
    fr = N.mh_frame()
    fr.d_block_offsets = 0x10000
    fr.d_codes = 0x20000
    fr.codes_bytes = 4096
    fr.d_frame_code_offsets = 0x80000
    fr.dims = N.mh_dims(2045, 1531, 0, 0xFFFFFFFF)
    fr.n_frames = 4
    for k, v in kw.items():
        setattr(fr, k, v)
    return fr


def _short(**kw):
    """Stops an otherwise accepted call at the last-but-one capacity rule, ahead of any HIP call."""
    return _frame(**dict(dict(codes_bytes=2), **kw))


def _stride(mh):
    return (int(mh.lib().mh_lut_bytes()) + 15) // 16 * 16


def _crops(mh, fr=None, geoms=GEOMS, total=1000, crops=CROPS, n=4, size=(CW, CH), luts=LUTS, stride=None,
           fstatus=None, cstatus=None, out=OUT, pitch=PITCH, cstride=CSTRIDE):
    from metalhuffman_amd import _native as N
    fr = _frame() if fr is None else fr
    return N.lib().mh_decode_set_crops(ctypes.byref(fr) if fr is not False else None, geoms, total, crops, n,
                                       size[0], size[1], luts, _stride(mh) if stride is None else stride, fstatus,
                                       cstatus, out, pitch, cstride, None)


def _planes(mh, fr=None, geoms=GEOMS, total=1000, crops=CROPS, n=4, size=(CW, CH), fmt=F16, C=3, ps=1,
            scale=(1.0, 2.0, 3.0, 4.0), bias=(0.0, 0.5, 1.0, 1.5), luts=LUTS, stride=None, fstatus=None,
            cstatus=None, out=OUT, pitch=NPITCH, plane=NPLANE, cstride=NSTRIDE):
    from metalhuffman_amd import _native as N
    fr = _frame() if fr is None else fr
    arr = lambda v: None if v is None else (ctypes.c_float * len(v))(*v)
    return N.lib().mh_decode_set_crops_norm_planes(
        ctypes.byref(fr) if fr is not False else None, geoms, total, crops, n, size[0], size[1], fmt, C, ps,
        arr(scale), arr(bias), luts, _stride(mh) if stride is None else stride, fstatus, cstatus, out, pitch, plane,
        cstride, None)


BOTH = pytest.mark.parametrize("call", [_crops, _planes], ids=["crops", "planes"])


def test_set_symbols_and_record_layout(mh):
    from metalhuffman_amd import _native as N
    lib = ctypes.CDLL(mh.LIB_PATH)
    for name in ("mh_decode_set_crops", "mh_decode_set_crops_shape", "mh_decode_set_crops_norm_planes",
                 "mh_decode_set_crops_norm_planes_shape"):
        assert hasattr(lib, name), name
        assert name in mh.EXPORTS, name
    assert ctypes.sizeof(N.mh_frame_geom) == 16
    names = ["first_block", "width", "height", "reserved"]
    assert [f[0] for f in N.mh_frame_geom._fields_] == names
    assert [getattr(N.mh_frame_geom, f).offset for f in names] == [0, 4, 8, 12]
    assert all(f[1] is ctypes.c_uint32 for f in N.mh_frame_geom._fields_)
    # the argument lists are the parents' with (d_geoms, total_blocks) behind the frame
    L = N.lib()
    for parent in ("mh_decode_crops", "mh_decode_crops_norm_planes"):
        mine, theirs = getattr(L, parent.replace("mh_decode_", "mh_decode_set_")).argtypes, getattr(L, parent).argtypes
        assert list(mine) == [theirs[0], ctypes.c_void_p, ctypes.c_uint32] + list(theirs[1:])


@BOTH
def test_the_sets_own_checks(mh, call):
    """NULL d_geoms and total_blocks == 0 where a NULL d_crops is reported; a misaligned d_geoms where
    a misaligned d_crops is."""
    from metalhuffman_amd import _native as N
    assert call(mh, geoms=None) == INVALID
    assert call(mh, total=0) == INVALID
    assert call(mh, crops=None) == INVALID and call(mh, n=0) == INVALID
    for off in (4, 8, 12):
        assert call(mh, geoms=GEOMS + off) == ALIGN, off
    assert call(mh, crops=CROPS + 8) == ALIGN
    assert call(mh, _short(), total=1) == CAPACITY                      # (any non-zero count passes the host)
    assert call(mh, _short(), total=0xFFFFFFFF) == CAPACITY
    # order: invalid before dims before alignment before capacity
    bad_dims = _frame(dims=N.mh_dims(0, 1531, 0, 0))
    assert call(mh, bad_dims, geoms=None) == INVALID
    assert call(mh, bad_dims, total=0, geoms=GEOMS + 8) == INVALID
    assert call(mh, bad_dims, geoms=GEOMS + 8) == DIMS
    assert call(mh, geoms=None, size=(2046, 1)) == INVALID
    assert call(mh, geoms=GEOMS + 8, size=(2046, 1)) == DIMS
    assert call(mh, _short(), geoms=GEOMS + 8) == ALIGN
    assert call(mh, geoms=GEOMS + 8, pitch=8) == ALIGN                  # a misaligned record array AND a small pitch
    # ... and ahead of them all, the aliasing refusal
    assert call(mh, fstatus=FSTATUS, cstatus=FSTATUS, geoms=GEOMS + 8, size=(0, 0)) == INVALID


@BOTH
def test_dims_are_the_sets_maxima(mh, call):
    """block_width / block_height are ignored; width and height bound the crop size."""
    from metalhuffman_amd import _native as N
    for bw, bh in ((0, 0), (256, 192), (1, 0xFFFFFFFF), (0xFFFFFFFF, 7)):
        assert call(mh, _short(dims=N.mh_dims(2045, 1531, bw, bh))) == CAPACITY, (bw, bh)
    for w, h in ((0, 1531), (2045, 0), (65536, 1531), (2045, 65536), (0xFFFFFFFF, 1), (0xFFFFFFF9, 8)):
        assert call(mh, _short(dims=N.mh_dims(w, h, 0, 0))) == DIMS, (w, h)
    assert call(mh, _short(dims=N.mh_dims(65535, 65535, 0, 0))) == CAPACITY
    for size in ((0, 1), (1, 0), (2046, 1), (1, 1532), (0xFFFFFFFF, 1), (1, 0xFFFFFFFF)):
        assert call(mh, size=size) == DIMS, size
    kw = dict(pitch=2044) if call is _crops else dict(pitch=4088)
    for size in ((2045, 1531), (1, 1), (2045, 1), (1, 1531)):            # up to the maxima: past the dims check
        assert call(mh, _short(), size=size, **kw) == ALIGN, size


@pytest.mark.parametrize("kw,status", [
    (dict(d_codes=None), INVALID),
    (dict(d_block_offsets=None), INVALID),
    (dict(n_frames=0), INVALID),
    (dict(d_frame_code_offsets=None), INVALID),                # a batch without frame offsets
    (dict(flags=0x2), INVALID),                                # MH_FLAG_LANE_PAIRS
    (dict(flags=0x8), INVALID),
    (dict(d_codes=0x20004), ALIGN),
    (dict(codes_bytes=2), CAPACITY),
    (dict(flags=0x1 | 0x4, codes_bytes=2), CAPACITY),          # NO_DELTA | ANY_ORDER pass
    (dict(table2_entries=100, codes_bytes=2), CAPACITY),       # the table fields are ignored
    (dict(d_lut=0x70004, codes_bytes=2), CAPACITY),
    (dict(n_frames=1, d_frame_code_offsets=None, codes_bytes=2), CAPACITY),   # a set of one frame
])
@BOTH
def test_the_parents_frame_checks_still_fire(mh, call, kw, status):
    one = dict(ps=0) if call is _planes and kw.get("n_frames") == 1 else {}   # three planes of the one frame
    assert call(mh, _frame(**kw), **one) == status


def test_crops_parent_argument_checks_still_fire(mh):
    st = _stride(mh)
    assert _crops(mh, False) == INVALID
    assert _crops(mh, out=None) == INVALID and _crops(mh, luts=None) == INVALID
    assert _crops(mh, fstatus=FSTATUS, cstatus=FSTATUS) == INVALID
    assert _crops(mh, _short(), fstatus=FSTATUS, cstatus=CSTATUS) == CAPACITY
    assert _crops(mh, pitch=PITCH + 4) == ALIGN and _crops(mh, pitch=CW) == ALIGN
    assert _crops(mh, out=OUT + 4) == ALIGN and _crops(mh, cstride=CSTRIDE + 4) == ALIGN
    assert _crops(mh, crops=CROPS + 4) == ALIGN and _crops(mh, luts=LUTS + 8) == ALIGN
    assert _crops(mh, stride=st + 8) == ALIGN and _crops(mh, stride=8) == ALIGN
    assert _crops(mh, pitch=PITCH - 8) == CAPACITY and _crops(mh, pitch=(1 << 20) + 8) == CAPACITY
    assert _crops(mh, cstride=CSTRIDE - 8) == CAPACITY and _crops(mh, cstride=0) == CAPACITY
    assert _crops(mh, stride=st - 16) == CAPACITY and _crops(mh, stride=16) == CAPACITY
    assert _crops(mh, size=(CW, 3), cstride=PITCH * 2) == CAPACITY
    # order
    assert _crops(mh, _frame(flags=0x8), size=(2046, 1)) == INVALID
    assert _crops(mh, size=(2046, 24), crops=CROPS + 8, luts=LUTS + 8, stride=st - 16, pitch=252) == DIMS
    assert _crops(mh, crops=CROPS + 8, stride=st - 16, pitch=PITCH - 8) == ALIGN
    assert _crops(mh, _short(), stride=st - 16, pitch=PITCH - 8) == CAPACITY
    # the tile cap counts the crops: 131 tiles per 65535 x 1 crop
    from metalhuffman_amd import _native as N
    big = _frame(dims=N.mh_dims(65535, 65535, 0, 0))
    assert _crops(mh, big, n=(2 ** 31 - 1) // 131 + 1, size=(65535, 1), pitch=65536, cstride=65536) == CAPACITY


def test_planes_parent_argument_checks_still_fire(mh):
    st = _stride(mh)
    inf = float("inf")
    assert _planes(mh, False) == INVALID
    assert _planes(mh, C=0) == INVALID and _planes(mh, C=5) == INVALID
    assert _planes(mh, scale=None) == INVALID and _planes(mh, bias=None) == INVALID
    assert _planes(mh, scale=(1.0, inf, 1.0, 1.0)) == INVALID
    assert _planes(mh, _short(), scale=(1.0, 1.0, 1.0, inf)) == CAPACITY          # index >= n_planes is not read
    assert _planes(mh, fmt=3) == INVALID
    assert _planes(mh, fstatus=FSTATUS, cstatus=FSTATUS) == INVALID
    assert _planes(mh, ps=2) == DIMS                                              # (3 - 1) * 2 >= 4 frames
    assert _planes(mh, _short(), ps=0) == CAPACITY
    assert _planes(mh, C=0, size=(0, 0)) == INVALID and _planes(mh, size=(0, 1), ps=2) == DIMS
    assert _planes(mh, pitch=NPITCH + 8) == ALIGN and _planes(mh, plane=NPLANE + 8) == ALIGN
    assert _planes(mh, out=OUT + 8) == ALIGN and _planes(mh, cstride=NSTRIDE + 8) == ALIGN
    assert _planes(mh, pitch=NPITCH - 16) == CAPACITY                             # < round_up(w, 8) * 2
    assert _planes(mh, plane=NPLANE - 16) == CAPACITY                             # planes overlap
    assert _planes(mh, cstride=NSTRIDE - 16) == CAPACITY                          # slots overlap
    assert _planes(mh, stride=st - 16) == CAPACITY
    # one plane: the strides are ignored, the call is the normalised crops'
    assert _planes(mh, _short(), C=1, ps=99, plane=4, cstride=NPLANE) == CAPACITY
    assert _planes(mh, C=1, ps=99, plane=4, cstride=NPLANE - 16) == CAPACITY


def test_accepted_calls_reach_the_device(mh):
    """Without a HIP device a call that passes every check ends in MH_ERR_HIP (the first HIP call finds
    no device); with one, the fake pointers must not be launched on (tests/test_gpu_set_crops*.py make
    such calls with real buffers)."""
    from metalhuffman_amd import _native as N
    if N.lib().mh_device_count() > 0:
        return
    assert _crops(mh) == HIP and _planes(mh) == HIP
    assert _crops(mh, stride=0) == HIP and _planes(mh, stride=0, ps=0) == HIP
    assert _crops(mh, total=1, fstatus=FSTATUS, cstatus=CSTATUS) == HIP
    assert _crops(mh, size=(2045, 1531), pitch=2048, cstride=2048 * 1531) == HIP
    assert _planes(mh, C=1, plane=0, cstride=NPLANE) == HIP
    assert _crops(mh, _frame(n_frames=1, d_frame_code_offsets=None)) == HIP


def test_shape_twins(mh):
    from metalhuffman_amd import _native as N
    L = N.lib()
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    G, Wv = ctypes.byref(g), ctypes.byref(w)
    ok = lambda **kw: ctypes.byref(_frame(**kw))
    crops = lambda fr, n=4, size=(CW, CH), gp=G, wp=Wv: L.mh_decode_set_crops_shape(fr, n, size[0], size[1], None, gp, wp)
    planes = lambda fr, n=4, size=(CW, CH), fmt=F16, C=3, gp=G, wp=Wv: L.mh_decode_set_crops_norm_planes_shape(
        fr, n, size[0], size[1], fmt, C, None, gp, wp)
    for f in (crops, planes):
        assert f(None) == INVALID
        assert f(ok(), gp=None) == INVALID and f(ok(), wp=None) == INVALID
        assert f(ok(), n=0) == INVALID
        assert f(ok(n_frames=0)) == INVALID
        assert f(ok(flags=0x2)) == INVALID
        assert f(ok(dims=N.mh_dims(0, 16, 0, 0))) == DIMS
        assert f(ok(dims=N.mh_dims(16, 65536, 2, 8192))) == DIMS
        for size in ((0, 8), (8, 0), (2046, 8), (8, 1532), (0xFFFFFFFF, 1)):
            assert f(ok(), size=size) == DIMS, size
        # the block counts are ignored here too: an accepted description reaches the device query
        if L.mh_device_count() == 0:
            assert f(ok(dims=N.mh_dims(16, 16, 3, 2)), size=(1, 1)) == HIP
            assert f(ok()) == HIP
    assert planes(ok(), fmt=3) == INVALID
    assert planes(ok(), C=0) == INVALID and planes(ok(), C=5) == INVALID
    big = ok(dims=N.mh_dims(65535, 65535, 0, 0))
    assert crops(big, n=(2 ** 31 - 1) // (131 * 8193) + 1, size=(65535, 65535)) == CAPACITY
