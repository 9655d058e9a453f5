"""The C-ABI of the scaled region entries (include/metalhuffman.h: mh_decode_region_scaled,
mh_decode_region_scaled_shape, mh_box_reduce): exported, and every argument check made before any
HIP call, with fake pointers -- mh_decode_region's checks in its order, SW / SH in the place of
RW / RH and c = 8 >> log2_scale in the place of 8 in the alignment rules. CPU only."""
from __future__ import annotations

import ctypes

import pytest

INVALID, DIMS, CAPACITY, TABLE, ALIGN, HIP = -1, -2, -4, -5, -6, -7
LUTS, OUT = 0x60000, 0x50000
KS = (1, 2, 3)


def _frame(**kw):
    """A frame the entry accepts: 2048 x 1536, the table fields NULL / 0 (ignored)."""
    from metalhuffman_amd import _native as N
    fr = N.mh_frame()
    fr.d_block_offsets = 0x10000
    fr.d_codes = 0x20000
    fr.codes_bytes = 4096
    fr.dims = N.mh_dims(2048, 1536, 256, 192)
    fr.n_frames = 1
    for k, v in kw.items():
        setattr(fr, k, v)
    return fr


def _stride(mh):
    return (int(mh.lib().mh_lut_bytes()) + 15) // 16 * 16


def _region(*v):
    from metalhuffman_amd import _native as N
    return ctypes.byref(N.mh_region(*v))


def _call(mh, k, fr=None, rg=(16, 8, 32, 24), luts=LUTS, stride=None, out=OUT, pitch=None, fstride=0):
    """mh_decode_region_scaled with defaults that pass every check (the region is 256 x 192 pixels:
    SW = 256 >> k, the default pitch); callers that must not reach a launch pass codes_bytes=2."""
    from metalhuffman_amd import _native as N
    fr = _frame() if fr is None else fr
    return N.lib().mh_decode_region_scaled(ctypes.byref(fr) if fr is not False else None,
                                           _region(*rg) if rg is not None else None, k, luts,
                                           _stride(mh) if stride is None else stride, None, out,
                                           (256 >> k) if pitch is None else pitch, fstride, None)


SHORT = dict(codes_bytes=2)   # fails the LAST-but-one capacity rule: every earlier check was passed


def _short(**kw):
    return _frame(**dict(SHORT, **kw))


def test_scaled_symbols_exported(mh):
    lib = ctypes.CDLL(mh.LIB_PATH)
    for name in ("mh_decode_region_scaled", "mh_decode_region_scaled_shape", "mh_box_reduce"):
        assert hasattr(lib, name), name
        assert name in mh.EXPORTS, name


@pytest.mark.parametrize("k", (0,) + KS)
@pytest.mark.parametrize("kw,status", [
    (dict(d_codes=None), INVALID),
    (dict(d_block_offsets=None), INVALID),
    (dict(n_frames=0), INVALID),
    (dict(n_frames=2), INVALID),                               # batch without frame offsets
    (dict(flags=0x2), INVALID),                                # MH_FLAG_LANE_PAIRS: refused here
    (dict(flags=0x8), INVALID),
    (dict(d_codes=0x20004), ALIGN),
    (dict(codes_bytes=2), CAPACITY),
    (dict(flags=0x1 | 0x4, codes_bytes=2), CAPACITY),          # NO_DELTA | ANY_ORDER pass the flag check
    (dict(table2_entries=100, codes_bytes=2), CAPACITY),       # the table fields are ignored ...
    (dict(d_lut=0x70004, codes_bytes=2), CAPACITY),            # ... a misaligned d_lut included
])
def test_scaled_rejects_bad_frames(mh, k, kw, status):
    """The region entry's frame cases, code for code, at every scale (0 forwards)."""
    assert _call(mh, k, _frame(**kw)) == status


@pytest.mark.parametrize("k", KS)
def test_scaled_rejects_bad_arguments(mh, k):
    """Every code of the region entry at its place, SW / SH for RW / RH and c for 8."""
    from metalhuffman_amd import _native as N
    st, c, s = _stride(mh), 8 >> k, 1 << k
    sw, sh = 256 >> k, 192 >> k
    assert _call(mh, k, False) == INVALID                                   # NULL frame
    assert _call(mh, k, rg=None) == INVALID                                 # NULL region
    assert _call(mh, k, out=None) == INVALID
    assert _call(mh, k, luts=None) == INVALID
    assert _call(mh, k, _short(dims=N.mh_dims(2048, 1536, 255, 192))) == DIMS
    for rg in ((0, 0, 0, 1), (0, 0, 1, 0), (0, 0, 257, 1), (1, 0, 256, 1), (0, 0, 1, 193), (0, 192, 1, 1),
               (256, 0, 1, 1), (0xFFFFFFFF, 0, 2, 1), (0, 0xFFFFFFFF, 1, 2), (0xFFFFFFFF, 0, 0xFFFFFFFF, 1),
               (2, 0, 0xFFFFFFFF, 1)):
        assert _call(mh, k, rg=rg) == DIMS, rg
    # alignment to c: d_out, the pitch and (n_frames > 1) the frame stride
    two = lambda **kw: _frame(n_frames=2, d_frame_code_offsets=0x80000, **kw)
    if c > 1:
        assert _call(mh, k, pitch=sw + c // 2) == ALIGN
        assert _call(mh, k, out=OUT + c // 2) == ALIGN
        assert _call(mh, k, two(), fstride=sw * sh + c // 2) == ALIGN
    # ... and to no more than c: multiples of c that are not multiples of 2 c get past the alignment rule
    assert _call(mh, k, _short(), out=OUT + c, pitch=sw + c) == CAPACITY
    assert _call(mh, k, two(**SHORT), out=OUT + c, pitch=sw + c, fstride=(sw + c) * sh + c) == CAPACITY
    assert _call(mh, k, luts=LUTS + 8) == ALIGN                             # d_luts % 16
    assert _call(mh, k, stride=st + 8) == ALIGN                             # stride % 16
    assert _call(mh, k, stride=8) == ALIGN
    assert _call(mh, k, stride=st - 16) == CAPACITY                         # 0 < stride < mh_lut_bytes()
    assert _call(mh, k, stride=16) == CAPACITY
    # pitch: SW stands where RW does
    assert _call(mh, k, pitch=sw - c) == CAPACITY                           # an aligned pitch < SW
    assert _call(mh, k, pitch=(1 << 20) + 8) == CAPACITY
    # the right-edge region of a 2045-wide frame: RW = 253, SW = ceil(253 / s); out_pitch = SW - 1 is too small
    edge = lambda **kw: _frame(dims=N.mh_dims(2045, 1531, 256, 192), **kw)
    esw, esh = -(-253 // s), -(-187 // s)
    bad = esw - 1
    if bad % c == 0:                                                         # (k = 3; else SW - 1 is misaligned)
        assert _call(mh, k, edge(), rg=(224, 168, 32, 24), pitch=bad) == CAPACITY
    else:
        assert _call(mh, k, edge(), rg=(224, 168, 32, 24), pitch=bad) == ALIGN
        assert _call(mh, k, edge(), rg=(224, 168, 32, 24), pitch=bad // c * c) == CAPACITY
    # stride: out_pitch * SH - c overlaps
    assert _call(mh, k, two(), fstride=sw * sh - c) == CAPACITY
    e2 = edge(n_frames=2, d_frame_code_offsets=0x80000)
    assert _call(mh, k, e2, rg=(224, 168, 32, 24), pitch=32 * c, fstride=32 * c * esh - c) == CAPACITY
    assert _call(mh, k, edge(n_frames=2, d_frame_code_offsets=0x80000, **SHORT), rg=(224, 168, 32, 24), pitch=32 * c,
                 fstride=32 * c * esh) == CAPACITY                          # (passes the stride rule: stopped by SHORT)


def test_scaled_out_pitch_sw_minus_one(mh):
    """out_pitch = SW - 1 -> MH_ERR_CAPACITY where the alignment rule lets it through: k = 3 (any
    pitch is legal), and k = 1, 2 on a region whose SW - 1 is a multiple of c."""
    from metalhuffman_amd import _native as N
    assert _call(mh, 3, pitch=31) == CAPACITY                               # SW = 32
    # a region whose SW - 1 is no multiple of c stops at the alignment rule first: RW = 61, SW = 31, c = 4
    fr = lambda: _frame(dims=N.mh_dims(2045, 1531, 256, 192))
    assert _call(mh, 1, fr(), rg=(248, 0, 8, 1), pitch=30) == ALIGN
    # SW - 1 is a multiple of c when SW = 1: the last block of a 2041-wide frame, RW = 1
    one = lambda: _frame(dims=N.mh_dims(2041, 1531, 256, 192))
    for k in (1, 2):
        assert _call(mh, k, one(), rg=(255, 0, 1, 1), pitch=0) == CAPACITY  # SW = 1: SW - 1 = 0 is aligned
        assert _call(mh, k, _frame(**SHORT, dims=N.mh_dims(2041, 1531, 256, 192)), rg=(255, 0, 1, 1),
                     pitch=8 >> k) == CAPACITY                               # pitch c >= SW passes: stopped by SHORT


def test_scaled_bad_scale(mh):
    """log2_scale > 3 -> MH_ERR_INVALID_ARG, reported where a bad flag is: behind the NULL checks,
    ahead of the dims."""
    from metalhuffman_amd import _native as N
    for k in (4, 5, 8, 0xFFFFFFFF):
        assert _call(mh, k) == INVALID
        assert _call(mh, k, _frame(dims=N.mh_dims(2048, 1536, 255, 192))) == INVALID      # before dims
        assert _call(mh, k, rg=(250, 0, 32, 24), luts=LUTS + 8, pitch=3) == INVALID
    with pytest.raises(ValueError):
        from metalhuffman_amd.decoder import Region
        Region(0, 0, 1, 1).scaled_size(8, 8, 4)


def test_scaled_check_order(mh):
    """invalid argument, dims, alignment, capacity -- the region entry's order."""
    from metalhuffman_amd import _native as N
    st = _stride(mh)
    for k in KS:
        c, sw = 8 >> k, 256 >> k
        bad_dims = _frame(dims=N.mh_dims(2048, 1536, 255, 192))
        assert _call(mh, k, bad_dims, luts=LUTS + 8, stride=st - 16, pitch=sw - c) == DIMS
        assert _call(mh, k, rg=(250, 0, 32, 24), luts=LUTS + 8, stride=st - 16, pitch=sw - c) == DIMS
        assert _call(mh, k, luts=LUTS + 8, stride=st - 16, pitch=sw - c) == ALIGN
        assert _call(mh, k, stride=8, pitch=sw - c) == ALIGN
        assert _call(mh, k, _frame(flags=0x8), rg=(250, 0, 32, 24)) == INVALID
        assert _call(mh, k, _short(), stride=st - 16, pitch=sw - c) == CAPACITY


def test_scaled_k3_any_pitch(mh):
    """k = 3: c = 1, so an odd d_out, pitch and stride pass the alignment rule (the call is then
    stopped by the short code buffer, a later rule; without a device an accepted call ends in
    MH_ERR_HIP)."""
    from metalhuffman_amd import _native as N
    assert _call(mh, 3, _short(), out=OUT + 1, pitch=33) == CAPACITY
    two = _frame(n_frames=2, d_frame_code_offsets=0x80000, **SHORT)
    assert _call(mh, 3, two, out=OUT + 3, pitch=33, fstride=33 * 24 + 1) == CAPACITY
    assert _call(mh, 3, _short(), pitch=31) == CAPACITY                      # ... but not a pitch < SW = 32
    if N.lib().mh_device_count() == 0:
        assert _call(mh, 3, out=OUT + 1, pitch=33) == HIP
        for k in KS:
            assert _call(mh, k) == HIP and _call(mh, k, stride=0) == HIP


def test_scaled_shape_rejects_bad_arguments(mh):
    from metalhuffman_amd import _native as N
    L = N.lib()
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    G, Wv = ctypes.byref(g), ctypes.byref(w)
    ok, rg = lambda **kw: ctypes.byref(_frame(**kw)), _region(0, 0, 8, 8)
    f = L.mh_decode_region_scaled_shape
    for k in (0,) + KS:
        assert f(None, rg, k, None, G, Wv) == INVALID
        assert f(ok(), None, k, None, G, Wv) == INVALID
        assert f(ok(), rg, k, None, None, Wv) == INVALID
        assert f(ok(), rg, k, None, G, None) == INVALID
        assert f(ok(n_frames=0), rg, k, None, G, Wv) == INVALID
        assert f(ok(flags=0x2), rg, k, None, G, Wv) == INVALID
        assert f(ok(dims=N.mh_dims(16, 16, 3, 2)), rg, k, None, G, Wv) == DIMS
        assert f(ok(), _region(250, 0, 8, 8), k, None, G, Wv) == DIMS
        assert f(ok(), _region(0, 0, 0, 8), k, None, G, Wv) == DIMS
        if L.mh_device_count() == 0:
            assert f(ok(), rg, k, None, G, Wv) == HIP
    assert f(ok(), rg, 4, None, G, Wv) == INVALID
    assert f(ok(dims=N.mh_dims(16, 16, 3, 2)), rg, 4, None, G, Wv) == INVALID     # before dims
    big = _frame(dims=N.mh_dims(65535, 65535, 8192, 8192), n_frames=2048, d_frame_code_offsets=0x80000)
    assert f(ctypes.byref(big), _region(0, 0, 8192, 8192), 2, None, G, Wv) == CAPACITY


def test_scaled_size():
    from metalhuffman_amd.decoder import Region
    W, H = 597, 67
    full = Region(0, 0, 75, 9)
    assert [full.scaled_size(W, H, k) for k in range(4)] == [(597, 67), (299, 34), (150, 17), (75, 9)]
    assert Region(11, 0, 64, 9).scaled_size(W, H, 2) == (128, 17)      # RW = 509
    assert Region(0, 4, 10, 5).scaled_size(W, H, 3) == (10, 5)         # RH = 35
    assert Region(74, 8, 1, 1).scaled_size(W, H, 1) == (3, 2)          # the 5 x 3 corner block
    assert Region(74, 8, 1, 1).scaled_size(W, H, 3) == (1, 1)
