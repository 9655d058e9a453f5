"""The C-ABI of mh_decode_set_frames and mh_decode_set_frames_shape (include/metalhuffman.h): exported,
the two records' layouts as ctypes sees them, and every host check made before any HIP call, with fake
pointers -- the set crops' checks in the set crops' order (tests/test_set_crops_abi.py), the records
and the group map where the descriptors are, and no pitch or stride to judge. CPU only."""
from __future__ import annotations

import ctypes

import pytest

INVALID, DIMS, CAPACITY, ALIGN, HIP = -1, -2, -4, -6, -7
LUTS, OUT, FSTATUS, SSTATUS, GEOMS, RASTERS, SHARES, MAP = (0x60000, 0x50000, 0xA0000, 0xB0000, 0xC0000, 0xD0000,
                                                            0xE0000, 0xF0000)


def _frame(**kw):
    """A set the entry accepts: maxima 2045 x 1531, four frames; the block counts are deliberately not
    those of the maxima (they are ignored), and the table fields are NULL / 0."""
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


def _call(mh, fr=None, geoms=GEOMS, total=1000, rasters=RASTERS, shares=SHARES, gmap=MAP, n_groups=16, luts=LUTS,
          stride=None, fstatus=None, sstatus=None, out=OUT, out_bytes=1 << 20):
    from metalhuffman_amd import _native as N
    fr = _frame() if fr is None else fr
    return N.lib().mh_decode_set_frames(ctypes.byref(fr) if fr is not False else None, geoms, total, rasters, shares,
                                        gmap, n_groups, luts, _stride(mh) if stride is None else stride, fstatus,
                                        sstatus, out, out_bytes, None)


def test_symbols_and_record_layouts(mh):
    from metalhuffman_amd import _native as N
    lib = ctypes.CDLL(mh.LIB_PATH)
    for name in ("mh_decode_set_frames", "mh_decode_set_frames_shape", "mh_decode_set_plan"):
        assert hasattr(lib, name), name
        assert name in mh.EXPORTS, name
    for rec in (N.mh_set_raster, N.mh_set_share, N.mh_frame_geom):
        assert ctypes.sizeof(rec) == 16, rec
    assert ctypes.alignment(N.mh_set_raster) == 8 and ctypes.alignment(N.mh_set_share) == 4
    assert [f[0] for f in N.mh_set_raster._fields_] == ["offset", "pitch", "reserved"]
    assert [getattr(N.mh_set_raster, f).offset for f in ("offset", "pitch", "reserved")] == [0, 8, 12]
    assert [getattr(N.mh_set_raster, f).size for f in ("offset", "pitch", "reserved")] == [8, 4, 4]
    assert [f[0] for f in N.mh_set_share._fields_] == ["first_group", "groups", "reserved"]
    assert [getattr(N.mh_set_share, f).offset for f in ("first_group", "groups", "reserved")] == [0, 4, 8]
    assert N.mh_set_share.reserved.size == 8
    assert N.MH_DECODE_GROUP_WAVES == 8
    # the header says the same
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "metalhuffman.h")).read()
    assert "} mh_set_raster;" in hdr and "} mh_set_share;" in hdr and "#define MH_DECODE_GROUP_WAVES 8" in hdr
    assert "Not covered: a set for the region, window and scaled entries" in hdr


def test_null_and_zero_arguments(mh):
    assert _call(mh, False) == INVALID
    for kw in (dict(geoms=None), dict(rasters=None), dict(shares=None), dict(gmap=None), dict(out=None),
               dict(luts=None), dict(total=0), dict(n_groups=0), dict(out_bytes=0)):
        assert _call(mh, **kw) == INVALID, kw
    assert _call(mh, n_groups=0x80000000) == INVALID and _call(mh, n_groups=0xFFFFFFFF) == INVALID
    assert _call(mh, _short(), n_groups=0x7FFFFFFF) == CAPACITY              # the grid limit itself passes
    assert _call(mh, fstatus=FSTATUS, sstatus=FSTATUS) == INVALID           # the status arrays must not alias
    assert _call(mh, _short(), fstatus=FSTATUS, sstatus=SSTATUS) == CAPACITY
    assert _call(mh, _short(), total=1, out_bytes=1) == CAPACITY            # (any non-zero value passes the host)
    assert _call(mh, _short(), total=0xFFFFFFFF, out_bytes=2 ** 64 - 1) == CAPACITY


def test_alignment(mh):
    for name in ("geoms", "rasters", "shares"):
        for off in (4, 8, 12):
            assert _call(mh, **{name: 0xC0000 + off}) == ALIGN, (name, off)
    for off in (1, 2, 3):
        assert _call(mh, gmap=MAP + off) == ALIGN, off
    assert _call(mh, _short(), gmap=MAP + 4) == CAPACITY                     # 4-byte aligned is enough
    for off in (1, 4, 7):
        assert _call(mh, out=OUT + off) == ALIGN, off
    assert _call(mh, _short(), out=OUT + 8) == CAPACITY
    st = _stride(mh)
    assert _call(mh, luts=LUTS + 8) == ALIGN and _call(mh, stride=st + 8) == ALIGN and _call(mh, stride=8) == ALIGN
    assert _call(mh, stride=st - 16) == CAPACITY and _call(mh, stride=16) == CAPACITY
    assert _call(mh, _short(), stride=0) == CAPACITY                          # one shared table: past the stride rule


def test_order_of_the_checks(mh):
    from metalhuffman_amd import _native as N
    bad_dims = _frame(dims=N.mh_dims(0, 1531, 0, 0))
    assert _call(mh, bad_dims, rasters=None) == INVALID
    assert _call(mh, bad_dims, n_groups=0, shares=SHARES + 8) == INVALID
    assert _call(mh, bad_dims, shares=SHARES + 8) == DIMS
    assert _call(mh, _frame(flags=0x8), shares=SHARES + 8) == INVALID
    assert _call(mh, _short(), shares=SHARES + 8) == ALIGN
    assert _call(mh, _short(), gmap=MAP + 2, stride=16) == ALIGN
    assert _call(mh, fstatus=FSTATUS, sstatus=FSTATUS, geoms=GEOMS + 8, n_groups=0) == INVALID


def test_dims_are_the_sets_maxima(mh):
    from metalhuffman_amd import _native as N
    for bw, bh in ((0, 0), (256, 192), (1, 0xFFFFFFFF)):
        assert _call(mh, _short(dims=N.mh_dims(2045, 1531, bw, bh))) == CAPACITY, (bw, bh)
    for w, h in ((0, 1531), (2045, 0), (65536, 1531), (2045, 65536), (0xFFFFFFFF, 1)):
        assert _call(mh, _short(dims=N.mh_dims(w, h, 0, 0))) == DIMS, (w, h)
    assert _call(mh, _short(dims=N.mh_dims(65535, 65535, 0, 0))) == CAPACITY


@pytest.mark.parametrize("kw,status", [
    (dict(d_codes=None), INVALID),
    (dict(d_block_offsets=None), INVALID),
    (dict(n_frames=0), INVALID),
    (dict(d_frame_code_offsets=None), INVALID),                # a set of four without frame offsets
    (dict(flags=0x2), INVALID),                                # MH_FLAG_LANE_PAIRS
    (dict(flags=0x8), INVALID),
    (dict(d_codes=0x20004), ALIGN),
    (dict(codes_bytes=2), CAPACITY),
    (dict(flags=0x1 | 0x4, codes_bytes=2), CAPACITY),          # NO_DELTA | ANY_ORDER pass
    (dict(table2_entries=100, codes_bytes=2), CAPACITY),       # the table fields are ignored
    (dict(n_frames=1, d_frame_code_offsets=None, codes_bytes=2), CAPACITY),   # a set of one frame
])
def test_the_frame_checks_fire(mh, kw, status):
    assert _call(mh, _frame(**kw)) == status


def test_accepted_calls_reach_the_device(mh):
    """Without a HIP device a call that passes every check ends in MH_ERR_HIP; with one, the fake
    pointers must not be launched on (tests/test_gpu_decode_set_frames.py makes such calls)."""
    from metalhuffman_amd import _native as N
    if N.lib().mh_device_count() > 0:
        return
    assert _call(mh) == HIP and _call(mh, stride=0) == HIP
    assert _call(mh, n_groups=1, total=1, out_bytes=8, fstatus=FSTATUS, sstatus=SSTATUS) == HIP
    assert _call(mh, _frame(n_frames=1, d_frame_code_offsets=None)) == HIP


def test_shape_entry(mh):
    from metalhuffman_amd import _native as N
    L = N.lib()
    r, w = ctypes.c_uint32(), ctypes.c_uint32()
    R, W = ctypes.byref(r), ctypes.byref(w)
    assert L.mh_decode_set_frames_shape(None, None, R, W) == INVALID
    assert L.mh_decode_set_frames_shape(ctypes.byref(_frame()), None, None, W) == INVALID
    assert L.mh_decode_set_frames_shape(ctypes.byref(_frame()), None, R, None) == INVALID
    assert L.mh_decode_set_frames_shape(ctypes.byref(_frame(flags=0x2)), None, R, W) == INVALID
    if L.mh_device_count() == 0:
        assert L.mh_decode_set_frames_shape(ctypes.byref(_frame()), None, R, W) == HIP
        assert L.mh_decode_set_frames_shape(ctypes.byref(_frame(flags=0x1)), None, R, W) == HIP
