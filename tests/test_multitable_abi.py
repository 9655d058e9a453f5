"""The C-ABI of the per-frame-table batch entries (include/metalhuffman.h:
mh_build_luts_device, mh_decode_frames, mh_decode_frames_shape): exported, and every
argument check made before any HIP call, with fake pointers. CPU only."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

INVALID, DIMS, CAPACITY, TABLE, ALIGN = -1, -2, -4, -5, -6
LUTS, OUT = 0x60000, 0x50000


def _frame(**kw):
    """A frame mh_decode_frames accepts: the table fields stay NULL / 0 (ignored)."""
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


def test_new_symbols_exported(mh):
    lib = ctypes.CDLL(mh.LIB_PATH)
    for name in ("mh_build_luts_device", "mh_decode_frames", "mh_decode_frames_shape"):
        assert hasattr(lib, name), name
        assert name in mh.EXPORTS, name


@pytest.mark.parametrize("kw,status", [
    (dict(d_codes=None), INVALID),
    (dict(d_block_offsets=None), INVALID),
    (dict(n_frames=0), INVALID),
    (dict(n_frames=2), INVALID),                               # batch without frame offsets
    (dict(flags=0x2), INVALID),                                # MH_FLAG_LANE_PAIRS: refused here
    (dict(flags=0x8), INVALID),                                # first unassigned flag bit
    (dict(flags=0x80), INVALID),
    (dict(d_codes=0x20004), ALIGN),                            # not 16-byte aligned
    (dict(codes_bytes=2), CAPACITY),
    (dict(flags=0x1 | 0x4, codes_bytes=2), CAPACITY),          # NO_DELTA | ANY_ORDER pass the flag check
    (dict(table2_entries=100, codes_bytes=2), CAPACITY),       # the table fields are ignored ...
    (dict(d_lut=0x70004, codes_bytes=2), CAPACITY),            # ... a misaligned d_lut included
])
def test_decode_frames_rejects_bad_frames(mh, kw, status):
    from metalhuffman_amd import _native as N
    fr = _frame(**kw)
    assert N.lib().mh_decode_frames(ctypes.byref(fr), LUTS, _stride(mh), None, OUT, 2048, 0, None) == status


def test_decode_frames_rejects_bad_arguments(mh):
    """mh_decode's order and codes, the table rules in the place of the frame's table fields."""
    from metalhuffman_amd import _native as N
    L, st = N.lib(), _stride(mh)
    ok = lambda: ctypes.byref(_frame())
    assert L.mh_decode_frames(None, LUTS, st, None, OUT, 2048, 0, None) == INVALID
    assert L.mh_decode_frames(ok(), LUTS, st, None, None, 2048, 0, None) == INVALID          # no output
    assert L.mh_decode_frames(ok(), None, st, None, OUT, 2048, 0, None) == INVALID           # NULL d_luts
    bad_dims = ctypes.byref(_frame(dims=N.mh_dims(2048, 1536, 255, 192)))
    assert L.mh_decode_frames(bad_dims, LUTS, st, None, OUT, 2048, 0, None) == DIMS
    assert L.mh_decode_frames(ctypes.byref(_frame(dims=N.mh_dims(70000, 8, 8750, 1))), LUTS, st, None, OUT, 70000,
                              0, None) == DIMS
    assert L.mh_decode_frames(ok(), LUTS, st, None, OUT, 2044, 0, None) == ALIGN             # pitch % 8
    assert L.mh_decode_frames(ok(), LUTS, st, None, OUT + 4, 2048, 0, None) == ALIGN         # d_out % 8
    assert L.mh_decode_frames(ok(), LUTS + 8, st, None, OUT, 2048, 0, None) == ALIGN         # d_luts % 16
    assert L.mh_decode_frames(ok(), LUTS, st + 8, None, OUT, 2048, 0, None) == ALIGN         # stride % 16
    assert L.mh_decode_frames(ok(), LUTS, st - 16, None, OUT, 2048, 0, None) == CAPACITY     # stride < mh_lut_bytes()
    assert L.mh_decode_frames(ok(), LUTS, 0, None, OUT, 2048, 0, None) == CAPACITY
    assert L.mh_decode_frames(ok(), LUTS, st, None, OUT, 1024, 0, None) == CAPACITY          # pitch < width
    two = lambda: ctypes.byref(_frame(n_frames=2, d_frame_code_offsets=0x80000))
    assert L.mh_decode_frames(two(), LUTS, st, None, OUT, 2048, 2048 * 1536 + 4, None) == ALIGN   # frame stride % 8
    assert L.mh_decode_frames(two(), LUTS, st, None, OUT, 2048, 2048 * 1535, None) == CAPACITY    # frames overlap
    # dims are checked before alignment, alignment before capacity (mh_decode's order)
    assert L.mh_decode_frames(bad_dims, LUTS + 8, st - 16, None, OUT, 2044, 0, None) == DIMS
    assert L.mh_decode_frames(ok(), LUTS + 8, st - 16, None, OUT, 1024, 0, None) == ALIGN
    # n_frames == 1 with NULL d_frame_code_offsets is allowed: every check above passed it by


def test_decode_frames_shape_rejects_bad_arguments(mh):
    from metalhuffman_amd import _native as N
    L = N.lib()
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.mh_decode_frames_shape(None, None, ctypes.byref(g), ctypes.byref(w)) == INVALID
    assert L.mh_decode_frames_shape(ctypes.byref(_frame()), None, None, ctypes.byref(w)) == INVALID
    assert L.mh_decode_frames_shape(ctypes.byref(_frame()), None, ctypes.byref(g), None) == INVALID
    assert L.mh_decode_frames_shape(ctypes.byref(_frame(n_frames=0)), None, ctypes.byref(g), ctypes.byref(w)) == INVALID
    assert L.mh_decode_frames_shape(ctypes.byref(_frame(flags=0x2)), None, ctypes.byref(g), ctypes.byref(w)) == INVALID
    assert L.mh_decode_frames_shape(ctypes.byref(_frame(dims=N.mh_dims(16, 16, 3, 2))), None, ctypes.byref(g),
                                    ctypes.byref(w)) == DIMS


def test_build_luts_rejects_bad_arguments(mh):
    from metalhuffman_amd import _native as N
    L, st = N.lib(), _stride(mh)
    assert L.mh_build_luts_device(None, 4, LUTS, st, None, None) == INVALID
    assert L.mh_build_luts_device(0x10000, 4, None, st, None, None) == INVALID
    assert L.mh_build_luts_device(0x10000, 0, LUTS, st, None, None) == INVALID
    assert L.mh_build_luts_device(0x10000, 65536, LUTS, st, None, None) == INVALID
    assert L.mh_build_luts_device(0x10000, 4, LUTS + 4, st, None, None) == ALIGN
    assert L.mh_build_luts_device(0x10000, 4, LUTS, st + 4, None, None) == ALIGN
    assert L.mh_build_luts_device(0x10000, 4, LUTS, st - 16, None, None) == CAPACITY


def test_mh_decode_flag_set_unchanged(mh):
    """mh_decode keeps its flag set: 0x8 rejected, MH_FLAG_LANE_PAIRS accepted (and ignored), and
    it still wants the frame's own tables."""
    from metalhuffman_amd import _native as N
    L = N.lib()
    full = dict(d_table1=0x30000, d_table2=0x40000, table2_entries=256)
    assert L.mh_decode(ctypes.byref(_frame(flags=0x8, **full)), OUT, 2048, 0, None) == INVALID
    assert L.mh_decode(ctypes.byref(_frame(flags=0x2, codes_bytes=2, **full)), OUT, 2048, 0, None) == CAPACITY
    assert L.mh_decode(ctypes.byref(_frame()), OUT, 2048, 0, None) == INVALID                  # no T1 / T2
    assert L.mh_decode(ctypes.byref(_frame(**dict(full, table2_entries=100))), OUT, 2048, 0, None) == TABLE
    assert L.mh_decode(ctypes.byref(_frame(d_lut=0x70004, **full)), OUT, 2048, 0, None) == ALIGN


def test_pack_shared_table_default(mh):
    """DeviceFrames.pack still refuses mixed headers by default; the check runs before any
    device call. shared_table=False gets past it (and then needs a device: the GPU tests)."""
    from metalhuffman_amd import decoder as D
    a = mh.encode_frame(np.zeros((16, 16), np.uint8))
    b = mh.encode_frame((np.arange(256, dtype=np.uint8) * 7).reshape(16, 16))
    assert not np.array_equal(a.canon, b.canon)
    with pytest.raises(ValueError, match="a batch shares one canonical table"):
        D.DeviceFrames.pack([a, b], "cuda:0")
    with pytest.raises(ValueError, match="a batch shares one canonical table"):
        D.DeviceFrames.pack([a, b], "cuda:0", shared_table=True)
    c = mh.encode_frame(np.zeros((8, 16), np.uint8))
    with pytest.raises(ValueError, match="one size and one format"):
        D.DeviceFrames.pack([a, c], "cuda:0", shared_table=False)
