"""The C-ABI of the header-direct entries (include/metalhuffman.h: mh_decode_headers,
mh_decode_headers_shape, mh_header_luts_device, mh_stream_create_headers,
mh_stream_submit_header, mh_stream_slot_status): exported, and every argument check of the
decode and table entries made before any HIP call, with fake pointers. CPU only."""
from __future__ import annotations

import ctypes

import pytest

INVALID, DIMS, CAPACITY, TABLE, ALIGN = -1, -2, -4, -5, -6
HDRS, OUT, LUTS = 0x60001, 0x50000, 0x70000   # headers need no alignment
FST, HST = 0x90000, 0x91000

NEW = ("mh_decode_headers", "mh_header_luts_device", "mh_stream_create_headers", "mh_stream_submit_header",
       "mh_stream_slot_status", "mh_decode_headers_shape")


def _frame(**kw):
    """A frame mh_decode_headers accepts: the table fields stay NULL / 0 (ignored)."""
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
    for name in NEW:
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
def test_decode_headers_rejects_bad_frames(mh, kw, status):
    from metalhuffman_amd import _native as N
    fr = _frame(**kw)
    assert N.lib().mh_decode_headers(ctypes.byref(fr), HDRS, None, None, OUT, 2048, 0, None) == status
    assert N.lib().mh_decode_headers(ctypes.byref(fr), HDRS, FST, HST, OUT, 2048, 0, None) == status


def test_decode_headers_rejects_bad_arguments(mh):
    """mh_decode_frames' order and codes; NULL headers stand where the d_luts rules did."""
    from metalhuffman_amd import _native as N
    L = N.lib()
    ok = lambda: ctypes.byref(_frame())
    dh = L.mh_decode_headers
    assert dh(None, HDRS, None, None, OUT, 2048, 0, None) == INVALID
    assert dh(ok(), HDRS, None, None, None, 2048, 0, None) == INVALID          # no output
    assert dh(ok(), None, None, None, OUT, 2048, 0, None) == INVALID           # NULL headers
    assert dh(ok(), HDRS, FST, FST, OUT, 2048, 0, None) == INVALID             # aliased status arrays
    bad_dims = ctypes.byref(_frame(dims=N.mh_dims(2048, 1536, 255, 192)))
    assert dh(bad_dims, HDRS, None, None, OUT, 2048, 0, None) == DIMS
    assert dh(ctypes.byref(_frame(dims=N.mh_dims(70000, 8, 8750, 1))), HDRS, None, None, OUT, 70000, 0, None) == DIMS
    assert dh(ok(), HDRS, None, None, OUT, 2044, 0, None) == ALIGN             # pitch % 8
    assert dh(ok(), HDRS, None, None, OUT + 4, 2048, 0, None) == ALIGN         # d_out % 8
    assert dh(ok(), HDRS, None, None, OUT, 1024, 0, None) == CAPACITY          # pitch < width
    two = lambda: ctypes.byref(_frame(n_frames=2, d_frame_code_offsets=0x80000))
    assert dh(two(), HDRS, None, None, OUT, 2048, 2048 * 1536 + 4, None) == ALIGN   # frame stride % 8
    assert dh(two(), HDRS, None, None, OUT, 2048, 2048 * 1535, None) == CAPACITY    # frames overlap
    # dims are checked before alignment, alignment before capacity (mh_decode's order)
    assert dh(bad_dims, HDRS, None, None, OUT, 2044, 0, None) == DIMS
    assert dh(ok(), HDRS, None, None, OUT + 4, 1024, 0, None) == ALIGN
    # NULL headers come before the dims, as NULL d_luts does in mh_decode_frames
    assert dh(bad_dims, None, None, None, OUT, 2048, 0, None) == INVALID
    assert L.mh_decode_frames(bad_dims, None, _stride(mh), None, OUT, 2048, 0, None) == INVALID


def test_decode_headers_shape_rejects_bad_arguments(mh):
    from metalhuffman_amd import _native as N
    L = N.lib()
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    sh = L.mh_decode_headers_shape
    assert sh(None, None, ctypes.byref(g), ctypes.byref(w)) == INVALID
    assert sh(ctypes.byref(_frame()), None, None, ctypes.byref(w)) == INVALID
    assert sh(ctypes.byref(_frame()), None, ctypes.byref(g), None) == INVALID
    assert sh(ctypes.byref(_frame(n_frames=0)), None, ctypes.byref(g), ctypes.byref(w)) == INVALID
    assert sh(ctypes.byref(_frame(flags=0x2)), None, ctypes.byref(g), ctypes.byref(w)) == INVALID
    assert sh(ctypes.byref(_frame(dims=N.mh_dims(16, 16, 3, 2))), None, ctypes.byref(g), ctypes.byref(w)) == DIMS


def test_header_luts_rejects_bad_arguments(mh):
    """mh_build_luts_device's rules."""
    from metalhuffman_amd import _native as N
    L, st = N.lib(), _stride(mh)
    for fn in (L.mh_header_luts_device, L.mh_build_luts_device):
        assert fn(None, 4, LUTS, st, None, None) == INVALID
        assert fn(0x10000, 4, None, st, None, None) == INVALID
        assert fn(0x10000, 0, LUTS, st, None, None) == INVALID
        assert fn(0x10000, 65536, LUTS, st, None, None) == INVALID
        assert fn(0x10000, 4, LUTS + 4, st, None, None) == ALIGN
        assert fn(0x10000, 4, LUTS, st + 4, None, None) == ALIGN
        assert fn(0x10000, 4, LUTS, st - 16, None, None) == CAPACITY


def test_stream_entries_reject_null_handles(mh):
    """The header-mode stream entries refuse NULL handles and arguments before any HIP call."""
    from metalhuffman_amd import _native as N
    L = N.lib()
    h = ctypes.c_void_p()
    proto = _frame()
    assert L.mh_stream_create_headers(None, 4096, 2, None, ctypes.byref(h)) == INVALID
    assert L.mh_stream_create_headers(ctypes.byref(proto), 4096, 0, None, ctypes.byref(h)) == INVALID
    assert L.mh_stream_create_headers(ctypes.byref(proto), 4096, 65, None, ctypes.byref(h)) == INVALID
    assert L.mh_stream_create_headers(ctypes.byref(proto), 2, 2, None, ctypes.byref(h)) == INVALID
    assert L.mh_stream_create_headers(ctypes.byref(_frame(dims=N.mh_dims(16, 16, 3, 2))), 4096, 2, None,
                                      ctypes.byref(h)) == DIMS
    assert L.mh_stream_submit_header(None, 0x1000, 0x2000, 64, 0x3000, None, None) == INVALID
    st = ctypes.c_int32(5)
    assert L.mh_stream_slot_status(None, 0, ctypes.byref(st)) == INVALID
