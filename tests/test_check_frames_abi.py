"""The C-ABI of the per-frame-table check (include/metalhuffman.h: mh_check_frames, mh_check_headers, their
*_shape twins, MH_ERR_STREAM): exported, declared, and every argument check made before any HIP call, in
mh_decode_frames' / mh_decode_headers' order, with fake pointers. CPU only."""
from __future__ import annotations

import ctypes
import os

import pytest

INVALID, DIMS, CAPACITY, TABLE, ALIGN, HIP, STREAM = -1, -2, -4, -5, -6, -7, -9
LUTS, HEADERS, STATUS, HSTATUS, REPORT, VERDICT = 0x60000, 0x61000, 0x70000, 0x71000, 0x72000, 0x73000
SHORT = dict(codes_bytes=2)   # fails the codes' capacity rule, behind every alignment rule


def _frame(**kw):
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


def _frames(mh, fr=None, luts=LUTS, stride=None, status=STATUS, report=REPORT, verdict=VERDICT):
    """mh_check_frames; the default frame stops at the codes' capacity rule, so no call reaches a launch."""
    fr = _frame(**SHORT) if fr is None else fr
    return mh.lib().mh_check_frames(ctypes.byref(fr) if fr is not False else None, luts,
                                    _stride(mh) if stride is None else stride, status, report, verdict, None)


def _headers(mh, fr=None, headers=HEADERS, status=STATUS, hstatus=HSTATUS, report=REPORT, verdict=VERDICT):
    fr = _frame(**SHORT) if fr is None else fr
    return mh.lib().mh_check_headers(ctypes.byref(fr) if fr is not False else None, headers, status, hstatus, report,
                                     verdict, None)


def test_symbols_exported_and_declared(mh):
    lib = ctypes.CDLL(mh.LIB_PATH)
    names = ("mh_check_frames", "mh_check_frames_shape", "mh_check_headers", "mh_check_headers_shape",
             "mh_check_frame_cpu")
    header = open(os.path.join(os.path.dirname(os.path.dirname(mh.LIB_PATH)), "include", "metalhuffman.h")).read()
    for name in names:
        assert hasattr(lib, name), name
        assert name in mh.EXPORTS, name
        assert f"int {name}(" in header, name
    assert "#define MH_ERR_STREAM (-9)" in header
    assert "Not covered: mh_check with per-frame" not in header
    assert "Word [1] is always 0" in header
    assert mh.MH_ERR_STREAM == STREAM
    assert mh.lib().mh_error_string(STREAM) not in (b"unknown error", mh.lib().mh_error_string(-8))
    from metalhuffman_amd import decoder as D, encoder as E
    assert callable(D.check_frames) and callable(D.check_headers) and callable(mh.check_frame)
    assert callable(E.AsyncEncodedBatch.check)


def test_aliasing_pairs_are_refused_first(mh):
    """verdict / frame status, verdict / header status, header status / frame status: MH_ERR_INVALID_ARG,
    ahead of every other rule (a frame with bad dims, a misaligned table)."""
    from metalhuffman_amd import _native as N
    bad = _frame(dims=N.mh_dims(2048, 1536, 255, 192))
    for fr in (None, bad):
        assert _frames(mh, fr, status=VERDICT) == INVALID
        assert _headers(mh, fr, status=VERDICT) == INVALID
        assert _headers(mh, fr, hstatus=VERDICT) == INVALID
        assert _headers(mh, fr, hstatus=STATUS) == INVALID
    assert _frames(mh, luts=LUTS + 8, status=VERDICT) == INVALID
    # NULL arrays alias nothing
    assert _frames(mh, status=None, verdict=None) == CAPACITY
    assert _headers(mh, status=None, hstatus=None, verdict=None) == CAPACITY
    assert _headers(mh, status=None, hstatus=None) == CAPACITY


@pytest.mark.parametrize("call", ["frames", "headers"])
def test_null_and_frame_rules(mh, call):
    go = _frames if call == "frames" else _headers
    short = lambda **kw: _frame(**dict(SHORT, **kw))
    assert go(mh, False) == INVALID
    assert go(mh, report=None) == INVALID                                 # the report is required
    assert go(mh, verdict=None) == CAPACITY                               # the verdict is not
    assert go(mh, status=None) == CAPACITY
    assert (go(mh, luts=None) if call == "frames" else go(mh, headers=None)) == INVALID
    for kw, status in ((dict(d_codes=None), INVALID), (dict(d_block_offsets=None), INVALID),
                       (dict(n_frames=0), INVALID), (dict(n_frames=2), INVALID),
                       (dict(flags=0x2), INVALID), (dict(flags=0x8), INVALID),
                       (dict(flags=0x1 | 0x4), CAPACITY),                 # NO_DELTA | ANY_ORDER are accepted
                       (dict(table2_entries=100), CAPACITY),              # the table fields are ignored ...
                       (dict(d_lut=0x70004), CAPACITY),                   # ... a misaligned d_lut included
                       (dict(d_codes=0x20004), ALIGN)):
        assert go(mh, short(**kw)) == status, kw
    from metalhuffman_amd import _native as N
    assert go(mh, short(dims=N.mh_dims(2048, 1536, 255, 192))) == DIMS
    assert go(mh, short(dims=N.mh_dims(0, 1536, 0, 192))) == DIMS
    # no raster arguments: nothing asks for a pitch or an output pointer
    assert go(mh, report=REPORT + 2) == ALIGN
    assert go(mh, verdict=VERDICT + 1) == ALIGN
    assert go(mh, report=REPORT + 4, verdict=VERDICT + 4) == CAPACITY      # 4-byte alignment is enough


def test_order_invalid_dims_align_capacity(mh):
    from metalhuffman_amd import _native as N
    st = _stride(mh)
    bad_dims = _frame(dims=N.mh_dims(2048, 1536, 255, 192), **SHORT)
    for go in (_frames, _headers):
        assert go(mh, _frame(flags=0x8, dims=N.mh_dims(2048, 1536, 255, 192)), report=REPORT + 2) == INVALID
        assert go(mh, bad_dims, report=REPORT + 2) == DIMS
        assert go(mh, report=None, verdict=VERDICT + 2) == INVALID
        assert go(mh, report=REPORT + 2) == ALIGN                          # ahead of the codes' capacity
    assert _frames(mh, bad_dims, luts=LUTS + 8, stride=st - 16) == DIMS
    assert _frames(mh, luts=LUTS + 8, stride=st - 16) == ALIGN
    assert _frames(mh, _frame(), stride=st - 16, report=REPORT + 1) == ALIGN
    assert _frames(mh, _frame(), stride=st - 16) == CAPACITY


def test_stride_rules(mh):
    """mh_decode_region's: 0 is one table for all frames, any other stride a multiple of 16 and at least
    mh_lut_bytes(); the headers entry has no stride and no alignment rule for its headers."""
    st = _stride(mh)
    ok = _frame()
    assert _frames(mh, ok, stride=8) == ALIGN
    assert _frames(mh, ok, stride=st + 8) == ALIGN
    assert _frames(mh, ok, luts=LUTS + 8) == ALIGN
    assert _frames(mh, ok, stride=16) == CAPACITY
    assert _frames(mh, ok, stride=st - 16) == CAPACITY
    assert _frames(mh, stride=0) == CAPACITY and _frames(mh, stride=st) == CAPACITY    # (the short frame's code)
    assert _headers(mh, headers=HEADERS + 1) == CAPACITY
    # mh_decode_frames itself keeps refusing stride 0
    assert mh.lib().mh_decode_frames(ctypes.byref(ok), LUTS, 0, None, 0x50000, 2048, 0, None) == CAPACITY


def test_accepted_calls_reach_the_device(mh):
    """A call that passes every check ends in MH_ERR_HIP on a machine without a device: there the first HIP
    call finds none. (With a device the fake pointers must not be launched on; test_gpu_check_frames.py
    makes the same calls with real buffers.)"""
    if mh.lib().mh_device_count() > 0:
        return
    two = _frame(n_frames=2, d_frame_code_offsets=0x80000)
    for fr in (_frame(), two, _frame(flags=0x5)):
        assert _frames(mh, fr, stride=0) == HIP
        assert _frames(mh, fr) == HIP
        assert _frames(mh, fr, status=None, verdict=None) == HIP
        assert _headers(mh, fr) == HIP
        assert _headers(mh, fr, status=None, hstatus=None, verdict=None) == HIP


def test_tile_capacity(mh):
    from metalhuffman_amd import _native as N
    big = lambda n: _frame(dims=N.mh_dims(65535, 65535, 8192, 8192), n_frames=n, d_frame_code_offsets=0x80000)
    assert _frames(mh, big(2048)) == CAPACITY and _headers(mh, big(2048)) == CAPACITY     # 2^31 tiles
    if mh.lib().mh_device_count() == 0:
        assert _frames(mh, big(2047)) == HIP


@pytest.mark.parametrize("entry", ["mh_check_frames_shape", "mh_check_headers_shape"])
def test_shape_entries(mh, entry):
    from metalhuffman_amd import _native as N
    fn = getattr(mh.lib(), entry)
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    G, W = ctypes.byref(g), ctypes.byref(w)
    ok = lambda **kw: ctypes.byref(_frame(**kw))
    assert fn(None, None, G, W) == INVALID
    assert fn(ok(), None, None, W) == INVALID
    assert fn(ok(), None, G, None) == INVALID
    assert fn(ok(n_frames=0), None, G, W) == INVALID
    assert fn(ok(flags=0x2), None, G, W) == INVALID
    assert fn(ok(dims=N.mh_dims(16, 16, 3, 2)), None, G, W) == DIMS
    if mh.lib().mh_device_count() == 0:
        assert fn(ok(), None, G, W) == HIP
