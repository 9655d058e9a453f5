"""The C-ABI of the shared-table batch encoder (include/metalhuffman.h:
mh_encode_frames_shared_device_async, mh_encode_frames_shared_workspace_bytes and the host twins):
exported, and every host check made before any HIP call, with fake pointers, in
mh_encode_frames_device_async's order. CPU only: a call that passed every check would launch, so
each case here fails one check and the cases that probe the ORDER fail two, expecting the earlier
one's code."""
from __future__ import annotations

import ctypes

import pytest

OK, INVALID, DIMS, CAPACITY, ALIGN = 0, -1, -2, -4, -6
GRAY, CANON_IN, CANON, CODES, LENS, FCO, OFFS, INIT, STATUS, HSTATUS, WS = (
    0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 0x90000, 0xA0000, 0x100000)
W, H, N = 64, 64, 2


def _args(mh, **kw):
    a = dict(gray=GRAY, gstride=W * H, n=N, w=W, h=H, flags=0, canon_in=None, canon=CANON, codes=CODES, slot=16384,
             lens=LENS, fco=FCO, offs=OFFS, init=None, status=STATUS, hstatus=HSTATUS, ws=WS, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = int(mh.lib().mh_encode_frames_shared_workspace_bytes(a["w"], a["h"], a["n"]))
    return a


def _shared(mh, **kw):
    a = _args(mh, **kw)
    return mh.lib().mh_encode_frames_shared_device_async(
        a["gray"], a["gstride"], a["n"], a["w"], a["h"], a["flags"], a["canon_in"], a["canon"], a["codes"], a["slot"],
        a["lens"], a["fco"], a["offs"], a["init"], a["status"], a["hstatus"], a["ws"], a["ws_bytes"], None)


def _per_frame(mh, **kw):
    """The same arguments to mh_encode_frames_device_async (its workspace is the smaller one)."""
    a = _args(mh, **kw)
    return mh.lib().mh_encode_frames_device_async(
        a["gray"], a["gstride"], a["n"], a["w"], a["h"], a["flags"], a["canon"], a["codes"], a["slot"], a["lens"],
        a["fco"], a["offs"], a["init"], a["status"], a["ws"], a["ws_bytes"], None)


def test_symbols_exported(mh):
    lib = ctypes.CDLL(mh.LIB_PATH)
    for name in ("mh_encode_frames_shared_device_async", "mh_encode_frames_shared_workspace_bytes",
                 "mh_frame_histogram", "mh_encode_frame_with_header"):
        assert hasattr(lib, name), name
        assert name in mh.EXPORTS, name


def test_workspace_covers_the_per_frame_one(mh):
    L = mh.lib()
    for w, h, n in [(1, 1, 1), (64, 64, 2), (2048, 1536, 64), (1040, 1032, 3)]:
        shared = int(L.mh_encode_frames_shared_workspace_bytes(w, h, n))
        assert shared % 256 == 0 and shared > int(L.mh_encode_frames_workspace_bytes(w, h, n))


# one failing check each, with mh_encode_frames_device_async's code for the same arguments
SINGLE = [
    (dict(gray=None), INVALID), (dict(codes=None), INVALID), (dict(offs=None), INVALID), (dict(ws=None), INVALID),
    (dict(n=0), INVALID),
    (dict(flags=0x40), INVALID), (dict(flags=0x2), INVALID), (dict(flags=0x400), INVALID),
    (dict(w=0), DIMS), (dict(h=0), DIMS), (dict(w=65536), DIMS), (dict(h=65536), DIMS),
    (dict(codes=CODES + 4), ALIGN), (dict(slot=16380), ALIGN), (dict(ws=WS + 128), ALIGN),
    (dict(gstride=W * H - 1), CAPACITY),
    (dict(ws_bytes=0), CAPACITY),
]


@pytest.mark.parametrize("kw,status", SINGLE)
def test_each_check_and_its_code(mh, kw, status):
    assert _shared(mh, **kw) == status
    assert _shared(mh, canon_in=CANON_IN, **kw) == status          # supplied mode: the same checks
    assert _per_frame(mh, **kw) == status


def test_short_workspace(mh):
    need = int(mh.lib().mh_encode_frames_shared_workspace_bytes(W, H, N))
    assert _shared(mh, ws_bytes=need - 1) == CAPACITY
    assert _shared(mh, canon_in=CANON_IN, ws_bytes=need - 1) == CAPACITY
    # the per-frame entry's workspace is too small for this one
    assert _shared(mh, ws_bytes=int(mh.lib().mh_encode_frames_workspace_bytes(W, H, N))) == CAPACITY


def test_header_pointers(mh):
    """Built mode needs d_canon_header; supplied mode does not. A short workspace stops the calls
    that pass this check before any launch."""
    assert _shared(mh, canon=None) == INVALID
    assert _shared(mh, canon=None, canon_in=CANON_IN, ws_bytes=0) == CAPACITY     # optional there
    assert _shared(mh, canon=CANON_IN, canon_in=CANON_IN, ws_bytes=0) == CAPACITY  # aliasing is allowed
    assert _shared(mh, lens=None, fco=None, status=None, hstatus=None, init=None, ws_bytes=0) == CAPACITY


# two failing checks: the earlier one's code, as in mh_encode_frames_device_async
ORDER = [
    (dict(gray=None, flags=0x40, w=0, codes=CODES + 4, ws_bytes=0), INVALID),   # NULL first
    (dict(flags=0x40, w=0), INVALID),                                           # flags before dims
    (dict(w=0, codes=CODES + 4), DIMS),                                         # dims before alignment
    (dict(h=65536, slot=1000), DIMS),
    (dict(codes=CODES + 4, gstride=1), ALIGN),                                  # alignment before the gray stride
    (dict(ws=WS + 16, ws_bytes=0), ALIGN),                                      # ... and before the workspace size
    (dict(gstride=1, ws_bytes=0), CAPACITY),
]


@pytest.mark.parametrize("kw,status", ORDER)
def test_check_order(mh, kw, status):
    assert _shared(mh, **kw) == status
    assert _shared(mh, canon_in=CANON_IN, **kw) == status
    assert _per_frame(mh, **kw) == status


def test_one_frame_ignores_the_gray_stride(mh):
    """n_frames == 1: the stride is unused (mh_encode_frames_device_async's rule)."""
    assert _shared(mh, n=1, gstride=0, ws_bytes=0) == CAPACITY
    assert _per_frame(mh, n=1, gstride=0, ws_bytes=0) == CAPACITY


def test_built_mode_symbol_limit(mh):
    """Built mode: the batch holds fewer than 2^32 symbols (32-bit tree weights), checked ahead of
    the workspace size; supplied mode builds no tree and has no such limit. 2048 x 1536 is
    3,145,728 symbols: 1,365 frames fit, 1,366 do not."""
    big = 1 << 62
    assert _shared(mh, w=2048, h=1536, n=1366, gstride=2048 * 1536, slot=1 << 23, ws_bytes=big) == CAPACITY
    # the same batch in supplied mode, and 1,365 frames in built mode, pass every check but the
    # workspace's (one byte short)
    for kw in (dict(n=1366, canon_in=CANON_IN), dict(n=1365)):
        need = int(mh.lib().mh_encode_frames_shared_workspace_bytes(2048, 1536, kw["n"]))
        assert _shared(mh, w=2048, h=1536, gstride=2048 * 1536, slot=1 << 23, ws_bytes=need - 1, **kw) == CAPACITY
