"""The C-ABI of the windows entries (include/metalhuffman.h: mh_decode_windows,
mh_decode_windows_shape): exported, and every host check made before any HIP call, with fake
pointers, in mh_decode_region's order; decoder.windows_of_rects; decode_windows' validation of a
host list. CPU only. (The windows themselves live in device memory and are judged by the kernel:
tests/test_gpu_windows.py.)"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

INVALID, DIMS, CAPACITY, ALIGN, HIP = -1, -2, -4, -6, -7
LUTS, OUT, WINDOWS, FSTATUS, WSTATUS = 0x60000, 0x50000, 0x90000, 0xA0000, 0xB0000
BW, BH = 32, 24                       # the default window size, blocks
PITCH, WSTRIDE = 8 * BW, 8 * BW * 8 * BH


def _frame(**kw):
    """A frame mh_decode_windows accepts: 2048 x 1536 (256 x 192 blocks), the table fields NULL / 0."""
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


def _call(mh, fr=None, windows=WINDOWS, n=4, size=(BW, BH), luts=LUTS, stride=None, fstatus=None, wstatus=None,
          out=OUT, pitch=PITCH, wstride=WSTRIDE):
    """mh_decode_windows with defaults that pass every check; the callers that must not reach a
    launch stop it with codes_bytes = 2 (SHORT), the last-but-one capacity rule."""
    from metalhuffman_amd import _native as N
    fr = _frame() if fr is None else fr
    return N.lib().mh_decode_windows(ctypes.byref(fr) if fr is not False else None, windows, n, size[0], size[1],
                                     luts, _stride(mh) if stride is None else stride, fstatus, wstatus, out, pitch,
                                     wstride, None)


SHORT = dict(codes_bytes=2)


def _short(**kw):
    return _frame(**dict(SHORT, **kw))


def test_windows_symbols_exported(mh):
    lib = ctypes.CDLL(mh.LIB_PATH)
    for name in ("mh_decode_windows", "mh_decode_windows_shape"):
        assert hasattr(lib, name), name
        assert name in mh.EXPORTS, name
    from metalhuffman_amd import _native as N
    assert ctypes.sizeof(N.mh_window) == 16 and ctypes.sizeof(N.mh_region) == 16
    assert [f[0] for f in N.mh_window._fields_] == ["frame", "bx0", "by0", "reserved"]
    assert N.mh_window.by0.offset == 8 and N.mh_window.reserved.offset == 12


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
def test_windows_rejects_bad_frames(mh, kw, status):
    assert _call(mh, _frame(**kw)) == status


def test_windows_rejects_bad_arguments(mh):
    """Every host check with its code: mh_decode_region's, n_windows rasters of 8 bw x 8 bh in the
    place of n_frames rasters of RW x RH, and the additions for the descriptor array."""
    from metalhuffman_amd import _native as N
    st = _stride(mh)
    # MH_ERR_INVALID_ARG
    assert _call(mh, False) == INVALID                                   # NULL frame
    assert _call(mh, out=None) == INVALID
    assert _call(mh, luts=None) == INVALID
    assert _call(mh, windows=None) == INVALID                            # NULL d_windows
    assert _call(mh, n=0) == INVALID                                     # no windows
    assert _call(mh, fstatus=FSTATUS, wstatus=FSTATUS) == INVALID        # the two status arrays alias
    assert _call(mh, _short(), fstatus=FSTATUS, wstatus=WSTATUS) == CAPACITY   # (distinct ones pass)
    assert _call(mh, _short(), wstatus=WSTATUS) == CAPACITY
    # MH_ERR_DIMS: the frame's, then the window size's
    assert _call(mh, _short(dims=N.mh_dims(2048, 1536, 255, 192))) == DIMS
    for size in ((0, 1), (1, 0), (0, 0), (257, 1), (1, 193), (0xFFFFFFFF, 1), (1, 0xFFFFFFFF)):
        assert _call(mh, size=size) == DIMS, size
    for size in ((256, 192), (1, 1), (256, 1), (1, 192)):                # sizes up to the whole grid are inside:
        assert _call(mh, _short(), size=size, pitch=2044) == ALIGN, size  # they get past the dims check
    # MH_ERR_ALIGN
    assert _call(mh, pitch=PITCH + 4) == ALIGN                           # pitch % 8
    assert _call(mh, out=OUT + 4) == ALIGN                               # d_out % 8
    assert _call(mh, wstride=WSTRIDE + 4) == ALIGN                       # window stride % 8 (n_windows > 1)
    assert _call(mh, windows=WINDOWS + 8) == ALIGN                       # d_windows % 16
    assert _call(mh, windows=WINDOWS + 4) == ALIGN
    assert _call(mh, luts=LUTS + 8) == ALIGN                             # d_luts % 16
    assert _call(mh, stride=st + 8) == ALIGN                             # table stride % 16
    assert _call(mh, stride=8) == ALIGN
    # MH_ERR_CAPACITY
    assert _call(mh, pitch=PITCH - 8) == CAPACITY                        # pitch < 8 bw
    assert _call(mh, pitch=(1 << 20) + 8) == CAPACITY
    assert _call(mh, wstride=WSTRIDE - 8) == CAPACITY                    # window slots overlap
    assert _call(mh, wstride=0) == CAPACITY
    assert _call(mh, pitch=PITCH + 8, wstride=WSTRIDE) == CAPACITY       # the stride follows the pitch
    assert _call(mh, _short()) == CAPACITY                               # codes_bytes < MH_CODES_PAD
    assert _call(mh, stride=st - 16) == CAPACITY                         # 0 < table stride < mh_lut_bytes()
    assert _call(mh, stride=16) == CAPACITY
    # the FULL 8 bw x 8 bh per slot, whatever the frame's edge clips: in a 2045 x 1531 frame a region at the
    # bottom edge has RH = 187 and mh_decode_region takes a frame stride of 256 * 187; a window slot is 192 rows
    edge = lambda: _frame(dims=N.mh_dims(2045, 1531, 256, 192))
    assert _call(mh, edge(), wstride=PITCH * 187) == CAPACITY
    assert _call(mh, edge(), wstride=PITCH * 191) == CAPACITY
    assert _call(mh, _short(dims=N.mh_dims(2045, 1531, 256, 192)), wstride=PITCH * 192, pitch=PITCH + 4) == ALIGN
    # a window as wide as a frame that is 2045 pixels wide still needs 8 * 256 = 2048 bytes per row
    assert _call(mh, edge(), size=(256, 1), pitch=2040, wstride=2048 * 8) == CAPACITY


def test_windows_check_order(mh):
    """Invalid argument before dims, dims before alignment, alignment before capacity
    (mh_decode_region's order); the window size counts as dims, the descriptor array's alignment
    as alignment."""
    from metalhuffman_amd import _native as N
    st = _stride(mh)
    bad_dims = _frame(dims=N.mh_dims(2048, 1536, 255, 192))
    assert _call(mh, _frame(flags=0x8), size=(257, 1)) == INVALID
    assert _call(mh, bad_dims, windows=None) == INVALID
    assert _call(mh, bad_dims, n=0) == INVALID
    assert _call(mh, size=(0, 1), fstatus=FSTATUS, wstatus=FSTATUS) == INVALID
    assert _call(mh, bad_dims, windows=WINDOWS + 8, stride=st - 16, pitch=252) == DIMS
    assert _call(mh, size=(257, 24), windows=WINDOWS + 8, luts=LUTS + 8, stride=st - 16, pitch=252) == DIMS
    assert _call(mh, windows=WINDOWS + 8, stride=st - 16, pitch=PITCH - 8) == ALIGN
    assert _call(mh, luts=LUTS + 8, pitch=PITCH - 8) == ALIGN
    assert _call(mh, wstride=WSTRIDE - 4) == ALIGN                       # misaligned AND too small
    assert _call(mh, stride=8, wstride=0) == ALIGN
    assert _call(mh, _short(), stride=st - 16, pitch=PITCH - 8) == CAPACITY


def test_windows_accepted_calls_reach_the_device(mh):
    """Every capacity rule answers MH_ERR_CAPACITY, so "passed the checks" shows only in a call that
    passes them all: without a HIP device such a call ends in MH_ERR_HIP (the first HIP call finds
    no device). With a device the fake pointers must not be launched on; there
    tests/test_gpu_windows.py makes the same calls with real buffers."""
    from metalhuffman_amd import _native as N
    assert _call(mh, stride=16) == CAPACITY and _call(mh, pitch=PITCH - 8) == CAPACITY
    if N.lib().mh_device_count() > 0:
        return
    assert _call(mh) == HIP
    assert _call(mh, stride=0) == HIP                                     # the shared table
    assert _call(mh, fstatus=FSTATUS, wstatus=WSTATUS) == HIP
    assert _call(mh, n=1, wstride=0) == HIP and _call(mh, n=1, wstride=12) == HIP   # one window: no stride rule
    assert _call(mh, pitch=PITCH + 8, wstride=(PITCH + 8) * 8 * BH) == HIP
    assert _call(mh, size=(256, 192), pitch=2048, wstride=2048 * 1536) == HIP       # the whole grid
    two = _frame(n_frames=2, d_frame_code_offsets=0x80000)
    assert _call(mh, two, n=1000) == HIP                                  # more windows than frames
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    assert N.lib().mh_decode_windows_shape(ctypes.byref(_frame()), 4, BW, BH, None, ctypes.byref(g),
                                           ctypes.byref(w)) == HIP


def test_windows_tile_capacity(mh):
    """More than 2^31 - 1 tiles: a window of 8192 x 8192 blocks is 8192 * 128 = 2^20 tiles, so 2048 of
    them are 2^31 -- counted over the WINDOWS, whatever n_frames is."""
    from metalhuffman_amd import _native as N
    big = lambda n: _frame(dims=N.mh_dims(65535, 65535, 8192, 8192), n_frames=n, d_frame_code_offsets=0x80000)
    full = dict(size=(8192, 8192), pitch=65536, wstride=65536 * 65536)
    assert _call(mh, big(1), n=2048, **full) == CAPACITY
    assert _call(mh, big(4096), n=2048, **full) == CAPACITY
    row = dict(size=(8192, 1), pitch=65536, wstride=65536 * 8)           # 128 tiles per window
    assert _call(mh, big(2), n=1 << 24, **row) == CAPACITY
    L = N.lib()
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.mh_decode_windows_shape(ctypes.byref(big(1)), 2048, 8192, 8192, None, ctypes.byref(g),
                                     ctypes.byref(w)) == CAPACITY
    if L.mh_device_count() == 0:   # (accepted: MH_ERR_HIP without a device, see above)
        assert _call(mh, big(1), n=2047, **full) == HIP
        assert _call(mh, big(1 << 24), n=4, **row) == HIP                 # 2^31 tiles over the FRAMES do not count
        assert _call(mh, big(2), n=1 << 20, **row) == HIP


def test_windows_shape_rejects_bad_arguments(mh):
    from metalhuffman_amd import _native as N
    L = N.lib()
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    G, Wv = ctypes.byref(g), ctypes.byref(w)
    ok = lambda **kw: ctypes.byref(_frame(**kw))
    assert L.mh_decode_windows_shape(None, 4, BW, BH, None, G, Wv) == INVALID
    assert L.mh_decode_windows_shape(ok(), 4, BW, BH, None, None, Wv) == INVALID
    assert L.mh_decode_windows_shape(ok(), 4, BW, BH, None, G, None) == INVALID
    assert L.mh_decode_windows_shape(ok(), 0, BW, BH, None, G, Wv) == INVALID
    assert L.mh_decode_windows_shape(ok(n_frames=0), 4, BW, BH, None, G, Wv) == INVALID
    assert L.mh_decode_windows_shape(ok(flags=0x2), 4, BW, BH, None, G, Wv) == INVALID
    assert L.mh_decode_windows_shape(ok(dims=N.mh_dims(16, 16, 3, 2)), 4, 1, 1, None, G, Wv) == DIMS
    for size in ((0, 8), (8, 0), (257, 8), (8, 193), (0xFFFFFFFF, 1)):
        assert L.mh_decode_windows_shape(ok(), 4, size[0], size[1], None, G, Wv) == DIMS, size


# ---- decoder.windows_of_rects ---------------------------------------------------------------------

W, H = 597, 67   # 75 x 9 blocks, partial right and bottom blocks


def test_windows_of_rects_offsets():
    """Each window starts at its rectangle's block; (dx, dy) is the rectangle's sub-block offset;
    region_of_rect's rounding rectangle by rectangle."""
    from metalhuffman_amd.decoder import region_of_rect, windows_of_rects
    f, x0, y0 = [2, 0, 1, 0], [0, 8, 29, 500], [0, 16, 13, 40]
    wins, size, dx, dy = windows_of_rects(W, H, f, x0, y0, 24, 16)
    assert wins.shape == (4, 3) and wins.dtype.kind == "i"
    assert wins.tolist() == [[2, 0, 0], [0, 1, 2], [1, 3, 1], [0, 62, 5]]
    assert dx.tolist() == [0, 0, 5, 4] and dy.tolist() == [0, 0, 5, 0]
    # 24 pixels at offset 0 are 3 blocks, at offset 5 (or 4) they are 4: one size for all
    assert size == (4, 3)
    for i in range(4):
        rg, ddx, ddy = region_of_rect(W, H, x0[i], y0[i], 24, 16)
        assert (rg.bx0, rg.by0) == tuple(wins[i, 1:]) and (ddx, ddy) == (dx[i], dy[i])
        assert rg.bw <= size[0] and rg.bh <= size[1]
    # rectangle i lies inside its window at (dx, dy)
    assert ((dx + 24 <= 8 * size[0]) & (dy + 16 <= 8 * size[1])).all()


def test_windows_of_rects_one_size():
    from metalhuffman_amd.decoder import windows_of_rects
    # on the grid: exactly the rectangle's blocks
    wins, size, dx, dy = windows_of_rects(W, H, [0, 1], [8, 64], [16, 0], 8, 8)
    assert size == (1, 1) and wins.tolist() == [[0, 1, 2], [1, 8, 0]] and not dx.any() and not dy.any()
    # one rectangle straddles a block boundary in x only, another in y only: the size grows in both
    wins, size, dx, dy = windows_of_rects(W, H, [0, 0], [7, 8], [8, 7], 8, 8)
    assert size == (2, 2) and wins.tolist() == [[0, 0, 1], [0, 1, 0]]
    assert dx.tolist() == [7, 0] and dy.tolist() == [0, 7]
    # scalars are one rectangle; the frame's last pixels
    wins, size, dx, dy = windows_of_rects(W, H, 2, 592, 64, 5, 3)
    assert wins.tolist() == [[2, 74, 8]] and size == (1, 1) and (int(dx[0]), int(dy[0])) == (0, 0)
    wins, size, dx, dy = windows_of_rects(W, H, [1], [0], [0], W, H)
    assert wins.tolist() == [[1, 0, 0]] and size == (75, 9)


def test_windows_of_rects_errors():
    from metalhuffman_amd.decoder import windows_of_rects
    for bad in (([0], [0], [0], 0, 1), ([0], [0], [0], 1, 0), ([0], [-1], [0], 2, 2), ([0], [0], [-1], 2, 2),
                ([0], [590], [0], 8, 1), ([0], [0], [60], 1, 8), ([0], [597], [0], 1, 1), ([0], [0], [67], 1, 1),
                ([0], [0], [0], 598, 1), ([-1], [0], [0], 1, 1), ([0, 0], [0, 590], [0, 0], 8, 8)):
        with pytest.raises(ValueError):
            windows_of_rects(W, H, *bad)
    with pytest.raises(ValueError):
        windows_of_rects(0, 8, [0], [0], [0], 1, 1)
    with pytest.raises(ValueError):
        windows_of_rects(W, H, [0, 1], [0], [0], 1, 1)                    # arrays of different lengths
    # every rectangle lies inside the frame, but the window GROWN to the common size does not: the first
    # rectangle needs 2 blocks (offset 4), and 2 blocks from the second's block 74 leave the 75-block grid
    with pytest.raises(ValueError, match="leaves the 75x9 block grid"):
        windows_of_rects(W, H, [0, 0], [4, 592], [0, 0], 5, 3)
    with pytest.raises(ValueError, match="leaves the 75x9 block grid"):
        windows_of_rects(W, H, [0, 0], [0, 0], [6, 64], 3, 3)
    wins, size, _, _ = windows_of_rects(W, H, [0, 0], [4, 584], [0, 0], 5, 3)   # (one block earlier it fits)
    assert size == (2, 1) and wins.tolist() == [[0, 0, 0], [0, 73, 0]]


# ---- decode_windows' validation of a host list -----------------------------------------------------

def _host_frames(n=3):
    """A DeviceFrames description with host tensors: decode_windows validates the size and a host list
    before it looks at a buffer, so these calls end in the ValueError under test (or, for a valid list,
    in the ValueError that the buffers are not on a HIP device)."""
    import torch
    from metalhuffman_amd import decoder as D
    z = torch.zeros(16, dtype=torch.uint8)
    return D.DeviceFrames(W, H, n, torch.zeros(4, dtype=torch.int32), z, None)


@pytest.mark.parametrize("windows,size", [
    ([(3, 0, 0)], (10, 3)),                    # frame >= n_frames
    ([(0, 0, 0), (-1, 0, 0)], (10, 3)),
    ([(0, 66, 0)], (10, 3)),                   # bx0 + bw > 75
    ([(0, 0, 7)], (10, 3)),                    # by0 + bh > 9
    ([(0, -1, 0)], (10, 3)),
    ([(0, 0, -1)], (10, 3)),
    ([(0, 0xFFFFFFFF, 0)], (10, 3)),
    ([(0, 1, 0)], (75, 9)),
    ([(0, 0, 0, 0)], (10, 3)),                 # a host list is (frame, bx0, by0)
    ([], (10, 3)),
    ([(0.5, 0, 0)], (10, 3)),
])
def test_decode_windows_rejects_bad_host_lists(windows, size):
    from metalhuffman_amd import decoder as D
    with pytest.raises(ValueError, match="window"):
        D.decode_windows(_host_frames(), None, windows, size)
    with pytest.raises(ValueError, match="window"):
        D.decode_windows(_host_frames(), None, np.asarray(windows), size)


@pytest.mark.parametrize("size", [(0, 3), (10, 0), (76, 3), (10, 10), (-1, 3)])
def test_decode_windows_rejects_bad_sizes(size):
    from metalhuffman_amd import decoder as D
    with pytest.raises(ValueError, match="does not fit"):
        D.decode_windows(_host_frames(), None, [(0, 0, 0)], size)
    with pytest.raises(ValueError, match="does not fit"):
        D.decode_windows_shape(_host_frames(), 1, size)


def test_decode_windows_accepts_good_host_lists():
    """The same call with windows at the grid's corners gets past the list's validation: it ends at
    the next check (the buffers are host tensors)."""
    from metalhuffman_amd import decoder as D
    good = [(0, 0, 0), (2, 65, 6), (1, 65, 0), (0, 0, 6)]
    assert D._host_windows(_host_frames(), good, 10, 3).tolist() == [list(g) + [0] for g in good]
    assert D._host_windows(_host_frames(), good, 10, 3).dtype == np.int32
    with pytest.raises(ValueError, match="HIP device"):
        D.decode_windows(_host_frames(), None, good, (10, 3))
