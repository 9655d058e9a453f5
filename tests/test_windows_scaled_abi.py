"""The C-ABI of the scaled windows entries (include/metalhuffman.h: mh_decode_windows_scaled,
mh_decode_windows_scaled_shape): exported, and every host check made before any HIP call, with fake
pointers -- mh_decode_windows' checks in its order, n_windows rasters of c bw x c bh in the place of
8 bw x 8 bh and c = 8 >> log2_scale in the place of 8 in the alignment rules; the scale reported
where mh_decode_region_scaled reports it; the Python wrappers' ValueErrors. CPU only."""
from __future__ import annotations

import ctypes

import pytest

INVALID, DIMS, CAPACITY, ALIGN, HIP = -1, -2, -4, -6, -7
LUTS, OUT, WINDOWS, FSTATUS, WSTATUS = 0x60000, 0x50000, 0x90000, 0xA0000, 0xB0000
BW, BH = 32, 24                       # the default window size, blocks
KS = (1, 2, 3)


def _frame(**kw):
    """A frame the entry accepts: 2048 x 1536 (256 x 192 blocks), the table fields NULL / 0."""
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


def _call(mh, k, fr=None, windows=WINDOWS, n=4, size=(BW, BH), luts=LUTS, stride=None, fstatus=None, wstatus=None,
          out=OUT, pitch=None, wstride=None):
    """mh_decode_windows_scaled with defaults that pass every check: the tight pitch c bw and slot
    stride c bw * c bh of the given size. Callers that must not reach a launch pass codes_bytes = 2
    (SHORT), the last-but-one capacity rule."""
    from metalhuffman_amd import _native as N
    fr = _frame() if fr is None else fr
    c = 8 >> k if k <= 3 else 1
    pitch = c * size[0] if pitch is None else pitch
    wstride = c * size[0] * c * size[1] if wstride is None else wstride
    return N.lib().mh_decode_windows_scaled(ctypes.byref(fr) if fr is not False else None, windows, n, size[0],
                                            size[1], k, luts, _stride(mh) if stride is None else stride, fstatus,
                                            wstatus, out, pitch, wstride, None)


def _call0(mh, fr=None, windows=WINDOWS, n=4, size=(BW, BH), luts=LUTS, stride=None, fstatus=None, wstatus=None,
           out=OUT, pitch=8 * BW, wstride=8 * BW * 8 * BH):
    """mh_decode_windows with the same arguments (the verdicts log2_scale = 0 must give)."""
    from metalhuffman_amd import _native as N
    fr = _frame() if fr is None else fr
    return N.lib().mh_decode_windows(ctypes.byref(fr) if fr is not False else None, windows, n, size[0], size[1],
                                     luts, _stride(mh) if stride is None else stride, fstatus, wstatus, out, pitch,
                                     wstride, None)


SHORT = dict(codes_bytes=2)


def _short(**kw):
    return _frame(**dict(SHORT, **kw))


def test_windows_scaled_symbols_exported(mh):
    lib = ctypes.CDLL(mh.LIB_PATH)
    for name in ("mh_decode_windows_scaled", "mh_decode_windows_scaled_shape"):
        assert hasattr(lib, name), name
        assert name in mh.EXPORTS, name
    from metalhuffman_amd import decoder as D
    assert callable(D.decode_windows_scaled) and callable(D.decode_windows_scaled_shape)


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
def test_windows_scaled_rejects_bad_frames(mh, k, kw, status):
    """The windows entry's frame cases, code for code, at every scale (0 forwards)."""
    assert _call(mh, k, _frame(**kw)) == status


@pytest.mark.parametrize("k", KS)
def test_windows_scaled_rejects_bad_arguments(mh, k):
    """Every host check with its code: mh_decode_windows', c for 8."""
    from metalhuffman_amd import _native as N
    st, c = _stride(mh), 8 >> k
    pitch, wstride = c * BW, c * BW * c * BH
    # MH_ERR_INVALID_ARG
    assert _call(mh, k, False) == INVALID                                   # NULL frame
    assert _call(mh, k, out=None) == INVALID
    assert _call(mh, k, luts=None) == INVALID
    assert _call(mh, k, windows=None) == INVALID                            # NULL d_windows
    assert _call(mh, k, n=0) == INVALID                                     # no windows
    assert _call(mh, k, fstatus=FSTATUS, wstatus=FSTATUS) == INVALID        # the two status arrays alias
    assert _call(mh, k, _short(), fstatus=FSTATUS, wstatus=WSTATUS) == CAPACITY   # (distinct ones pass)
    assert _call(mh, k, _short(), wstatus=WSTATUS) == CAPACITY
    # MH_ERR_DIMS: the frame's, then the window size's
    assert _call(mh, k, _short(dims=N.mh_dims(2048, 1536, 255, 192))) == DIMS
    for size in ((0, 1), (1, 0), (0, 0), (257, 1), (1, 193), (0xFFFFFFFF, 1), (1, 0xFFFFFFFF)):
        assert _call(mh, k, size=size) == DIMS, size
    for size in ((256, 192), (1, 1), (256, 1), (1, 192)):                   # sizes up to the whole grid are inside:
        assert _call(mh, k, _short(), size=size, windows=WINDOWS + 8) == ALIGN, size   # past the dims check
    # MH_ERR_ALIGN: the descriptor array and the tables as in mh_decode_windows
    assert _call(mh, k, windows=WINDOWS + 8) == ALIGN                       # d_windows % 16
    assert _call(mh, k, windows=WINDOWS + 4) == ALIGN
    assert _call(mh, k, luts=LUTS + 8) == ALIGN                             # d_luts % 16
    assert _call(mh, k, stride=st + 8) == ALIGN                             # table stride % 16
    assert _call(mh, k, stride=8) == ALIGN
    # ... and d_out, the pitch and (n_windows > 1) the window stride to c
    if c > 1:
        assert _call(mh, k, pitch=pitch + c // 2) == ALIGN                  # bw c + c / 2
        assert _call(mh, k, out=OUT + c // 2) == ALIGN
        assert _call(mh, k, wstride=wstride + c // 2) == ALIGN
        assert _call(mh, k, _short(), n=1, wstride=wstride + c // 2) == CAPACITY   # one window: no stride rule
    # ... and to no more than c: bw c + c is accepted by the alignment rule (stopped later by SHORT)
    assert _call(mh, k, _short(), pitch=pitch + c, wstride=(pitch + c) * c * BH) == CAPACITY
    assert _call(mh, k, _short(), out=OUT + c, pitch=pitch + c, wstride=(pitch + c) * c * BH + c) == CAPACITY
    # MH_ERR_CAPACITY: the pitch and stride minima
    assert _call(mh, k, pitch=pitch - c) == CAPACITY                        # pitch < bw c
    assert _call(mh, k, pitch=(1 << 20) + 8) == CAPACITY
    assert _call(mh, k, wstride=wstride - c) == CAPACITY                    # window slots overlap
    assert _call(mh, k, wstride=0) == CAPACITY
    assert _call(mh, k, pitch=pitch + c, wstride=wstride) == CAPACITY       # the stride follows the pitch
    assert _call(mh, k, _short()) == CAPACITY                               # codes_bytes < MH_CODES_PAD
    assert _call(mh, k, stride=st - 16) == CAPACITY                         # 0 < table stride < mh_lut_bytes()
    assert _call(mh, k, stride=16) == CAPACITY
    # the FULL c bw x c bh per slot, whatever the frame's edge clips (a bottom-edge region's SH is smaller)
    edge = lambda **kw: _frame(dims=N.mh_dims(2045, 1531, 256, 192), **kw)
    assert _call(mh, k, edge(), wstride=pitch * (c * BH - 1)) == CAPACITY
    assert _call(mh, k, edge(**SHORT), wstride=pitch * c * BH) == CAPACITY  # (passes the stride rule: SHORT)
    assert _call(mh, k, edge(), size=(256, 1), pitch=256 * c - c, wstride=256 * c * c) == CAPACITY


def test_windows_scaled_k3_any_pitch(mh):
    """k = 3: c = 1, so an odd d_out, pitch and window stride pass the alignment rule."""
    assert _call(mh, 3, _short(), out=OUT + 1, pitch=BW + 1, wstride=(BW + 1) * BH + 1) == CAPACITY
    assert _call(mh, 3, _short(), out=OUT + 3, pitch=BW + 3, wstride=(BW + 3) * BH) == CAPACITY
    assert _call(mh, 3, pitch=BW - 1) == CAPACITY                           # ... but not a pitch < bw c
    assert _call(mh, 3, pitch=BW + 1, wstride=(BW + 1) * BH - 1) == CAPACITY


def test_windows_scaled_bad_scale(mh):
    """log2_scale > 3 -> MH_ERR_INVALID_ARG, reported where a bad flag is: behind the NULL checks,
    ahead of the dims, the alignment and the capacity rules."""
    from metalhuffman_amd import _native as N
    for k in (4, 5, 8, 0xFFFFFFFF):
        assert _call(mh, k) == INVALID
        assert _call(mh, k, _frame(dims=N.mh_dims(2048, 1536, 255, 192))) == INVALID      # before dims
        assert _call(mh, k, size=(257, 1), windows=WINDOWS + 8, luts=LUTS + 8, pitch=3) == INVALID
        assert _call(mh, k, _short()) == INVALID


def test_windows_scaled_scale_zero_is_decode_windows(mh):
    """log2_scale = 0 forwards: mh_decode_windows' verdict for the same arguments, case by case."""
    from metalhuffman_amd import _native as N
    st = _stride(mh)
    P, WS = 8 * BW, 8 * BW * 8 * BH
    # (no case passes every check: the fake pointers must never be launched on)
    cases = [dict(fr=False), dict(out=None), dict(windows=None), dict(n=0),
             dict(fstatus=FSTATUS, wstatus=FSTATUS), dict(size=(257, 1)), dict(size=(0, 1)),
             dict(pitch=P + 4), dict(out=OUT + 4), dict(wstride=WS + 4), dict(windows=WINDOWS + 8),
             dict(luts=LUTS + 8), dict(stride=st + 8), dict(pitch=P - 8), dict(wstride=WS - 8), dict(wstride=0),
             dict(stride=st - 16), dict(fr=_short(), stride=0), dict(fr=_short(), n=1, wstride=12),
             dict(fr=_short(), n=1, wstride=WS + 4), dict(fr=_short())]
    seen = set()
    for kw in cases:
        a = _call(mh, 0, **dict(dict(pitch=P, wstride=WS), **kw))
        b = _call0(mh, **kw)
        assert a == b and a != 0 and a != HIP, (kw, a, b)
        seen.add(a)
    assert _call(mh, 0, _frame(dims=N.mh_dims(2048, 1536, 255, 192)), pitch=P, wstride=WS) == DIMS
    assert _call(mh, 0, _short(), pitch=P, wstride=WS) == CAPACITY
    assert {INVALID, DIMS, ALIGN, CAPACITY} <= seen
    # the full-size rules, not c's: a pitch of 8 bw + 4 is misaligned at k = 0 and aligned at k = 1
    assert _call(mh, 0, pitch=P + 4, wstride=WS) == ALIGN
    assert _call(mh, 1, _short(), pitch=4 * BW + 4, wstride=(4 * BW + 4) * 4 * BH) == CAPACITY


def test_windows_scaled_check_order(mh):
    """Invalid argument before dims, dims before alignment, alignment before capacity."""
    from metalhuffman_amd import _native as N
    st = _stride(mh)
    for k in KS:
        c = 8 >> k
        pitch, wstride = c * BW, c * BW * c * BH
        bad_dims = _frame(dims=N.mh_dims(2048, 1536, 255, 192))
        assert _call(mh, k, _frame(flags=0x8), size=(257, 1)) == INVALID
        assert _call(mh, k, bad_dims, windows=None) == INVALID
        assert _call(mh, k, bad_dims, n=0) == INVALID
        assert _call(mh, k, size=(0, 1), fstatus=FSTATUS, wstatus=FSTATUS) == INVALID
        assert _call(mh, k, bad_dims, windows=WINDOWS + 8, stride=st - 16, pitch=pitch - c) == DIMS
        assert _call(mh, k, size=(257, 24), windows=WINDOWS + 8, luts=LUTS + 8, stride=st - 16) == DIMS
        assert _call(mh, k, windows=WINDOWS + 8, stride=st - 16, pitch=pitch - c) == ALIGN
        assert _call(mh, k, luts=LUTS + 8, pitch=pitch - c) == ALIGN
        assert _call(mh, k, stride=8, wstride=0) == ALIGN
        if c > 1:
            assert _call(mh, k, wstride=wstride - c // 2) == ALIGN          # misaligned AND too small
        assert _call(mh, k, _short(), stride=st - 16, pitch=pitch - c) == CAPACITY


def test_windows_scaled_accepted_calls_reach_the_device(mh):
    """A call that passes every check ends in MH_ERR_HIP on a machine without a HIP device (the first
    HIP call finds none). With a device the fake pointers must not be launched on; there
    tests/test_gpu_windows_scaled.py makes the same calls with real buffers."""
    from metalhuffman_amd import _native as N
    if N.lib().mh_device_count() > 0:
        return
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    for k in KS:
        c = 8 >> k
        pitch = c * BW
        assert _call(mh, k) == HIP
        assert _call(mh, k, stride=0) == HIP                                 # the shared table
        assert _call(mh, k, fstatus=FSTATUS, wstatus=WSTATUS) == HIP
        assert _call(mh, k, n=1, wstride=0) == HIP                           # one window: no stride rule
        assert _call(mh, k, out=OUT + c, pitch=pitch + c, wstride=(pitch + c) * c * BH + c) == HIP
        assert _call(mh, k, size=(256, 192), pitch=256 * c, wstride=256 * c * 192 * c) == HIP
        two = _frame(n_frames=2, d_frame_code_offsets=0x80000)
        assert _call(mh, k, two, n=1000) == HIP                              # more windows than frames
        assert N.lib().mh_decode_windows_scaled_shape(ctypes.byref(_frame()), 4, BW, BH, k, None, ctypes.byref(g),
                                                      ctypes.byref(w)) == HIP
    assert _call(mh, 3, out=OUT + 1, pitch=BW + 1, wstride=(BW + 1) * BH + 1) == HIP


def test_windows_scaled_tile_capacity(mh):
    """More than 2^31 - 1 tiles, counted over the windows as in mh_decode_windows."""
    from metalhuffman_amd import _native as N
    big = lambda n: _frame(dims=N.mh_dims(65535, 65535, 8192, 8192), n_frames=n, d_frame_code_offsets=0x80000)
    for k in KS:
        c = 8 >> k
        full = dict(size=(8192, 8192), pitch=8192 * c, wstride=8192 * c * 8192 * c)
        assert _call(mh, k, big(1), n=2048, **full) == CAPACITY
        g, w = ctypes.c_uint32(), ctypes.c_uint32()
        assert N.lib().mh_decode_windows_scaled_shape(ctypes.byref(big(1)), 2048, 8192, 8192, k, None,
                                                      ctypes.byref(g), ctypes.byref(w)) == CAPACITY
        if N.lib().mh_device_count() == 0:
            assert _call(mh, k, big(1), n=2047, **full) == HIP


def test_windows_scaled_shape_rejects_bad_arguments(mh):
    from metalhuffman_amd import _native as N
    L = N.lib()
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    G, Wv = ctypes.byref(g), ctypes.byref(w)
    ok = lambda **kw: ctypes.byref(_frame(**kw))
    f = L.mh_decode_windows_scaled_shape
    for k in (0,) + KS:
        assert f(None, 4, BW, BH, k, None, G, Wv) == INVALID
        assert f(ok(), 4, BW, BH, k, None, None, Wv) == INVALID
        assert f(ok(), 4, BW, BH, k, None, G, None) == INVALID
        assert f(ok(), 0, BW, BH, k, None, G, Wv) == INVALID
        assert f(ok(n_frames=0), 4, BW, BH, k, None, G, Wv) == INVALID
        assert f(ok(flags=0x2), 4, BW, BH, k, None, G, Wv) == INVALID
        assert f(ok(dims=N.mh_dims(16, 16, 3, 2)), 4, 1, 1, k, None, G, Wv) == DIMS
        for size in ((0, 8), (8, 0), (257, 8), (8, 193), (0xFFFFFFFF, 1)):
            assert f(ok(), 4, size[0], size[1], k, None, G, Wv) == DIMS, size
    assert f(ok(), 4, BW, BH, 4, None, G, Wv) == INVALID
    assert f(ok(dims=N.mh_dims(16, 16, 3, 2)), 4, 1, 1, 4, None, G, Wv) == INVALID      # before dims
    assert f(ok(), 4, 257, 8, 0xFFFFFFFF, None, G, Wv) == INVALID


# ---- the Python wrappers -----------------------------------------------------------------------------

W, H = 597, 67   # 75 x 9 blocks


def _host_frames(n=3):
    """A DeviceFrames description with host tensors: the wrappers validate the scale, the size and a
    host list before they look at a buffer."""
    import torch
    from metalhuffman_amd import decoder as D
    z = torch.zeros(16, dtype=torch.uint8)
    return D.DeviceFrames(W, H, n, torch.zeros(4, dtype=torch.int32), z, None)


@pytest.mark.parametrize("bad", [-1, 4, 1.5, 8])
def test_decode_windows_scaled_rejects_bad_scales(bad):
    from metalhuffman_amd import decoder as D
    with pytest.raises(ValueError, match="log2_scale"):
        D.decode_windows_scaled(_host_frames(), None, [(0, 0, 0)], (10, 3), bad)
    with pytest.raises(ValueError, match="log2_scale"):
        D.decode_windows_scaled_shape(_host_frames(), 1, (10, 3), bad)


@pytest.mark.parametrize("k", (0,) + KS)
@pytest.mark.parametrize("size", [(0, 3), (10, 0), (76, 3), (10, 10), (-1, 3)])
def test_decode_windows_scaled_rejects_bad_sizes(size, k):
    from metalhuffman_amd import decoder as D
    with pytest.raises(ValueError, match="does not fit"):
        D.decode_windows_scaled(_host_frames(), None, [(0, 0, 0)], size, k)
    with pytest.raises(ValueError, match="does not fit"):
        D.decode_windows_scaled_shape(_host_frames(), 1, size, k)


@pytest.mark.parametrize("k", (0,) + KS)
@pytest.mark.parametrize("windows", [
    [(3, 0, 0)],                    # frame >= n_frames
    [(0, 0, 0), (-1, 0, 0)],
    [(0, 66, 0)],                   # bx0 + bw > 75
    [(0, 0, 7)],                    # by0 + bh > 9
    [(0, 0xFFFFFFFF, 0)],
    [(0, 0, 0, 0)],                 # a host list is (frame, bx0, by0)
    [],
    [(0.5, 0, 0)],
])
def test_decode_windows_scaled_rejects_bad_host_lists(windows, k):
    from metalhuffman_amd import decoder as D
    with pytest.raises(ValueError, match="window"):
        D.decode_windows_scaled(_host_frames(), None, windows, (10, 3), k)


def test_decode_windows_scaled_accepts_good_host_lists_and_counts():
    """Windows at the grid's corners get past the list's validation: the call ends at the next check
    (the buffers are host tensors). No windows is a ValueError of the shape wrapper."""
    from metalhuffman_amd import decoder as D
    good = [(0, 0, 0), (2, 65, 6), (1, 65, 0), (0, 0, 6)]
    for k in (0,) + KS:
        with pytest.raises(ValueError, match="HIP device"):
            D.decode_windows_scaled(_host_frames(), None, good, (10, 3), k)
    assert "dx[i] // s" in D.decode_windows_scaled.__doc__ and "multiples of s" in D.decode_windows_scaled.__doc__
