"""The C-ABI of the crops entries (include/metalhuffman.h: mh_decode_crops, mh_decode_crops_shape):
exported, the descriptor's layout, and every host check made before any HIP call, with fake
pointers, in mh_decode_windows' order; decode_crops' validation of a host list. CPU only. (The crops
themselves live in device memory and are judged by the kernel: tests/test_gpu_crops.py.)"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

INVALID, DIMS, CAPACITY, ALIGN, HIP = -1, -2, -4, -6, -7
LUTS, OUT, CROPS, FSTATUS, CSTATUS = 0x60000, 0x50000, 0x90000, 0xA0000, 0xB0000
CW, CH = 250, 190                     # the default crop size, pixels (w % 8 != 0)
PITCH, CSTRIDE = 256, 256 * CH


def _frame(**kw):
    """A frame mh_decode_crops accepts: 2045 x 1531 (256 x 192 blocks), the table fields NULL / 0."""
    from metalhuffman_amd import _native as N
    fr = N.mh_frame()
    fr.d_block_offsets = 0x10000
    fr.d_codes = 0x20000
    fr.codes_bytes = 4096
    fr.dims = N.mh_dims(2045, 1531, 256, 192)
    fr.n_frames = 1
    for k, v in kw.items():
        setattr(fr, k, v)
    return fr


def _stride(mh):
    return (int(mh.lib().mh_lut_bytes()) + 15) // 16 * 16


def _call(mh, fr=None, crops=CROPS, n=4, size=(CW, CH), luts=LUTS, stride=None, fstatus=None, cstatus=None,
          out=OUT, pitch=PITCH, cstride=CSTRIDE):
    """mh_decode_crops with defaults that pass every check; the callers that must not reach a launch
    stop it with codes_bytes = 2 (SHORT), the last-but-one capacity rule."""
    from metalhuffman_amd import _native as N
    fr = _frame() if fr is None else fr
    return N.lib().mh_decode_crops(ctypes.byref(fr) if fr is not False else None, crops, n, size[0], size[1],
                                   luts, _stride(mh) if stride is None else stride, fstatus, cstatus, out, pitch,
                                   cstride, None)


SHORT = dict(codes_bytes=2)


def _short(**kw):
    return _frame(**dict(SHORT, **kw))


def test_crops_symbols_exported(mh):
    lib = ctypes.CDLL(mh.LIB_PATH)
    for name in ("mh_decode_crops", "mh_decode_crops_shape"):
        assert hasattr(lib, name), name
        assert name in mh.EXPORTS, name
    from metalhuffman_amd import _native as N
    assert ctypes.sizeof(N.mh_crop) == 16
    assert [f[0] for f in N.mh_crop._fields_] == ["frame", "x0", "y0", "reserved"]
    assert [getattr(N.mh_crop, f).offset for f in ("frame", "x0", "y0", "reserved")] == [0, 4, 8, 12]
    assert all(f[1] is ctypes.c_uint32 for f in N.mh_crop._fields_)


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
def test_crops_rejects_bad_frames(mh, kw, status):
    assert _call(mh, _frame(**kw)) == status


def test_crops_rejects_bad_arguments(mh):
    """Every host check with its code: mh_decode_windows', n_crops rasters of w x h in the place of
    n_windows rasters of 8 bw x 8 bh."""
    from metalhuffman_amd import _native as N
    st = _stride(mh)
    # MH_ERR_INVALID_ARG
    assert _call(mh, False) == INVALID                                   # NULL frame
    assert _call(mh, out=None) == INVALID
    assert _call(mh, luts=None) == INVALID
    assert _call(mh, crops=None) == INVALID                              # NULL d_crops
    assert _call(mh, n=0) == INVALID                                     # no crops
    assert _call(mh, fstatus=FSTATUS, cstatus=FSTATUS) == INVALID        # the two status arrays alias
    assert _call(mh, _short(), fstatus=FSTATUS, cstatus=CSTATUS) == CAPACITY   # (distinct ones pass)
    assert _call(mh, _short(), cstatus=CSTATUS) == CAPACITY
    # MH_ERR_DIMS: the frame's, then the crop size's -- in PIXELS, against the declared W x H
    assert _call(mh, _short(dims=N.mh_dims(2045, 1531, 255, 192))) == DIMS
    for size in ((0, 1), (1, 0), (0, 0), (2046, 1), (1, 1532), (2048, 1), (1, 1536), (0xFFFFFFFF, 1),
                 (1, 0xFFFFFFFF)):
        assert _call(mh, size=size) == DIMS, size
    for size in ((2045, 1531), (1, 1), (2045, 1), (1, 1531)):            # sizes up to the whole frame are inside:
        assert _call(mh, _short(), size=size, pitch=2044) == ALIGN, size  # they get past the dims check
    # MH_ERR_ALIGN
    assert _call(mh, pitch=PITCH + 4) == ALIGN                           # pitch % 8
    assert _call(mh, pitch=CW) == ALIGN                                  # w itself, not a multiple of 8
    assert _call(mh, out=OUT + 4) == ALIGN                               # d_out % 8
    assert _call(mh, cstride=CSTRIDE + 4) == ALIGN                       # crop stride % 8 (n_crops > 1)
    assert _call(mh, crops=CROPS + 8) == ALIGN                           # d_crops % 16
    assert _call(mh, crops=CROPS + 4) == ALIGN
    assert _call(mh, luts=LUTS + 8) == ALIGN                             # d_luts % 16
    assert _call(mh, stride=st + 8) == ALIGN                             # table stride % 16
    assert _call(mh, stride=8) == ALIGN
    # MH_ERR_CAPACITY
    assert _call(mh, pitch=PITCH - 8) == CAPACITY                        # pitch 248 < w = 250
    assert _call(mh, pitch=(1 << 20) + 8) == CAPACITY
    assert _call(mh, cstride=CSTRIDE - 8) == CAPACITY                    # crop slots overlap
    assert _call(mh, cstride=0) == CAPACITY
    assert _call(mh, pitch=PITCH + 8, cstride=CSTRIDE) == CAPACITY       # the stride follows the pitch
    assert _call(mh, _short()) == CAPACITY                               # codes_bytes < MH_CODES_PAD
    assert _call(mh, stride=st - 16) == CAPACITY                         # 0 < table stride < mh_lut_bytes()
    assert _call(mh, stride=16) == CAPACITY
    # the slot is w x h exactly: h rows, not the block rows the crop touches
    assert _call(mh, _short(), size=(CW, 3), cstride=PITCH * 3) == CAPACITY   # (passes the stride rule)
    assert _call(mh, size=(CW, 3), cstride=PITCH * 2) == CAPACITY
    # the whole frame's width, 2045, needs a pitch of 2048
    assert _call(mh, size=(2045, 1), pitch=2040, cstride=2048) == CAPACITY


def test_crops_check_order(mh):
    """Invalid argument before dims, dims before alignment, alignment before capacity
    (mh_decode_windows' order); the crop size counts as dims, the descriptor array's alignment as
    alignment."""
    from metalhuffman_amd import _native as N
    st = _stride(mh)
    bad_dims = _frame(dims=N.mh_dims(2045, 1531, 255, 192))
    assert _call(mh, _frame(flags=0x8), size=(2046, 1)) == INVALID
    assert _call(mh, bad_dims, crops=None) == INVALID
    assert _call(mh, bad_dims, n=0) == INVALID
    assert _call(mh, size=(0, 1), fstatus=FSTATUS, cstatus=FSTATUS) == INVALID
    assert _call(mh, bad_dims, crops=CROPS + 8, stride=st - 16, pitch=252) == DIMS
    assert _call(mh, size=(2046, 24), crops=CROPS + 8, luts=LUTS + 8, stride=st - 16, pitch=252) == DIMS
    assert _call(mh, crops=CROPS + 8, stride=st - 16, pitch=PITCH - 8) == ALIGN
    assert _call(mh, luts=LUTS + 8, pitch=PITCH - 8) == ALIGN
    assert _call(mh, cstride=CSTRIDE - 4) == ALIGN                       # misaligned AND too small
    assert _call(mh, stride=8, cstride=0) == ALIGN
    assert _call(mh, _short(), stride=st - 16, pitch=PITCH - 8) == CAPACITY


def test_crops_accepted_calls_reach_the_device(mh):
    """Every capacity rule answers MH_ERR_CAPACITY, so "passed the checks" shows only in a call that
    passes them all: without a HIP device such a call ends in MH_ERR_HIP (the first HIP call finds no
    device). With a device the fake pointers must not be launched on; there tests/test_gpu_crops.py
    makes the same calls with real buffers."""
    from metalhuffman_amd import _native as N
    assert _call(mh, stride=16) == CAPACITY and _call(mh, pitch=PITCH - 8) == CAPACITY
    if N.lib().mh_device_count() > 0:
        return
    assert _call(mh) == HIP
    assert _call(mh, stride=0) == HIP                                     # the shared table
    assert _call(mh, fstatus=FSTATUS, cstatus=CSTATUS) == HIP
    assert _call(mh, n=1, cstride=0) == HIP and _call(mh, n=1, cstride=12) == HIP   # one crop: no stride rule
    assert _call(mh, pitch=PITCH + 8, cstride=(PITCH + 8) * CH) == HIP
    assert _call(mh, size=(2045, 1531), pitch=2048, cstride=2048 * 1531) == HIP     # the whole frame
    assert _call(mh, size=(1, 1), pitch=8, cstride=8) == HIP
    two = _frame(n_frames=2, d_frame_code_offsets=0x80000)
    assert _call(mh, two, n=1000) == HIP                                  # more crops than frames
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    assert N.lib().mh_decode_crops_shape(ctypes.byref(_frame()), 4, CW, CH, None, ctypes.byref(g),
                                         ctypes.byref(w)) == HIP


def test_crops_tile_capacity(mh):
    """More than 2^31 - 1 tiles: a crop of 65535 x 65535 pixels is 8192 words per row = 131 tiles of 63
    words, times (65535 + 14) / 8 = 8193 block rows -- counted over the CROPS, whatever n_frames is."""
    from metalhuffman_amd import _native as N
    tiles = 131 * 8193
    most = (2 ** 31 - 1) // tiles
    big = lambda n: _frame(dims=N.mh_dims(65535, 65535, 8192, 8192), n_frames=n, d_frame_code_offsets=0x80000)
    full = dict(size=(65535, 65535), pitch=65536, cstride=65536 * 65535)
    assert _call(mh, big(1), n=most + 1, **full) == CAPACITY
    assert _call(mh, big(4096), n=most + 1, **full) == CAPACITY
    row = dict(size=(65535, 1), pitch=65536, cstride=65536)              # 131 tiles per crop (CBH = 1)
    assert _call(mh, big(2), n=(2 ** 31 - 1) // 131 + 1, **row) == CAPACITY
    L = N.lib()
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.mh_decode_crops_shape(ctypes.byref(big(1)), most + 1, 65535, 65535, None, ctypes.byref(g),
                                   ctypes.byref(w)) == CAPACITY
    if L.mh_device_count() == 0:   # (accepted: MH_ERR_HIP without a device, see above)
        assert _call(mh, big(1), n=most, **full) == HIP
        assert _call(mh, big(1 << 24), n=4, **row) == HIP                 # tiles over the FRAMES do not count
        assert _call(mh, big(2), n=(2 ** 31 - 1) // 131, **row) == HIP


def test_crops_shape_rejects_bad_arguments(mh):
    from metalhuffman_amd import _native as N
    L = N.lib()
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    G, Wv = ctypes.byref(g), ctypes.byref(w)
    ok = lambda **kw: ctypes.byref(_frame(**kw))
    assert L.mh_decode_crops_shape(None, 4, CW, CH, None, G, Wv) == INVALID
    assert L.mh_decode_crops_shape(ok(), 4, CW, CH, None, None, Wv) == INVALID
    assert L.mh_decode_crops_shape(ok(), 4, CW, CH, None, G, None) == INVALID
    assert L.mh_decode_crops_shape(ok(), 0, CW, CH, None, G, Wv) == INVALID
    assert L.mh_decode_crops_shape(ok(n_frames=0), 4, CW, CH, None, G, Wv) == INVALID
    assert L.mh_decode_crops_shape(ok(flags=0x2), 4, CW, CH, None, G, Wv) == INVALID
    assert L.mh_decode_crops_shape(ok(dims=N.mh_dims(16, 16, 3, 2)), 4, 1, 1, None, G, Wv) == DIMS
    for size in ((0, 8), (8, 0), (2046, 8), (8, 1532), (0xFFFFFFFF, 1)):
        assert L.mh_decode_crops_shape(ok(), 4, size[0], size[1], None, G, Wv) == DIMS, size


# ---- decode_crops' validation of a host list --------------------------------------------------------

W, H = 597, 67   # 75 x 9 blocks, partial right and bottom blocks


def _host_frames(n=3):
    """A DeviceFrames description with host tensors: decode_crops validates the size and a host list
    before it looks at a buffer, so these calls end in the ValueError under test (or, for a valid list,
    in the ValueError that the buffers are not on a HIP device)."""
    import torch
    from metalhuffman_amd import decoder as D
    z = torch.zeros(16, dtype=torch.uint8)
    return D.DeviceFrames(W, H, n, torch.zeros(4, dtype=torch.int32), z, None)


@pytest.mark.parametrize("crops,size", [
    ([(3, 0, 0)], (80, 24)),                   # frame >= n_frames
    ([(0, 0, 0), (-1, 0, 0)], (80, 24)),
    ([(0, 518, 0)], (80, 24)),                 # x0 + w > 597
    ([(0, 0, 44)], (80, 24)),                  # y0 + h > 67
    ([(0, -1, 0)], (80, 24)),
    ([(0, 0, -1)], (80, 24)),
    ([(0, 0xFFFFFFFF, 0)], (80, 24)),
    ([(0, 1, 0)], (597, 67)),
    ([(0, 0, 0, 0)], (80, 24)),                # a host list is (frame, x0, y0)
    ([], (80, 24)),
    ([(0.5, 0, 0)], (80, 24)),
])
def test_decode_crops_rejects_bad_host_lists(crops, size):
    from metalhuffman_amd import decoder as D
    with pytest.raises(ValueError, match="crop"):
        D.decode_crops(_host_frames(), None, crops, size)
    with pytest.raises(ValueError, match="crop"):
        D.decode_crops(_host_frames(), None, np.asarray(crops), size)


@pytest.mark.parametrize("size", [(0, 3), (10, 0), (598, 3), (10, 68), (-1, 3)])
def test_decode_crops_rejects_bad_sizes(size):
    from metalhuffman_amd import decoder as D
    with pytest.raises(ValueError, match="does not fit"):
        D.decode_crops(_host_frames(), None, [(0, 0, 0)], size)
    with pytest.raises(ValueError, match="does not fit"):
        D.decode_crops_shape(_host_frames(), 1, size)


def test_decode_crops_accepts_good_host_lists():
    """The same call with crops at the frame's corners gets past the list's validation: it ends at the
    next check (the buffers are host tensors)."""
    from metalhuffman_amd import decoder as D
    good = [(0, 0, 0), (2, 517, 43), (1, 517, 0), (0, 0, 43)]
    assert D._host_crops(_host_frames(), good, 80, 24).tolist() == [list(g) + [0] for g in good]
    assert D._host_crops(_host_frames(), good, 80, 24).dtype == np.int32
    with pytest.raises(ValueError, match="HIP device"):
        D.decode_crops(_host_frames(), None, good, (80, 24))
