"""The C-ABI of the normalised-crops entries (include/metalhuffman.h: mh_decode_crops_norm,
mh_decode_crops_norm_shape): exported, the descriptor's layout, and every host check made before any
HIP call, with fake pointers, in mh_decode_crops' order; decode_crops_normalized's validation of a
host list. CPU only. (The crops themselves live in device memory and are judged by the kernel:
tests/test_gpu_crops_norm.py.)"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

INVALID, DIMS, CAPACITY, ALIGN, HIP = -1, -2, -4, -6, -7
LUTS, OUT, CROPS, FSTATUS, CSTATUS = 0x60000, 0x50000, 0x90000, 0xA0000, 0xB0000
CW, CH = 250, 190                     # the default crop size, pixels (w % 8 != 0): 256 elements per row
F16, BF16, F32 = 0, 1, 2
ESIZE = {F16: 2, BF16: 2, F32: 4}
NAN, INF = float("nan"), float("inf")


def _frame(**kw):
    """A frame mh_decode_crops_norm accepts: 2045 x 1531 (256 x 192 blocks), the table fields NULL / 0."""
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


def _call(mh, fr=None, crops=CROPS, n=4, size=(CW, CH), fmt=F16, scale=1.0, bias=0.0, luts=LUTS, stride=None,
          fstatus=None, cstatus=None, out=OUT, pitch=None, cstride=None):
    """mh_decode_crops_norm with defaults that pass every check (pitch: round_up(w, 8) elements; the
    stride: h rows); the callers that must not reach a launch stop it with codes_bytes = 2 (SHORT)."""
    from metalhuffman_amd import _native as N
    fr = _frame() if fr is None else fr
    pitch = (size[0] + 7) // 8 * 8 * ESIZE.get(fmt, 2) if pitch is None else pitch
    cstride = pitch * size[1] if cstride is None else cstride
    return N.lib().mh_decode_crops_norm(ctypes.byref(fr) if fr is not False else None, crops, n, size[0], size[1],
                                        fmt, scale, bias, luts, _stride(mh) if stride is None else stride, fstatus,
                                        cstatus, out, pitch, cstride, None)


SHORT = dict(codes_bytes=2)


def _short(**kw):
    return _frame(**dict(SHORT, **kw))


def test_norm_symbols_exported(mh):
    lib = ctypes.CDLL(mh.LIB_PATH)
    for name in ("mh_decode_crops_norm", "mh_decode_crops_norm_shape", "mh_norm_table"):
        assert hasattr(lib, name), name
        assert name in mh.EXPORTS, name
    from metalhuffman_amd import _native as N
    assert ctypes.sizeof(N.mh_norm_crop) == 16
    assert [f[0] for f in N.mh_norm_crop._fields_] == ["frame", "x0", "y0", "flags"]
    assert [getattr(N.mh_norm_crop, f).offset for f in ("frame", "x0", "y0", "flags")] == [0, 4, 8, 12]
    assert all(f[1] is ctypes.c_uint32 for f in N.mh_norm_crop._fields_)
    assert (N.MH_NORM_F16, N.MH_NORM_BF16, N.MH_NORM_F32, N.MH_CROP_MIRROR) == (0, 1, 2, 1)
    assert (mh.MH_NORM_F16, mh.MH_NORM_BF16, mh.MH_NORM_F32, mh.MH_CROP_MIRROR) == (0, 1, 2, 1)
    # the byte entry is as it was
    assert [f[0] for f in N.mh_crop._fields_] == ["frame", "x0", "y0", "reserved"]


def test_norm_header_declares_the_entries():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "metalhuffman.h")).read()
    for piece in ("#define MH_NORM_F16 0u", "#define MH_NORM_BF16 1u", "#define MH_NORM_F32 2u",
                  "#define MH_CROP_MIRROR 0x1u", "uint32_t frame, x0, y0, flags;", "} mh_norm_crop;",
                  "int mh_decode_crops_norm(const mh_frame *frame, const mh_norm_crop *d_crops, uint32_t n_crops,",
                  "int mh_decode_crops_norm_shape(const mh_frame *frame, uint32_t n_crops, uint32_t w, uint32_t h,",
                  "int mh_norm_table(uint32_t format, float scale, float bias, void *table, size_t table_bytes);"):
        assert piece in text, piece


@pytest.mark.parametrize("fmt", [F16, BF16, F32])
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
def test_norm_rejects_bad_frames(mh, kw, status, fmt):
    assert _call(mh, _frame(**kw), fmt=fmt) == status


@pytest.mark.parametrize("fmt", [F16, BF16, F32])
def test_norm_rejects_bad_arguments(mh, fmt):
    """Every host check with its code: mh_decode_crops', with E-byte elements, 16-byte stores, and the
    format and the map checked where a bad flag is."""
    from metalhuffman_amd import _native as N
    st = _stride(mh)
    E = ESIZE[fmt]
    pitch, call = 256 * E, lambda *a, **kw: _call(mh, *a, fmt=fmt, **kw)
    cstride = pitch * CH
    # MH_ERR_INVALID_ARG
    assert call(False) == INVALID                                        # NULL frame
    assert call(out=None) == INVALID
    assert call(luts=None) == INVALID
    assert call(crops=None) == INVALID                                   # NULL d_crops
    assert call(n=0) == INVALID                                          # no crops
    assert call(fstatus=FSTATUS, cstatus=FSTATUS) == INVALID             # the two status arrays alias
    assert call(_short(), fstatus=FSTATUS, cstatus=CSTATUS) == CAPACITY  # (distinct ones pass)
    assert _call(mh, fmt=3) == INVALID and _call(mh, fmt=0xFFFFFFFF) == INVALID and _call(mh, _short(), fmt=3) == INVALID
    for bad in (NAN, INF, -INF):
        assert call(scale=bad) == INVALID and call(bias=bad) == INVALID and call(_short(), scale=bad) == INVALID
    assert call(_short(), scale=3.0e38, bias=-3.0e38) == CAPACITY        # (large and finite pass)
    assert call(_short(), scale=0.0, bias=0.0) == CAPACITY
    # MH_ERR_DIMS: the frame's, then the crop size's -- in PIXELS, against the declared W x H
    assert call(_short(dims=N.mh_dims(2045, 1531, 255, 192))) == DIMS
    for size in ((0, 1), (1, 0), (0, 0), (2046, 1), (1, 1532), (2048, 1), (1, 1536), (0xFFFFFFFF, 1),
                 (1, 0xFFFFFFFF)):
        assert call(size=size) == DIMS, size
    for size in ((2045, 1531), (1, 1), (2045, 1), (1, 1531)):            # sizes up to the whole frame are inside:
        assert call(_short(), size=size, pitch=2040) == ALIGN, size      # they get past the dims check
    # MH_ERR_ALIGN: 16 bytes, the row store
    assert call(pitch=pitch + 8) == ALIGN and call(pitch=pitch + 4) == ALIGN
    assert call(out=OUT + 8) == ALIGN and call(out=OUT + 4) == ALIGN
    assert call(cstride=cstride + 8) == ALIGN                            # crop stride % 16 (n_crops > 1)
    assert call(crops=CROPS + 8) == ALIGN                                # d_crops % 16
    assert call(luts=LUTS + 8) == ALIGN                                  # d_luts % 16
    assert call(stride=st + 8) == ALIGN and call(stride=8) == ALIGN      # table stride % 16
    # MH_ERR_CAPACITY
    assert call(pitch=pitch - 16) == CAPACITY                            # below w * E
    assert call(size=(256, CH), pitch=256 * E - 16, cstride=cstride) == CAPACITY   # w * E - 16, w % 8 == 0
    assert call(pitch=(1 << 20) + 16) == CAPACITY
    assert call(_short(), pitch=1 << 20, cstride=(1 << 20) * CH) == CAPACITY       # (2^20 itself passes)
    assert call(cstride=cstride - 16) == CAPACITY                        # crop slots overlap
    assert call(cstride=0) == CAPACITY
    assert call(pitch=pitch + 16, cstride=cstride) == CAPACITY           # the stride follows the pitch
    assert call(_short()) == CAPACITY                                    # codes_bytes < MH_CODES_PAD
    assert call(stride=st - 16) == CAPACITY and call(stride=16) == CAPACITY   # 0 < table stride < mh_lut_bytes()
    assert call(_short(), size=(CW, 3), cstride=pitch * 3) == CAPACITY   # (passes the stride rule)
    assert call(size=(CW, 3), cstride=pitch * 2) == CAPACITY             # the slot is h rows
    # the whole frame's width, 2045, needs 2048 elements
    assert call(size=(2045, 1), pitch=2048 * E - 16, cstride=2048 * E) == CAPACITY
    # the widest crop's row, 65536 elements of 4 bytes, is inside the pitch cap
    big = _frame(dims=N.mh_dims(65535, 8, 8192, 1), codes_bytes=2)
    assert call(big, size=(65535, 1), n=1, pitch=65536 * E) == CAPACITY
    assert call(big, size=(65535, 1), n=1, pitch=65536 * E - 16) == CAPACITY


def test_norm_pitch_holds_the_written_row(mh):
    """A row is written with round_up(w, 8) elements. At 2 bytes every multiple of 16 that is >= 2 w
    holds them; at 4 bytes the least aligned pitch >= 4 w does not when w % 8 is 1..4 -- the row's
    last store would run into the next row -- and is refused. (Accepted shows as MH_ERR_HIP, so the
    accepted half needs a machine without a device.)"""
    from metalhuffman_amd import _native as N
    no_device = N.lib().mh_device_count() == 0
    for w in range(1, 18):
        for fmt in (F16, BF16, F32):
            E = ESIZE[fmt]
            least = (w * E + 15) // 16 * 16                  # the least aligned pitch >= w * E
            row = (w + 7) // 8 * 8 * E
            assert (least < row) == (E == 4 and 1 <= w % 8 <= 4)
            if least < row:
                assert row - least == 16
                assert _call(mh, size=(w, 4), fmt=fmt, n=1, pitch=least) == CAPACITY
            elif no_device:
                assert _call(mh, size=(w, 4), fmt=fmt, n=1, pitch=least) == HIP
            assert _call(mh, size=(w, 4), fmt=fmt, n=1, pitch=row - 16) == CAPACITY
            if no_device:
                assert _call(mh, size=(w, 4), fmt=fmt, n=1, pitch=row) == HIP


def test_norm_check_order(mh):
    """Invalid argument (the format and the map with the flags) before dims, dims before alignment,
    alignment before capacity."""
    from metalhuffman_amd import _native as N
    st = _stride(mh)
    bad_dims = _frame(dims=N.mh_dims(2045, 1531, 255, 192))
    assert _call(mh, _frame(flags=0x8), size=(2046, 1)) == INVALID
    assert _call(mh, bad_dims, fmt=3) == INVALID and _call(mh, bad_dims, scale=NAN) == INVALID
    assert _call(mh, size=(0, 1), bias=INF) == INVALID and _call(mh, size=(0, 1), fmt=7, out=OUT + 8) == INVALID
    assert _call(mh, bad_dims, crops=None) == INVALID
    assert _call(mh, bad_dims, n=0) == INVALID
    assert _call(mh, size=(0, 1), fstatus=FSTATUS, cstatus=FSTATUS) == INVALID
    assert _call(mh, bad_dims, crops=CROPS + 8, stride=st - 16, pitch=504) == DIMS
    assert _call(mh, size=(2046, 24), crops=CROPS + 8, luts=LUTS + 8, stride=st - 16, pitch=504) == DIMS
    assert _call(mh, crops=CROPS + 8, stride=st - 16, pitch=512 - 16) == ALIGN
    assert _call(mh, luts=LUTS + 8, pitch=512 - 16) == ALIGN
    assert _call(mh, cstride=512 * CH - 8) == ALIGN                      # misaligned AND too small
    assert _call(mh, stride=8, cstride=0) == ALIGN
    assert _call(mh, _short(), stride=st - 16, pitch=512 - 16) == CAPACITY


def test_norm_accepted_calls_reach_the_device(mh):
    """Without a HIP device a call that passes every check ends in MH_ERR_HIP (the first HIP call finds
    no device). With a device the fake pointers must not be launched on; there
    tests/test_gpu_crops_norm.py makes the same calls with real buffers."""
    from metalhuffman_amd import _native as N
    assert _call(mh, stride=16) == CAPACITY
    if N.lib().mh_device_count() > 0:
        return
    for fmt in (F16, BF16, F32):
        E = ESIZE[fmt]
        assert _call(mh, fmt=fmt) == HIP
        assert _call(mh, fmt=fmt, stride=0) == HIP                        # the shared table
        assert _call(mh, fmt=fmt, fstatus=FSTATUS, cstatus=CSTATUS) == HIP
        assert _call(mh, fmt=fmt, n=1, cstride=0) == HIP and _call(mh, fmt=fmt, n=1, cstride=8) == HIP
        assert _call(mh, fmt=fmt, pitch=256 * E + 48, cstride=(256 * E + 48) * CH + 80) == HIP
        assert _call(mh, fmt=fmt, size=(2045, 1531)) == HIP               # the whole frame
        assert _call(mh, fmt=fmt, size=(1, 1), pitch=8 * E, cstride=8 * E) == HIP
        assert _call(mh, fmt=fmt, scale=-3.0e38, bias=1.0e-45) == HIP
        g, w = ctypes.c_uint32(), ctypes.c_uint32()
        assert N.lib().mh_decode_crops_norm_shape(ctypes.byref(_frame()), 4, CW, CH, fmt, None, ctypes.byref(g),
                                                  ctypes.byref(w)) == HIP
    two = _frame(n_frames=2, d_frame_code_offsets=0x80000)
    assert _call(mh, two, n=1000) == HIP                                  # more crops than frames


def test_norm_tile_capacity(mh):
    """The tile cap is mh_decode_crops': counted over the CROPS, 131 tiles x 8193 block rows for a crop
    of 65535 x 65535."""
    from metalhuffman_amd import _native as N
    tiles = 131 * 8193
    most = (2 ** 31 - 1) // tiles
    big = lambda n: _frame(dims=N.mh_dims(65535, 65535, 8192, 8192), n_frames=n, d_frame_code_offsets=0x80000)
    assert _call(mh, big(1), n=most + 1, size=(65535, 65535), fmt=F32) == CAPACITY
    L = N.lib()
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    assert L.mh_decode_crops_norm_shape(ctypes.byref(big(1)), most + 1, 65535, 65535, F16, None, ctypes.byref(g),
                                        ctypes.byref(w)) == CAPACITY
    if L.mh_device_count() == 0:
        assert _call(mh, big(1), n=most, size=(65535, 65535), fmt=F32) == HIP


def test_norm_shape_rejects_bad_arguments(mh):
    from metalhuffman_amd import _native as N
    L = N.lib()
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    G, Wv = ctypes.byref(g), ctypes.byref(w)
    ok = lambda **kw: ctypes.byref(_frame(**kw))
    shape = L.mh_decode_crops_norm_shape
    assert shape(None, 4, CW, CH, F16, None, G, Wv) == INVALID
    assert shape(ok(), 4, CW, CH, F16, None, None, Wv) == INVALID
    assert shape(ok(), 4, CW, CH, F16, None, G, None) == INVALID
    assert shape(ok(), 0, CW, CH, F16, None, G, Wv) == INVALID
    assert shape(ok(n_frames=0), 4, CW, CH, F16, None, G, Wv) == INVALID
    assert shape(ok(flags=0x2), 4, CW, CH, F16, None, G, Wv) == INVALID
    assert shape(ok(), 4, CW, CH, 3, None, G, Wv) == INVALID
    assert shape(ok(), 4, 0, CH, 3, None, G, Wv) == INVALID              # the format before the dims
    assert shape(ok(dims=N.mh_dims(16, 16, 3, 2)), 4, 1, 1, F32, None, G, Wv) == DIMS
    for size in ((0, 8), (8, 0), (2046, 8), (8, 1532), (0xFFFFFFFF, 1)):
        assert shape(ok(), 4, size[0], size[1], BF16, None, G, Wv) == DIMS, size


# ---- decode_crops_normalized's validation of a host list ------------------------------------------------

W, H = 597, 67   # 75 x 9 blocks, partial right and bottom blocks


def _host_frames(n=3):
    """A DeviceFrames description with host tensors: the size, the format, the map and a host list are
    validated before a buffer is looked at, so these calls end in the ValueError under test (or, for
    a valid list, in the ValueError that the buffers are not on a HIP device)."""
    import torch
    from metalhuffman_amd import decoder as D
    z = torch.zeros(16, dtype=torch.uint8)
    return D.DeviceFrames(W, H, n, torch.zeros(4, dtype=torch.int32), z, None)


@pytest.mark.parametrize("crops,size", [
    ([(3, 0, 0)], (80, 24)),                   # frame >= n_frames
    ([(0, 0, 0), (-1, 0, 0)], (80, 24)),
    ([(0, 518, 0)], (80, 24)),                 # x0 + w > 597
    ([(0, 518, 0, 1)], (80, 24)),
    ([(0, 0, 44)], (80, 24)),                  # y0 + h > 67
    ([(0, -1, 0)], (80, 24)),
    ([(0, 0xFFFFFFFF, 0, 0)], (80, 24)),
    ([(0, 1, 0)], (597, 67)),
    ([(0, 0, 0, 2)], (80, 24)),                # an unknown flag bit
    ([(0, 0, 0, 1), (0, 0, 0, 3)], (80, 24)),
    ([(0, 0, 0, 0x80000001)], (80, 24)),
    ([(0, 0, 0, -1)], (80, 24)),
    ([(0, 0, 0, 1)], (19, 13)),                # mirrored, w % 8 != 0
    ([(0, 0, 0, 0), (1, 5, 5, 1)], (81, 24)),
    ([(0, 0, 0, 0, 0)], (80, 24)),             # five columns
    ([], (80, 24)),
    ([(0.5, 0, 0)], (80, 24)),
])
def test_decode_crops_normalized_rejects_bad_host_lists(crops, size):
    import torch
    from metalhuffman_amd import decoder as D
    with pytest.raises(ValueError, match="crop"):
        D.decode_crops_normalized(_host_frames(), None, crops, size, torch.float16)
    with pytest.raises(ValueError, match="crop"):
        D.decode_crops_normalized(_host_frames(), None, np.asarray(crops), size, torch.float32, 1 / 255.0, -0.5)


@pytest.mark.parametrize("size", [(0, 3), (10, 0), (598, 3), (10, 68), (-1, 3)])
def test_decode_crops_normalized_rejects_bad_sizes(size):
    import torch
    from metalhuffman_amd import decoder as D
    with pytest.raises(ValueError, match="does not fit"):
        D.decode_crops_normalized(_host_frames(), None, [(0, 0, 0)], size, torch.bfloat16)
    with pytest.raises(ValueError, match="does not fit"):
        D.decode_crops_normalized_shape(_host_frames(), 1, size, torch.bfloat16)


def test_decode_crops_normalized_rejects_bad_formats_and_maps():
    import torch
    from metalhuffman_amd import decoder as D
    for bad in (torch.uint8, torch.float64, "int8", 3, None):
        with pytest.raises(ValueError, match="format"):
            D.decode_crops_normalized(_host_frames(), None, [(0, 0, 0)], (80, 24), bad)
        with pytest.raises(ValueError, match="format"):
            D.decode_crops_normalized_shape(_host_frames(), 1, (80, 24), bad)
    for bad in (NAN, INF, -INF, 1e39):
        with pytest.raises(ValueError, match="finite"):
            D.decode_crops_normalized(_host_frames(), None, [(0, 0, 0)], (80, 24), torch.float16, scale=bad)
        with pytest.raises(ValueError, match="finite"):
            D.decode_crops_normalized(_host_frames(), None, [(0, 0, 0)], (80, 24), torch.float16, bias=bad)


def test_decode_crops_normalized_accepts_good_host_lists():
    """Crops at the frame's corners, mirrored and not, get past the list's validation: the call ends at
    the next check (the buffers are host tensors)."""
    import torch
    from metalhuffman_amd import decoder as D
    good = [(0, 0, 0, 0), (2, 517, 43, 1), (1, 517, 0, 0), (0, 0, 43, 1)]
    assert D._host_norm_crops(_host_frames(), good, 80, 24).tolist() == [list(g) for g in good]
    assert D._host_norm_crops(_host_frames(), good, 80, 24).dtype == np.int32
    three = [g[:3] for g in good]
    assert D._host_norm_crops(_host_frames(), three, 19, 13).tolist() == [list(g) + [0] for g in three]
    assert D._host_norm_crops(_host_frames(), [g[:3] + (0,) for g in good], 19, 13)[:, 3].tolist() == [0] * 4
    with pytest.raises(ValueError, match="HIP device"):
        D.decode_crops_normalized(_host_frames(), None, good, (80, 24), torch.float16, 1 / 255.0)
    # decode_crops' own list rule is as it was: three columns
    with pytest.raises(ValueError, match="crop"):
        D.decode_crops(_host_frames(), None, good, (80, 24))
