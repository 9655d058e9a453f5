"""The C-ABI of the region entries (include/metalhuffman.h: mh_decode_region,
mh_decode_region_shape): exported, and every argument check made before any HIP call, with fake
pointers; decoder.region_of_rect on edge rectangles. CPU only."""
from __future__ import annotations

import ctypes

import pytest

INVALID, DIMS, CAPACITY, TABLE, ALIGN = -1, -2, -4, -5, -6
LUTS, OUT = 0x60000, 0x50000


def _frame(**kw):
    """A frame mh_decode_region accepts: 2048 x 1536, the table fields NULL / 0 (ignored)."""
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


def _call(mh, fr=None, rg=(16, 8, 32, 24), luts=LUTS, stride=None, out=OUT, pitch=256, fstride=0):
    """mh_decode_region with defaults that pass every check up to the last one; the default call
    itself is stopped by codes_bytes=2 in the callers that must not reach a launch."""
    from metalhuffman_amd import _native as N
    fr = _frame() if fr is None else fr
    return N.lib().mh_decode_region(ctypes.byref(fr) if fr is not False else None,
                                    _region(*rg) if rg is not None else None, luts,
                                    _stride(mh) if stride is None else stride, None, out, pitch, fstride, None)


SHORT = dict(codes_bytes=2)   # fails the LAST-but-one capacity rule: every earlier check was passed


def test_region_symbols_exported(mh):
    lib = ctypes.CDLL(mh.LIB_PATH)
    for name in ("mh_decode_region", "mh_decode_region_shape"):
        assert hasattr(lib, name), name
        assert name in mh.EXPORTS, name
    from metalhuffman_amd import _native as N
    assert ctypes.sizeof(N.mh_region) == 16


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
def test_region_rejects_bad_frames(mh, kw, status):
    assert _call(mh, _frame(**kw)) == status


def test_region_rejects_bad_arguments(mh):
    """mh_decode_frames' checks in its order, RW / RH in the place of W / H."""
    from metalhuffman_amd import _native as N
    st = _stride(mh)
    short = lambda **kw: _frame(**dict(SHORT, **kw))
    assert _call(mh, False) == INVALID                                   # NULL frame
    assert _call(mh, rg=None) == INVALID                                 # NULL region
    assert _call(mh, out=None) == INVALID
    assert _call(mh, luts=None) == INVALID
    bad_dims = lambda: short(dims=N.mh_dims(2048, 1536, 255, 192))
    assert _call(mh, bad_dims()) == DIMS
    # the region's own rules: MH_ERR_DIMS
    for rg in ((0, 0, 0, 1), (0, 0, 1, 0), (0, 0, 257, 1), (1, 0, 256, 1), (0, 0, 1, 193), (0, 192, 1, 1),
               (256, 0, 1, 1), (0xFFFFFFFF, 0, 2, 1), (0, 0xFFFFFFFF, 1, 2), (0xFFFFFFFF, 0, 0xFFFFFFFF, 1),
               (2, 0, 0xFFFFFFFF, 1)):
        assert _call(mh, rg=rg) == DIMS, rg
    for rg in ((0, 0, 256, 192), (255, 191, 1, 1), (0, 0, 1, 1)):       # the grid's corners are inside:
        assert _call(mh, short(), rg=rg, pitch=2044) == ALIGN, rg       # they get past the dims check
    assert _call(mh, pitch=252) == ALIGN                                 # pitch % 8
    assert _call(mh, out=OUT + 4) == ALIGN                               # d_out % 8
    assert _call(mh, luts=LUTS + 8) == ALIGN                             # d_luts % 16
    assert _call(mh, stride=st + 8) == ALIGN                             # stride % 16
    assert _call(mh, stride=8) == ALIGN
    assert _call(mh, stride=st - 16) == CAPACITY                         # 0 < stride < mh_lut_bytes()
    assert _call(mh, stride=16) == CAPACITY
    # (stride 0, the shared table, is accepted: test_region_accepted_calls_reach_the_device)
    # pitch: RW = 8 * 32 = 256 stands where W = 2048 does
    assert _call(mh, pitch=248) == CAPACITY                              # pitch < RW
    assert _call(mh, pitch=(1 << 20) + 8) == CAPACITY
    # the right-edge region of a 2045-wide frame: RW = 2045 - 8 * 224 = 253, so a pitch of 256 holds it
    assert _call(mh, _frame(dims=N.mh_dims(2045, 1531, 256, 192)), rg=(224, 168, 32, 24), pitch=248) == CAPACITY
    two = lambda **kw: _frame(n_frames=2, d_frame_code_offsets=0x80000, **kw)
    assert _call(mh, two(), fstride=256 * 192 + 4) == ALIGN                       # frame stride % 8
    assert _call(mh, two(), fstride=256 * 191) == CAPACITY                        # region rasters overlap (RH = 192)
    # RH of the bottom-edge region of a 1531-high frame is 1531 - 8 * 168 = 187
    e3 = _frame(n_frames=2, d_frame_code_offsets=0x80000, dims=N.mh_dims(2045, 1531, 256, 192))
    assert _call(mh, e3, rg=(224, 168, 32, 24), fstride=256 * 186) == CAPACITY   # overlap


def test_region_accepted_calls_reach_the_device(mh):
    """Every capacity rule answers MH_ERR_CAPACITY, so "passed the check" shows only in a call that
    passes them all: on a machine without a HIP device such a call ends in MH_ERR_HIP (-7, the
    first HIP call finds no device) -- stride 0 (the shared table), and a pitch >= RW that is < W.
    With a device the fake pointers must not be launched on: there test_gpu_region.py makes the
    same calls with real buffers (every shared-table case; the right-edge region's pitch 512 < 597)."""
    from metalhuffman_amd import _native as N
    assert _call(mh, stride=16) == CAPACITY and _call(mh, pitch=248) == CAPACITY
    if N.lib().mh_device_count() > 0:
        return
    HIP = -7
    assert _call(mh, stride=0) == HIP
    assert _call(mh, stride=_stride(mh)) == HIP
    assert _call(mh, pitch=256) == HIP and 256 < 2048                    # RW = 256 <= pitch < W
    edge = _frame(dims=N.mh_dims(2045, 1531, 256, 192))                  # RW = 253, RH = 187
    assert _call(mh, edge, rg=(224, 168, 32, 24), pitch=256) == HIP
    e2 = _frame(n_frames=2, d_frame_code_offsets=0x80000, dims=N.mh_dims(2045, 1531, 256, 192))
    assert _call(mh, e2, rg=(224, 168, 32, 24), fstride=256 * 187) == HIP     # stride >= RH * pitch, < H * pitch
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    assert N.lib().mh_decode_region_shape(ctypes.byref(_frame()), _region(0, 0, 8, 8), None, ctypes.byref(g),
                                          ctypes.byref(w)) == HIP


def test_region_check_order(mh):
    """dims before alignment, alignment before capacity (mh_decode's order); the region's dims
    count as dims."""
    from metalhuffman_amd import _native as N
    st = _stride(mh)
    bad_dims = _frame(dims=N.mh_dims(2048, 1536, 255, 192))
    assert _call(mh, bad_dims, luts=LUTS + 8, stride=st - 16, pitch=252) == DIMS
    assert _call(mh, rg=(250, 0, 32, 24), luts=LUTS + 8, stride=st - 16, pitch=252) == DIMS
    assert _call(mh, luts=LUTS + 8, stride=st - 16, pitch=248) == ALIGN
    assert _call(mh, stride=8, pitch=248) == ALIGN
    assert _call(mh, _frame(flags=0x8), rg=(250, 0, 32, 24)) == INVALID    # invalid argument before dims
    assert _call(mh, _frame(**SHORT), stride=st - 16, pitch=248) == CAPACITY


def test_region_tile_capacity(mh):
    """More than 2^31 - 1 tiles: 8192 x 8192 blocks are 8192 * 128 = 2^20 tiles per frame, so 2048
    frames of the full region are 2^31."""
    from metalhuffman_amd import _native as N
    big = lambda n: _frame(dims=N.mh_dims(65535, 65535, 8192, 8192), n_frames=n, d_frame_code_offsets=0x80000)
    rg = (0, 0, 8192, 8192)
    fs = 65536 * 65535
    assert _call(mh, big(2048), rg=rg, pitch=65536, fstride=fs) == CAPACITY
    # the REGION's tiles count, not the frame's: 2^20 frames of a 128-tile region are 2^27 tiles of 2^40 blocks,
    # and one block row of 8192 blocks (128 tiles) over 2^24 frames is 2^31
    assert _call(mh, big(1 << 24), rg=(0, 7, 8192, 1), pitch=65536, fstride=65536 * 8) == CAPACITY
    if N.lib().mh_device_count() == 0:   # (accepted: MH_ERR_HIP without a device, see above)
        assert _call(mh, big(1 << 20), rg=(0, 7, 8192, 1), pitch=65536, fstride=65536 * 8) == -7
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    L = N.lib()
    assert L.mh_decode_region_shape(ctypes.byref(big(2048)), _region(*rg), None, ctypes.byref(g),
                                    ctypes.byref(w)) == CAPACITY


def test_region_shape_rejects_bad_arguments(mh):
    from metalhuffman_amd import _native as N
    L = N.lib()
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    G, Wv = ctypes.byref(g), ctypes.byref(w)
    ok, rg = lambda **kw: ctypes.byref(_frame(**kw)), _region(0, 0, 8, 8)
    assert L.mh_decode_region_shape(None, rg, None, G, Wv) == INVALID
    assert L.mh_decode_region_shape(ok(), None, None, G, Wv) == INVALID
    assert L.mh_decode_region_shape(ok(), rg, None, None, Wv) == INVALID
    assert L.mh_decode_region_shape(ok(), rg, None, G, None) == INVALID
    assert L.mh_decode_region_shape(ok(n_frames=0), rg, None, G, Wv) == INVALID
    assert L.mh_decode_region_shape(ok(flags=0x2), rg, None, G, Wv) == INVALID
    assert L.mh_decode_region_shape(ok(dims=N.mh_dims(16, 16, 3, 2)), rg, None, G, Wv) == DIMS
    assert L.mh_decode_region_shape(ok(), _region(250, 0, 8, 8), None, G, Wv) == DIMS
    assert L.mh_decode_region_shape(ok(), _region(0xFFFFFFFF, 0, 2, 1), None, G, Wv) == DIMS
    assert L.mh_decode_region_shape(ok(), _region(0, 0, 0, 8), None, G, Wv) == DIMS


def test_decode_frames_stride_zero_still_refused(mh):
    """Only the region entry takes a stride of 0; mh_decode_frames keeps MH_ERR_CAPACITY."""
    from metalhuffman_amd import _native as N
    assert N.lib().mh_decode_frames(ctypes.byref(_frame()), LUTS, 0, None, OUT, 2048, 0, None) == CAPACITY
    assert N.lib().mh_decode_frames(ctypes.byref(_frame()), LUTS, 8, None, OUT, 2048, 0, None) == ALIGN


def test_region_of_rect():
    from metalhuffman_amd.decoder import Region, region_of_rect
    W, H = 597, 67   # 75 x 9 blocks, partial right and bottom blocks
    assert region_of_rect(W, H, 0, 0, W, H) == (Region(0, 0, 75, 9), 0, 0)
    assert region_of_rect(W, H, 0, 0, 1, 1) == (Region(0, 0, 1, 1), 0, 0)
    assert region_of_rect(W, H, 596, 66, 1, 1) == (Region(74, 8, 1, 1), 4, 2)
    assert region_of_rect(W, H, 7, 7, 2, 2) == (Region(0, 0, 2, 2), 7, 7)        # straddles four blocks
    assert region_of_rect(W, H, 8, 16, 8, 8) == (Region(1, 2, 1, 1), 0, 0)       # exactly one block
    assert region_of_rect(W, H, 8, 16, 9, 9) == (Region(1, 2, 2, 2), 0, 0)
    assert region_of_rect(W, H, 29, 13, 300, 41) == (Region(3, 1, 39, 6), 5, 5)
    assert region_of_rect(W, H, 592, 64, 5, 3) == (Region(74, 8, 1, 1), 0, 0)    # the partial corner block
    r, dx, dy = region_of_rect(W, H, 500, 40, 97, 27)                            # up to the right / bottom edge
    assert (r, dx, dy) == (Region(62, 5, 13, 4), 4, 0) and r.pixel_size(W, H) == (101, 27)
    assert Region(11, 0, 64, 9).pixel_size(W, H) == (509, 67) and Region(0, 4, 10, 5).pixel_size(W, H) == (80, 35)
    for bad in ((0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 2, 2), (0, -1, 2, 2), (590, 0, 8, 1), (0, 60, 1, 8),
                (597, 0, 1, 1), (0, 67, 1, 1), (0, 0, 598, 1)):
        with pytest.raises(ValueError):
            region_of_rect(W, H, *bad)
    with pytest.raises(ValueError):
        region_of_rect(0, 8, 0, 0, 1, 1)


def test_region_kernel_budget(mh):
    """mh_decode_region_kernel (raw and delta): no spill, no scratch, within 80 VGPRs (3 workgroups
    of 8 waves per CU) and the multitable kernel's static LDS -- the budget DESIGN.md section 3d states."""
    from metalhuffman_amd import isa_guard
    if not isa_guard.available():
        pytest.skip("ROCm llvm tools not found")
    ks, res = isa_guard.kernels(mh.LIB_PATH), isa_guard.resources(mh.LIB_PATH)
    region = [k for k in ks if "mh_decode_region_kernel" in k]
    multi = [k for k in ks if "mh_decode_multitable_kernel" in k]
    assert len(region) == 2 and len(multi) == 2, (region, multi)
    for k in region:
        assert ks[k][:3] == (0, 0, 0) and ks[k][3] <= 80, (k, ks[k])
        assert res[k]["vgpr"] == ks[k][3] and res[k]["scratch"] == 0
        assert res[k]["lds"] == res[multi[0]]["lds"] == 53280, (k, res[k])
