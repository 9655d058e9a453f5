"""The C-ABI of the planes entries (include/metalhuffman.h: mh_decode_crops_norm_planes,
mh_decode_crops_norm_planes_shape): exported, and every host check made before any HIP call, with
fake pointers, in mh_decode_crops_norm's order; with one plane, mh_decode_crops_norm's own verdicts;
decode_crops_normalized_planes' validation on the host; codec.norm_coefficients. CPU only. (The
samples themselves live in device memory and are judged by the kernel:
tests/test_gpu_crops_planes.py.)"""
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
NF = 12                               # frames of the default batch


def _frame(**kw):
    """A batch of NF frames of 2045 x 1531 (256 x 192 blocks) that the entry accepts."""
    from metalhuffman_amd import _native as N
    fr = N.mh_frame()
    fr.d_block_offsets = 0x10000
    fr.d_codes = 0x20000
    fr.codes_bytes = 4096
    fr.d_frame_code_offsets = 0x80000
    fr.dims = N.mh_dims(2045, 1531, 256, 192)
    fr.n_frames = NF
    for k, v in kw.items():
        setattr(fr, k, v)
    return fr


def _stride(mh):
    return (int(mh.lib().mh_lut_bytes()) + 15) // 16 * 16


def _floats(v, C):
    """scale / bias as the C array the entry reads: a list as given (it may be longer than C), a
    number repeated C times, or None (NULL)."""
    if v is None:
        return None
    v = [v] * max(C, 1) if isinstance(v, (int, float)) else list(v)
    return (ctypes.c_float * len(v))(*v)


def _call(mh, fr=None, crops=CROPS, n=4, size=(CW, CH), fmt=F16, C=3, fstride=1, scale=1.0, bias=0.0, luts=LUTS,
          stride=None, fstatus=None, cstatus=None, out=OUT, pitch=None, pstride=None, cstride=None):
    """mh_decode_crops_norm_planes with defaults that pass every check (pitch: round_up(w, 8)
    elements; a plane: h rows; a slot: C planes); the callers that must not reach a launch stop it
    with codes_bytes = 2 (SHORT)."""
    from metalhuffman_amd import _native as N
    fr = _frame() if fr is None else fr
    pitch = (size[0] + 7) // 8 * 8 * ESIZE.get(fmt, 2) if pitch is None else pitch
    pstride = pitch * size[1] if pstride is None else pstride
    cstride = (max(C, 1) - 1) * pstride + pitch * size[1] if cstride is None else cstride
    return N.lib().mh_decode_crops_norm_planes(ctypes.byref(fr) if fr is not False else None, crops, n, size[0],
                                               size[1], fmt, C, fstride, _floats(scale, C), _floats(bias, C), luts,
                                               _stride(mh) if stride is None else stride, fstatus, cstatus, out,
                                               pitch, pstride, cstride, None)


SHORT = dict(codes_bytes=2)


def _short(**kw):
    return _frame(**dict(SHORT, **kw))


def test_planes_symbols_exported(mh):
    lib = ctypes.CDLL(mh.LIB_PATH)
    for name in ("mh_decode_crops_norm_planes", "mh_decode_crops_norm_planes_shape"):
        assert hasattr(lib, name), name
        assert name in mh.EXPORTS, name
    from metalhuffman_amd import _native as N
    assert N.MH_MAX_PLANES == 4 == mh.MH_MAX_PLANES
    assert len(N.lib().mh_decode_crops_norm_planes.argtypes) == 19
    assert len(N.lib().mh_decode_crops_norm_planes_shape.argtypes) == 9


def test_planes_header_declares_the_entries():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "metalhuffman.h")).read()
    for piece in ("#define MH_MAX_PLANES 4u",
                  "int mh_decode_crops_norm_planes(const mh_frame *frame, const mh_norm_crop *d_crops, uint32_t n_crops,",
                  "uint32_t n_planes, uint32_t plane_frame_stride,",
                  "const float *scale, const float *bias,",
                  "void *d_out, size_t out_pitch, size_t out_plane_stride,",
                  "size_t out_crop_stride, void *stream);",
                  "int mh_decode_crops_norm_planes_shape(const mh_frame *frame, uint32_t n_crops, uint32_t w, uint32_t h,",
                  "uint32_t format, uint32_t n_planes, void *stream,",
                  "uint32_t *groups_per_plane, uint32_t *waves_per_group);"):
        assert piece in text, piece
    # what the planes entry covers has left the normalised crops' list, and its own list names what is still out
    assert "several channels" not in text and "per crop or per frame" not in text
    for still_out in ("channels-last output", "a pair per crop", "vertical flips", "crops at a reduced scale",
                      "byte output with planes"):
        assert still_out in text, still_out


@pytest.mark.parametrize("fmt", [F16, BF16, F32])
@pytest.mark.parametrize("kw,status", [
    (dict(d_codes=None), INVALID),
    (dict(d_block_offsets=None), INVALID),
    (dict(n_frames=0), INVALID),
    (dict(d_frame_code_offsets=None), INVALID),                # a batch without frame offsets
    (dict(flags=0x2), INVALID),                                # MH_FLAG_LANE_PAIRS: refused here
    (dict(flags=0x8), INVALID),
    (dict(d_codes=0x20004), ALIGN),
    (dict(codes_bytes=2), CAPACITY),
    (dict(flags=0x1 | 0x4, codes_bytes=2), CAPACITY),          # NO_DELTA | ANY_ORDER pass the flag check
    (dict(table2_entries=100, codes_bytes=2), CAPACITY),       # the table fields are ignored ...
    (dict(d_lut=0x70004, codes_bytes=2), CAPACITY),            # ... a misaligned d_lut included
])
def test_planes_rejects_bad_frames(mh, kw, status, fmt):
    assert _call(mh, _frame(**kw), fmt=fmt) == status


@pytest.mark.parametrize("fmt", [F16, BF16, F32])
def test_planes_rejects_bad_arguments(mh, fmt):
    """mh_decode_crops_norm's host checks with their codes, at three planes."""
    from metalhuffman_amd import _native as N
    st = _stride(mh)
    E = ESIZE[fmt]
    pitch, call = 256 * E, lambda *a, **kw: _call(mh, *a, fmt=fmt, **kw)
    pstride = pitch * CH
    cstride = 3 * pstride
    assert call(False) == INVALID                                        # NULL frame
    assert call(out=None) == INVALID
    assert call(luts=None) == INVALID
    assert call(crops=None) == INVALID
    assert call(n=0) == INVALID
    assert call(fstatus=FSTATUS, cstatus=FSTATUS) == INVALID             # the two status arrays alias
    assert call(_short(), fstatus=FSTATUS, cstatus=CSTATUS) == CAPACITY  # (distinct ones pass)
    assert _call(mh, fmt=3) == INVALID and _call(mh, fmt=0xFFFFFFFF) == INVALID and _call(mh, _short(), fmt=3) == INVALID
    assert call(_short(dims=N.mh_dims(2045, 1531, 255, 192))) == DIMS
    for size in ((0, 1), (1, 0), (0, 0), (2046, 1), (1, 1532), (0xFFFFFFFF, 1), (1, 0xFFFFFFFF)):
        assert call(size=size) == DIMS, size
    for size in ((2045, 1531), (1, 1), (2045, 1), (1, 1531)):            # sizes up to the whole frame are inside
        assert call(_short(), size=size, pitch=2040) == ALIGN, size
    assert call(pitch=pitch + 8) == ALIGN and call(pitch=pitch + 4) == ALIGN
    assert call(out=OUT + 8) == ALIGN and call(out=OUT + 4) == ALIGN
    assert call(cstride=cstride + 8) == ALIGN                            # crop stride % 16 (n_crops > 1)
    assert call(crops=CROPS + 8) == ALIGN
    assert call(luts=LUTS + 8) == ALIGN
    assert call(stride=st + 8) == ALIGN and call(stride=8) == ALIGN
    assert call(pitch=pitch - 16) == CAPACITY                            # below the written row
    assert call(pitch=(1 << 20) + 16) == CAPACITY
    assert call(_short(), pitch=1 << 20) == CAPACITY                     # (2^20 itself passes)
    assert call(_short()) == CAPACITY                                    # codes_bytes < MH_CODES_PAD
    assert call(stride=st - 16) == CAPACITY and call(stride=16) == CAPACITY
    assert call(size=(2045, 1), pitch=2048 * E - 16) == CAPACITY         # the whole frame's width needs 2048 elements


@pytest.mark.parametrize("fmt", [F16, F32])
def test_planes_count_and_pairs(mh, fmt):
    """MH_ERR_INVALID_ARG, reported where a bad flag or format is: n_planes 0 or 5, a NULL array, any
    of the n_planes values not finite. Values at index >= n_planes are not looked at."""
    call = lambda *a, **kw: _call(mh, *a, fmt=fmt, **kw)
    for C in (0, 5, 6, 0xFFFFFFFF):
        assert call(C=C, scale=[1.0] * 8, bias=[0.0] * 8) == INVALID, C
        assert call(_short(), C=C, scale=[1.0] * 8, bias=[0.0] * 8) == INVALID, C
    for C in (1, 2, 3, 4):
        assert call(C=C, scale=None) == INVALID and call(C=C, bias=None) == INVALID
        assert call(_short(), C=C, scale=None, bias=None) == INVALID
        assert call(_short(), C=C) == CAPACITY                                       # (a good call passes)
        for c in range(C):
            for bad in (NAN, INF, -INF):
                v = [0.5] * C
                v[c] = bad
                assert call(C=C, scale=v) == INVALID, (C, c, bad)
                assert call(C=C, bias=v) == INVALID, (C, c, bad)
                assert call(_short(), C=C, scale=v, bias=v) == INVALID
        for c in range(C, 6):                                                        # ... beyond the planes: ignored
            for bad in (NAN, INF):
                v = [0.5] * 6
                v[c] = bad
                assert call(_short(), C=C, scale=v, bias=v) == CAPACITY, (C, c, bad)
        assert call(_short(), C=C, scale=[3.0e38] * C, bias=[-3.0e38] * C) == CAPACITY   # large and finite pass
        assert call(_short(), C=C, scale=[0.0] * C, bias=[0.0] * C) == CAPACITY


def test_planes_frame_stride(mh):
    """MH_ERR_DIMS, right after the crop-size check: (n_planes - 1) * plane_frame_stride >= n_frames,
    computed without wrapping. One plane ignores the stride; a stride of 0 is legal."""
    for C, s, ok in ((3, 5, True), (3, 6, False), (4, 3, True), (4, 4, False), (2, 11, True), (2, 12, False),
                     (3, 0, True), (4, 0, True), (2, 0xFFFFFFFF, False), (4, 0xFFFFFFFF, False),
                     (3, 0x80000000, False),          # 2 * 2^31 = 2^32: wraps to 0 in 32 bits
                     (4, 0x55555556, False),          # 3 * 0x55555556 = 2^32 + 2: wraps to 2
                     (3, 0x80000003, False),          # wraps to 6
                     (1, 12, True), (1, 0xFFFFFFFF, True), (1, 0x80000000, True)):
        assert (C - 1) * s < NF if ok else (C - 1) * s >= NF
        assert _call(mh, _short(), C=C, fstride=s) == (CAPACITY if ok else DIMS), (C, s)
    one = _short(n_frames=1, d_frame_code_offsets=None)
    assert _call(mh, one, C=4, fstride=0) == CAPACITY and _call(mh, one, C=2, fstride=1) == DIMS
    # behind the crop-size check (one code), ahead of alignment and capacity
    assert _call(mh, C=3, fstride=6, size=(0, 1)) == DIMS
    assert _call(mh, C=3, fstride=6, out=OUT + 8, pitch=8) == DIMS
    assert _call(mh, C=3, fstride=6, scale=NAN) == INVALID


@pytest.mark.parametrize("fmt", [F16, BF16, F32])
def test_planes_output_strides_at_their_edges(mh, fmt):
    """For n_planes > 1: out_plane_stride % 16 (MH_ERR_ALIGN) and >= out_pitch * h (MH_ERR_CAPACITY); for
    n_crops > 1: out_crop_stride >= (n_planes - 1) * out_plane_stride + out_pitch * h. Accepted shows as
    MH_ERR_CAPACITY through the short codes buffer -- so the strides under test are told apart from it
    by the cases that must be ALIGN, and by the accepted half on a machine without a device."""
    from metalhuffman_amd import _native as N
    no_device = N.lib().mh_device_count() == 0
    E = ESIZE[fmt]
    pitch = 256 * E
    plane = pitch * CH
    ok = HIP if no_device else None

    def verdict(want, **kw):
        if want is not None:
            assert _call(mh, fmt=fmt, **kw) == want, kw

    for C in (2, 3, 4):
        verdict(ALIGN, C=C, pstride=plane + 8)
        verdict(ALIGN, C=C, pstride=plane + 4, cstride=C * (plane + 16))
        verdict(ALIGN, C=C, pstride=plane - 8)                              # misaligned AND too small
        verdict(CAPACITY, C=C, pstride=plane - 16)                          # planes overlap
        verdict(CAPACITY, C=C, pstride=0)
        verdict(ok, C=C, pstride=plane)                                     # exactly h rows
        verdict(ok, C=C, pstride=plane + 16)
        verdict(ok, C=C, pstride=plane + 16, cstride=(C - 1) * (plane + 16) + plane)     # the slot's exact bytes
        verdict(CAPACITY, C=C, pstride=plane + 16, cstride=(C - 1) * (plane + 16) + plane - 16)
        verdict(CAPACITY, C=C, cstride=C * plane - 16)                      # slots overlap by one store
        verdict(CAPACITY, C=C, cstride=plane)                               # a byte crop's slot
        verdict(CAPACITY, C=C, cstride=0)
        verdict(ok, C=C, n=1, cstride=0)                                    # one sample: the crop stride is free
        verdict(ok, C=C, n=1, cstride=8)
        verdict(CAPACITY, C=C, n=1, pstride=plane - 16, cstride=0)          # ... the plane stride is not
        verdict(ALIGN, C=C, n=1, pstride=plane + 8, cstride=0)
        if C > 2:   # a plane stride so large that (C - 1) * stride wraps in 64 bits
            huge = (1 << 64) // (C - 1) + 16 - ((1 << 64) // (C - 1)) % 16
            assert huge % 16 == 0 and huge < 1 << 64 and ((C - 1) * huge) % (1 << 64) < plane
            verdict(CAPACITY, C=C, pstride=huge, cstride=C * plane)
    # one plane: the plane stride is ignored, whatever it is
    for ps in (0, 8, 4, plane - 16, 1 << 63):
        verdict(ok, C=1, pstride=ps, cstride=plane)
        assert _call(mh, _short(), fmt=fmt, C=1, pstride=ps, cstride=plane) == CAPACITY
        assert _call(mh, fmt=fmt, C=1, pstride=ps, cstride=plane - 16) == CAPACITY
        assert _call(mh, fmt=fmt, C=1, pstride=ps, cstride=plane + 8) == ALIGN


def test_planes_check_order(mh):
    """Invalid argument (the planes and the pairs with the flags and the format) before dims, dims
    before alignment, alignment before capacity."""
    from metalhuffman_amd import _native as N
    st = _stride(mh)
    bad_dims = _frame(dims=N.mh_dims(2045, 1531, 255, 192))
    plane = 512 * CH
    assert _call(mh, _frame(flags=0x8), size=(2046, 1)) == INVALID
    assert _call(mh, bad_dims, fmt=3) == INVALID and _call(mh, bad_dims, scale=NAN) == INVALID
    assert _call(mh, bad_dims, C=0) == INVALID and _call(mh, bad_dims, C=5) == INVALID
    assert _call(mh, bad_dims, scale=None) == INVALID and _call(mh, size=(0, 1), bias=None) == INVALID
    assert _call(mh, size=(0, 1), bias=INF) == INVALID and _call(mh, size=(0, 1), C=5, out=OUT + 8) == INVALID
    assert _call(mh, C=5, fstride=100, pstride=8, cstride=0) == INVALID
    assert _call(mh, bad_dims, crops=None) == INVALID
    assert _call(mh, size=(0, 1), fstatus=FSTATUS, cstatus=FSTATUS) == INVALID
    assert _call(mh, bad_dims, crops=CROPS + 8, stride=st - 16, pitch=504) == DIMS
    assert _call(mh, size=(2046, 24), crops=CROPS + 8, luts=LUTS + 8, stride=st - 16, pitch=504) == DIMS
    assert _call(mh, fstride=6, crops=CROPS + 8, pstride=8, cstride=0) == DIMS
    assert _call(mh, crops=CROPS + 8, stride=st - 16, pitch=512 - 16) == ALIGN
    assert _call(mh, pstride=plane + 8, cstride=0) == ALIGN                # misaligned plane, slots too small
    assert _call(mh, pstride=8) == ALIGN                                  # misaligned AND too small
    assert _call(mh, stride=8, pstride=0) == ALIGN
    assert _call(mh, _short(), stride=st - 16, pstride=0) == CAPACITY


def test_planes_tile_capacity(mh):
    """The tile cap is counted over n_crops * n_planes: 131 tiles x 8193 block rows for a crop of
    65535 x 65535."""
    from metalhuffman_amd import _native as N
    tiles = 131 * 8193
    most = (2 ** 31 - 1) // tiles
    big = _frame(dims=N.mh_dims(65535, 65535, 8192, 8192))
    L = N.lib()
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    shape = lambda n, C: L.mh_decode_crops_norm_planes_shape(ctypes.byref(big), n, 65535, 65535, F16, C, None,
                                                             ctypes.byref(g), ctypes.byref(w))
    for C in (1, 2, 3, 4):
        n = most // C
        assert (n + 1) * C * tiles > 2 ** 31 - 1 >= n * C * tiles
        assert _call(mh, big, n=n + 1, C=C, size=(65535, 65535), fmt=F32) == CAPACITY
        assert shape(n + 1, C) == CAPACITY
        if L.mh_device_count() == 0:
            assert _call(mh, big, n=n, C=C, size=(65535, 65535), fmt=F32) == HIP
            assert shape(n, C) == HIP
    # n_crops * n_planes itself past 2^32
    assert _call(mh, n=0x40000000, C=4, size=(8, 1), pitch=16) == CAPACITY
    assert _call(mh, n=0xFFFFFFFF, C=3, size=(8, 1), pitch=16) == CAPACITY


def _norm_cases():
    """tests/test_crops_norm_abi.py's argument table, as keyword sets both entries take."""
    P = 512
    S = P * CH
    cases = [dict(), dict(out=None), dict(luts=None), dict(crops=None), dict(n=0),
             dict(fstatus=FSTATUS, cstatus=FSTATUS), dict(fstatus=FSTATUS, cstatus=CSTATUS), dict(fmt=3),
             dict(fmt=0xFFFFFFFF), dict(scale=NAN), dict(bias=INF), dict(scale=-INF), dict(scale=3.0e38, bias=-3.0e38),
             dict(scale=0.0, bias=0.0), dict(pitch=P + 8), dict(pitch=P + 4), dict(out=OUT + 8), dict(out=OUT + 4),
             dict(cstride=S + 8), dict(crops=CROPS + 8), dict(luts=LUTS + 8), dict(stride=8), dict(pitch=P - 16),
             dict(size=(256, CH), pitch=P - 16, cstride=S), dict(pitch=(1 << 20) + 16),
             dict(pitch=1 << 20, cstride=(1 << 20) * CH), dict(cstride=S - 16), dict(cstride=0),
             dict(pitch=P + 16, cstride=S), dict(stride=16), dict(stride=0), dict(size=(CW, 3), cstride=P * 3),
             dict(size=(CW, 3), cstride=P * 2), dict(size=(2045, 1), pitch=4096 - 16, cstride=4096),
             dict(n=1, cstride=0), dict(n=1, cstride=8), dict(pitch=P + 48, cstride=(P + 48) * CH + 80),
             dict(size=(2045, 1531)), dict(size=(1, 1), pitch=16, cstride=16), dict(n=1000)]
    cases += [dict(size=s) for s in ((0, 1), (1, 0), (0, 0), (2046, 1), (1, 1532), (2048, 1), (1, 1536),
                                     (0xFFFFFFFF, 1), (1, 0xFFFFFFFF))]
    cases += [dict(size=(w, 4), fmt=f, n=1, pitch=p) for w in (1, 4, 5, 9, 12, 13) for f in (F16, F32)
              for p in ((w * ESIZE[f] + 15) // 16 * 16, (w + 7) // 8 * 8 * ESIZE[f])]
    return cases


FRAMES = [dict(), dict(codes_bytes=2), dict(flags=0x2), dict(flags=0x8), dict(flags=0x5), dict(d_codes=0x20004),
          dict(d_codes=None), dict(n_frames=0), dict(d_frame_code_offsets=None), dict(table2_entries=100),
          "bad_dims"]


@pytest.mark.parametrize("frame", range(len(FRAMES)))
def test_one_plane_is_the_normalised_crops_entry(mh, frame):
    """With n_planes == 1 the entry gives mh_decode_crops_norm's verdict for every argument set of that
    entry's own test, whatever the two plane strides hold. (With a device the fake pointers must not
    be launched on: there only the rejected sets are compared.)"""
    from metalhuffman_amd import _native as N
    L = N.lib()
    device = L.mh_device_count() > 0
    fkw = FRAMES[frame]
    fkw = dict(dims=N.mh_dims(2045, 1531, 255, 192)) if fkw == "bad_dims" else fkw
    seen = set()
    for kw in _norm_cases():
        kw = dict(kw)
        size, fmt = kw.pop("size", (CW, CH)), kw.pop("fmt", F16)
        n, scale, bias = kw.pop("n", 4), kw.pop("scale", 1.0), kw.pop("bias", 0.0)
        pitch = kw.pop("pitch", (size[0] + 7) // 8 * 8 * ESIZE.get(fmt, 2))
        cstride = kw.pop("cstride", pitch * size[1])
        stride = kw.pop("stride", _stride(mh))
        crops, luts, out = kw.pop("crops", CROPS), kw.pop("luts", LUTS), kw.pop("out", OUT)
        fstatus, cstatus = kw.pop("fstatus", None), kw.pop("cstatus", None)
        assert not kw
        fr = _frame(**fkw)
        if device and "codes_bytes" not in fkw:
            fr.codes_bytes = 2
        want = L.mh_decode_crops_norm(ctypes.byref(fr), crops, n, size[0], size[1], fmt, scale, bias, luts, stride,
                                      fstatus, cstatus, out, pitch, cstride, None)
        for fstride, pstride in ((1, 0), (0xFFFFFFFF, 8), (0, pitch * size[1]), (7, (1 << 64) - 1)):
            got = L.mh_decode_crops_norm_planes(ctypes.byref(fr), crops, n, size[0], size[1], fmt, 1, fstride,
                                                _floats(scale, 1), _floats(bias, 1), luts, stride, fstatus, cstatus,
                                                out, pitch, pstride, cstride, None)
            assert got == want, (fkw, size, fmt, n, pitch, cstride, fstride, pstride, got, want)
        seen.add(want)
    assert want in (INVALID, DIMS, ALIGN, CAPACITY, HIP)
    if not fkw:
        assert {INVALID, DIMS, ALIGN, CAPACITY} <= seen and (device or HIP in seen)


def test_planes_accepted_calls_reach_the_device(mh):
    """Without a HIP device a call that passes every check ends in MH_ERR_HIP (the first HIP call finds
    no device). With a device the fake pointers must not be launched on; there
    tests/test_gpu_crops_planes.py makes the same calls with real buffers."""
    from metalhuffman_amd import _native as N
    assert _call(mh, stride=16) == CAPACITY
    if N.lib().mh_device_count() > 0:
        return
    for fmt in (F16, BF16, F32):
        E = ESIZE[fmt]
        for C in (1, 2, 3, 4):
            assert _call(mh, fmt=fmt, C=C) == HIP
            assert _call(mh, fmt=fmt, C=C, stride=0) == HIP                 # the shared table
            assert _call(mh, fmt=fmt, C=C, fstride=0) == HIP                # one frame, C maps
            assert _call(mh, fmt=fmt, C=C, fstride=(NF - 1) // max(C - 1, 1)) == HIP
            assert _call(mh, fmt=fmt, C=C, fstatus=FSTATUS, cstatus=CSTATUS) == HIP
            pitch = 256 * E + 48
            assert _call(mh, fmt=fmt, C=C, pitch=pitch, pstride=pitch * CH + 32,
                         cstride=C * (pitch * CH + 32) + 80) == HIP
            assert _call(mh, fmt=fmt, C=C, size=(2045, 1531)) == HIP        # the whole frame
            assert _call(mh, fmt=fmt, C=C, size=(1, 1)) == HIP
            assert _call(mh, fmt=fmt, C=C, scale=[-3.0e38] * C, bias=[1.0e-45] * C) == HIP
            g, w = ctypes.c_uint32(), ctypes.c_uint32()
            assert N.lib().mh_decode_crops_norm_planes_shape(ctypes.byref(_frame()), 4, CW, CH, fmt, C, None,
                                                             ctypes.byref(g), ctypes.byref(w)) == HIP
    assert _call(mh, n=1000) == HIP                                         # more samples than frames


def test_planes_shape_rejects_bad_arguments(mh):
    from metalhuffman_amd import _native as N
    L = N.lib()
    g, w = ctypes.c_uint32(), ctypes.c_uint32()
    G, Wv = ctypes.byref(g), ctypes.byref(w)
    ok = lambda **kw: ctypes.byref(_frame(**kw))
    shape = L.mh_decode_crops_norm_planes_shape
    assert shape(None, 4, CW, CH, F16, 3, None, G, Wv) == INVALID
    assert shape(ok(), 4, CW, CH, F16, 3, None, None, Wv) == INVALID
    assert shape(ok(), 4, CW, CH, F16, 3, None, G, None) == INVALID
    assert shape(ok(), 0, CW, CH, F16, 3, None, G, Wv) == INVALID
    assert shape(ok(n_frames=0), 4, CW, CH, F16, 3, None, G, Wv) == INVALID
    assert shape(ok(flags=0x2), 4, CW, CH, F16, 3, None, G, Wv) == INVALID
    assert shape(ok(), 4, CW, CH, 3, 3, None, G, Wv) == INVALID
    for C in (0, 5, 0xFFFFFFFF):
        assert shape(ok(), 4, CW, CH, F16, C, None, G, Wv) == INVALID
        assert shape(ok(), 4, 0, CH, F16, C, None, G, Wv) == INVALID           # the planes before the dims
    assert shape(ok(), 4, 0, CH, 3, 3, None, G, Wv) == INVALID                 # the format before the dims
    assert shape(ok(dims=N.mh_dims(16, 16, 3, 2)), 4, 1, 1, F32, 3, None, G, Wv) == DIMS
    for size in ((0, 8), (8, 0), (2046, 8), (8, 1532), (0xFFFFFFFF, 1)):
        for C in (1, 4):
            assert shape(ok(), 4, size[0], size[1], BF16, C, None, G, Wv) == DIMS, size


# ---- decode_crops_normalized_planes' validation on the host ---------------------------------------------

W, H = 597, 67   # 75 x 9 blocks, partial right and bottom blocks
PAIRS3 = ([0.5, -1.0, 2.0], [0.0, 1.0, -2.0])


def _host_frames(n=6):
    """A DeviceFrames description with host tensors: the size, the format, the pairs, the plane stride
    and a host list are validated before a buffer is looked at, so these calls end in the ValueError
    under test (or, for a valid list, in the ValueError that the buffers are not on a HIP device)."""
    import torch
    from metalhuffman_amd import decoder as D
    z = torch.zeros(16, dtype=torch.uint8)
    return D.DeviceFrames(W, H, n, torch.zeros(4, dtype=torch.int32), z, None)


@pytest.mark.parametrize("crops,size", [
    ([(6, 0, 0)], (80, 24)),                   # frame >= n_frames
    ([(0, 0, 0), (-1, 0, 0)], (80, 24)),
    ([(0, 518, 0)], (80, 24)),                 # x0 + w > 597
    ([(0, 0, 44)], (80, 24)),                  # y0 + h > 67
    ([(0, 0xFFFFFFFF, 0, 0)], (80, 24)),
    ([(0, 0, 0, 2)], (80, 24)),                # an unknown flag bit
    ([(0, 0, 0, -1)], (80, 24)),
    ([(0, 0, 0, 1)], (19, 13)),                # mirrored, w % 8 != 0
    ([(0, 0, 0, 0, 0)], (80, 24)),             # five columns
    ([], (80, 24)),
    ([(0.5, 0, 0)], (80, 24)),
    ([(3, 0, 0), (4, 0, 0)], (80, 24)),        # frame 4 + 2 planes: no frame 6
    ([(3, 0, 0, 1), (5, 0, 0, 0)], (80, 24)),
])
def test_planes_wrapper_rejects_bad_host_lists(crops, size):
    import torch
    from metalhuffman_amd import decoder as D
    with pytest.raises(ValueError, match="crop"):
        D.decode_crops_normalized_planes(_host_frames(), None, crops, size, torch.float16, *PAIRS3)
    with pytest.raises(ValueError, match="crop"):
        D.decode_crops_normalized_planes(_host_frames(), None, np.asarray(crops), size, torch.float32, *PAIRS3)


def test_planes_wrapper_names_the_crop_whose_last_plane_is_missing():
    import torch
    from metalhuffman_amd import decoder as D
    good = [(0, 0, 0, 0), (3, 517, 43, 1), (1, 5, 5, 0)]
    for crops, ps, which in ((good + [(4, 0, 0, 0)], 1, "crop 3"), ([(0, 0, 0, 0), (2, 1, 1, 0)] + good, 2, "crop 1"),
                             ([(2, 9, 9, 1)], 2, "crop 0"), ([(0, 0, 0), (5, 0, 0)], 1, "crop 1")):
        with pytest.raises(ValueError, match=which):
            D.decode_crops_normalized_planes(_host_frames(), None, crops, (80, 24), torch.float16, *PAIRS3,
                                             plane_stride=ps)
    # the same lists are fine where the planes fit: the call ends at the next check (host buffers)
    for crops, ps in ((good, 1), ([(0, 0, 0, 0), (1, 1, 1, 1)], 2), ([(5, 0, 0)], 0)):
        with pytest.raises(ValueError, match="HIP device"):
            D.decode_crops_normalized_planes(_host_frames(), None, crops, (80, 24), torch.float16, *PAIRS3,
                                             plane_stride=ps)


def test_planes_wrapper_rejects_bad_pairs_strides_sizes_and_formats():
    import torch
    from metalhuffman_amd import decoder as D
    call = lambda *a, **kw: D.decode_crops_normalized_planes(_host_frames(), None, [(0, 0, 0)], (80, 24), *a, **kw)
    for scale, bias in (([], []), ([1.0] * 5, [0.0] * 5), ([1.0, 2.0], [0.0]), ([1.0], [0.0, 0.0]), (1.0, 0.0),
                        ([1.0, 2.0, 3.0], None)):
        with pytest.raises(ValueError, match="scale and bias"):
            call(torch.float16, scale, bias)
    for bad in (NAN, INF, -INF, 1e39):
        for c in range(3):
            v = [0.5, 0.25, 0.125]
            v[c] = bad
            with pytest.raises(ValueError, match="finite"):
                call(torch.float16, v, [0.0] * 3)
            with pytest.raises(ValueError, match="finite"):
                call(torch.bfloat16, [1.0] * 3, v)
    for ps in (-1, 3, 6, 1 << 32):
        with pytest.raises(ValueError, match="planes"):
            call(torch.float16, *PAIRS3, plane_stride=ps)
    with pytest.raises(ValueError, match="HIP device"):
        call(torch.float16, *PAIRS3, plane_stride=2)
    with pytest.raises(ValueError, match="HIP device"):
        call(torch.float16, [1.0], [0.0], plane_stride=1000)              # one plane: the stride is not used
    for bad in (torch.uint8, torch.float64, "int8", 3, None):
        with pytest.raises(ValueError, match="format"):
            call(bad, *PAIRS3)
        with pytest.raises(ValueError, match="format"):
            D.decode_crops_normalized_planes_shape(_host_frames(), 1, (80, 24), bad, 3)
    for size in ((0, 3), (10, 0), (598, 3), (10, 68), (-1, 3)):
        with pytest.raises(ValueError, match="does not fit"):
            D.decode_crops_normalized_planes(_host_frames(), None, [(0, 0, 0)], size, torch.bfloat16, *PAIRS3)
        with pytest.raises(ValueError, match="does not fit"):
            D.decode_crops_normalized_planes_shape(_host_frames(), 1, size, torch.bfloat16, 3)
    for C in (0, 5, -1):
        with pytest.raises(ValueError, match="planes"):
            D.decode_crops_normalized_planes_shape(_host_frames(), 1, (80, 24), torch.float16, C)
    with pytest.raises(ValueError, match="no crops"):
        D.decode_crops_normalized_planes_shape(_host_frames(), 0, (80, 24), torch.float16, 3)


# ---- codec.norm_coefficients ------------------------------------------------------------------------------

def test_norm_coefficients():
    from metalhuffman_amd import codec
    import metalhuffman_amd as mh
    assert mh.norm_coefficients is codec.norm_coefficients
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    scale, bias = codec.norm_coefficients(mean, std)
    assert len(scale) == len(bias) == 3
    for c in range(3):
        assert scale[c] == float(np.float32(1.0 / (255.0 * std[c])))
        assert bias[c] == float(np.float32(-mean[c] / std[c]))
        assert np.float32(scale[c]) == scale[c] and np.float32(bias[c]) == bias[c]     # float32 values
    assert codec.norm_coefficients([0.0], [1.0]) == ([float(np.float32(1.0 / 255.0))], [0.0])
    assert codec.norm_coefficients(0.5, -2.0) == ([float(np.float32(-1.0 / 510.0))], [0.25])
    assert codec.norm_coefficients(np.array([0.5, 0.25]), np.array([0.5, 0.25]))[1] == [-1.0, -1.0]
    for mean, std in (([0.5], [0.0]), ([0.5, 0.5], [1.0, 0.0]), ([0.5], [-0.0]), ([0.5], [NAN]), ([0.5], [INF]),
                      ([0.5], [-INF]), ([0.1, 0.2, 0.3], [0.1, NAN, 0.3]), ([NAN], [1.0]), ([INF], [1.0]),
                      ([0.5, 0.5], [1.0]), ([], []), ([1e30], [1e-30])):
        with pytest.raises(ValueError):
            codec.norm_coefficients(mean, std)
    # the pairs are what the entry takes
    C, s, b = __import__("metalhuffman_amd.decoder", fromlist=["x"])._plane_coefficients(scale, bias)
    assert C == 3 and list(s) == scale and list(b) == bias
