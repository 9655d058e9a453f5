"""Helpers of the normalised-crops tests (test_crops_norm_*.py, test_gpu_crops_norm.py): the expected
element table T[v] = cvt(fmaf(float32(v), scale, bias)) built WITHOUT the code under test -- libm's
fmaf through ctypes, numpy's float16 cast, and the textbook integer rounding for bfloat16 -- and the
expected bit patterns of a crop. Every comparison in those tests is on bit patterns."""
from __future__ import annotations

import ctypes

import numpy as np

F16, BF16, F32 = 0, 1, 2
FORMATS = (F16, BF16, F32)
NAMES = {F16: "float16", BF16: "bfloat16", F32: "float32"}
ESIZE = {F16: 2, BF16: 2, F32: 4}
BITS = {F16: np.uint16, BF16: np.uint16, F32: np.uint32}   # the dtype of an element's bit pattern
MIRROR = 1

_libm = ctypes.CDLL("libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]

# the fixed (scale, bias) pairs of the host test, shared with the GPU value test
PAIRS = [
    (1.0, 0.0),                                   # exact integers in every format
    (1.0 / 255.0, 0.0),                           # plain normalisation
    (1.0 / (255.0 * 0.229), -0.485 / 0.229),      # mean / std coefficients
    (-1.5, 3.0),                                  # negative scale
    (1.0, 256.0),                                 # bf16 ties at odd values
    (300.0, 0.0),                                 # f16 reaches +inf
    (2.0 ** -20, 0.0),                            # f16 subnormals
    (2.0 ** -140, 0.0),                           # f32 subnormals
    (0.0, 0.1),                                   # zero scale
]


def random_pairs(n=200, seed=2027):
    """Seeded (scale, bias) pairs over many magnitudes and both signs, finite in float32."""
    rng = np.random.default_rng(seed)
    mag = lambda: np.ldexp(rng.uniform(0.5, 1.0, n), rng.integers(-30, 12, n)) * rng.choice([-1.0, 1.0], n)
    return [(float(np.float32(s)), float(np.float32(b))) for s, b in zip(mag(), mag())]


def table_bits(fmt, scale, bias) -> np.ndarray:
    """T as bit patterns, uint16[256] or uint32[256]."""
    f = np.array([_libm.fmaf(float(v), scale, bias) for v in range(256)], np.float32)
    if fmt == F32:
        return f.view(np.uint32).copy()
    if fmt == F16:
        with np.errstate(over="ignore"):
            return np.float32(f).astype(np.float16).view(np.uint16).copy()
    bits = f.view(np.uint32).astype(np.uint64)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def up8(v):
    return (v + 7) // 8 * 8


def expected_crop(T, want, crop, size) -> np.ndarray:
    """The bit patterns of crop = (frame's expected raster `want`, x0, y0, flags) of size (w, h):
    T[numpy slice], reversed along x where mirrored."""
    x0, y0, flags = int(crop[1]), int(crop[2]), int(crop[3]) if len(crop) > 3 else 0
    w, h = size
    assert 0 <= x0 and x0 + w <= want.shape[1] and 0 <= y0 and y0 + h <= want.shape[0], (crop, size)
    px = want[y0: y0 + h, x0: x0 + w]
    if flags & MIRROR:
        px = px[:, ::-1]
    return T[px]


def torch_dtype(fmt):
    import torch
    return (torch.float16, torch.bfloat16, torch.float32)[fmt]


def bits_of(t, fmt) -> np.ndarray:
    """A torch tensor of the format's dtype -> its bit patterns on the host."""
    import torch
    return t.view(torch.int16 if ESIZE[fmt] == 2 else torch.int32).cpu().numpy().view(BITS[fmt])
