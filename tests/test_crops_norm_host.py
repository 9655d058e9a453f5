"""mh_norm_table / codec.norm_table, the CPU twin of mh_decode_crops_norm's conversion: the 256
elements T[v] = cvt(fmaf(float32(v), scale, bias)) for the three formats, compared bit for bit with
norm_helpers.table_bits (libm's fmaf, numpy's float16 cast, integer rounding for bfloat16). CPU only."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import norm_helpers as NH

INVALID, CAPACITY = -1, -4


def _c_table(mh, fmt, scale, bias):
    out = np.zeros(256, NH.BITS[fmt])
    assert mh.lib().mh_norm_table(fmt, scale, bias, out.ctypes.data_as(ctypes.c_void_p), out.nbytes) == 0
    return out


def _check(mh, fmt, scale, bias):
    from metalhuffman_amd import codec
    want = NH.table_bits(fmt, scale, bias)
    got = _c_table(mh, fmt, scale, bias)
    assert np.array_equal(got, want), (fmt, scale, bias, np.flatnonzero(got != want)[:8])
    py = codec.norm_table(NH.NAMES[fmt], scale, bias)
    assert py.shape == (256,) and py.dtype == (np.float16, np.uint16, np.float32)[fmt]
    assert np.array_equal(py.view(NH.BITS[fmt]), want), (fmt, scale, bias)
    return want


@pytest.mark.parametrize("fmt", NH.FORMATS)
@pytest.mark.parametrize("pair", NH.PAIRS)
def test_norm_table_fixed_pairs(mh, fmt, pair):
    _check(mh, fmt, *pair)


@pytest.mark.parametrize("fmt", NH.FORMATS)
def test_norm_table_random_pairs(mh, fmt):
    pairs = NH.random_pairs()
    assert len(pairs) == 200
    for s, b in pairs:
        _check(mh, fmt, s, b)


def test_norm_table_identity_is_exact(mh):
    """(1, 0): the integers 0..255 are exact in all three formats."""
    assert np.array_equal(_check(mh, NH.F16, 1.0, 0.0).view(np.float16).astype(np.float64), np.arange(256.0))
    assert np.array_equal(_check(mh, NH.F32, 1.0, 0.0).view(np.float32).astype(np.float64), np.arange(256.0))
    bf = _check(mh, NH.BF16, 1.0, 0.0)
    assert np.array_equal((bf.astype(np.uint32) << 16).view(np.float32).astype(np.float64), np.arange(256.0))


def test_norm_table_bf16_ties_to_even(mh):
    """(1, 256): bfloat16 has 8 significant bits, so 256..511 step by 2 and the odd values are ties:
    257 -> 256 and 259 -> 260."""
    t = (_check(mh, NH.BF16, 1.0, 256.0).astype(np.uint32) << 16).view(np.float32)
    assert t[1] == 256.0 and t[3] == 260.0 and t[0] == 256.0 and t[2] == 258.0 and t[255] == 512.0


def test_norm_table_f16_overflows_to_inf(mh):
    """(300, 0): 300 * 219 = 65700 is above 65520, the last value that rounds to 65504."""
    t = _check(mh, NH.F16, 300.0, 0.0).view(np.float16)
    assert np.isinf(t[219:]).all() and (t[219:] > 0).all() and np.isfinite(t[:219]).all() and t[218] == np.float16(65408)
    assert (_check(mh, NH.F16, -300.0, 0.0).view(np.float16)[219:] == -np.inf).all()
    assert not np.isnan(t).any()


def test_norm_table_subnormals_are_kept(mh):
    """(2^-20, 0): v 2^-20 is below 2^-14 for v < 64 -- binary16 subnormals, exact multiples of 2^-24.
    (2^-140, 0): binary32 subnormals."""
    t16 = _check(mh, NH.F16, 2.0 ** -20, 0.0)
    sub = [v for v in range(1, 256) if (t16[v] & 0x7C00) == 0]
    assert sub == list(range(1, 64)) and all(t16[v] == 16 * v for v in sub)
    t32 = _check(mh, NH.F32, 2.0 ** -140, 0.0)
    assert all((t32[v] & 0x7F800000) == 0 and t32[v] != 0 for v in range(1, 256))
    assert (_check(mh, NH.BF16, 2.0 ** -133, 0.0)[1:] != 0).all()       # bfloat16 subnormals too


def test_norm_table_zero_scale(mh):
    for fmt in NH.FORMATS:
        t = _check(mh, fmt, 0.0, 0.1)
        assert (t == t[0]).all()


def test_norm_table_argument_errors(mh):
    from metalhuffman_amd import codec
    L = mh.lib()
    buf = np.zeros(256, np.uint32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert "mh_norm_table" in mh.EXPORTS
    assert L.mh_norm_table(0, 1.0, 0.0, None, 1024) == INVALID
    assert L.mh_norm_table(3, 1.0, 0.0, p, 1024) == INVALID
    assert L.mh_norm_table(0xFFFFFFFF, 1.0, 0.0, p, 1024) == INVALID
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert L.mh_norm_table(0, bad, 0.0, p, 1024) == INVALID
        assert L.mh_norm_table(2, 1.0, bad, p, 1024) == INVALID
        with pytest.raises(ValueError, match="finite"):
            codec.norm_table("float16", bad, 0.0)
        with pytest.raises(ValueError, match="finite"):
            codec.norm_table("float32", 1.0, bad)
    assert L.mh_norm_table(3, float("nan"), 0.0, None, 0) == INVALID     # invalid argument before capacity
    for fmt, need in ((0, 512), (1, 512), (2, 1024)):
        assert L.mh_norm_table(fmt, 1.0, 0.0, p, need - 1) == CAPACITY
        assert L.mh_norm_table(fmt, 1.0, 0.0, p, 0) == CAPACITY
        assert L.mh_norm_table(fmt, 1.0, 0.0, p, need) == 0
    # exactly 256 elements are written
    buf[:] = 0xA5A5A5A5
    assert L.mh_norm_table(0, 1.0, 0.0, p, 1024) == 0
    assert (buf[128:] == 0xA5A5A5A5).all() and (buf[:128] != 0xA5A5A5A5).all()
    for bad in (3, -1, "float64", np.float64, "uint8", None, True):
        with pytest.raises(ValueError, match="format"):
            codec.norm_table(bad, 1.0, 0.0)
    with pytest.raises(ValueError, match="finite"):
        codec.norm_table(0, 1e39, 0.0)                                   # infinite once rounded to float32


def test_norm_table_accepts_dtypes(mh):
    import torch
    from metalhuffman_amd import codec
    for fmt, forms in ((0, (0, "float16", np.float16, np.dtype("float16"), torch.float16)),
                       (1, (1, "bfloat16", torch.bfloat16)),
                       (2, (2, "float32", np.float32, torch.float32))):
        want = NH.table_bits(fmt, 1.0 / 255.0, -0.5)
        for form in forms:
            assert np.array_equal(codec.norm_table(form, 1.0 / 255.0, -0.5).view(NH.BITS[fmt]), want), form
