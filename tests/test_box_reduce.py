"""mh_box_reduce (codec.box_reduce), the CPU twin of mh_decode_region_scaled's output stage, against
the numpy statement of the definition (scaled_helpers.box_reduce_np), and the rounding it shares
with the kernels (csrc/mh_box.hpp) over every reachable (sum, pixel count). CPU only."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from scaled_helpers import box_reduce_np

INVALID, CAPACITY = -1, -4


def _images(w, h, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    return (np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8),
            np.full((h, w), 255, np.uint8),
            (((yy + xx) & 1) * 255).astype(np.uint8))


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_box_reduce_matches_numpy(mh, k):
    """Every W, H in 1..17: random, all-255 (saturation) and a 0/255 checkerboard (ties)."""
    s = 1 << k
    for h in range(1, 18):
        for w in range(1, 18):
            for i, img in enumerate(_images(w, h, 1000 * k + 17 * h + w)):
                got = mh.box_reduce(img, k)
                assert got.shape == (-(-h // s), -(-w // s)) and got.dtype == np.uint8
                assert np.array_equal(got, box_reduce_np(img, k)), (w, h, k, i)
                if k == 0:
                    assert np.array_equal(got, img)


def test_definition_by_hand():
    """The numpy definition itself on cases worked out by hand: halves round up, edge cells average
    their in-frame pixels only."""
    assert box_reduce_np(np.array([[0, 255], [255, 0]], np.uint8), 1).tolist() == [[128]]      # 127.5 -> 128
    assert box_reduce_np(np.array([[1, 2], [3, 4]], np.uint8), 1).tolist() == [[3]]            # 2.5 -> 3
    assert box_reduce_np(np.array([[1, 1], [1, 2]], np.uint8), 1).tolist() == [[1]]            # 1.25 -> 1
    assert box_reduce_np(np.array([[10, 20, 31]], np.uint8), 1).tolist() == [[15, 31]]         # n = 2, n = 1
    assert box_reduce_np(np.array([[10], [21], [255]], np.uint8), 1).tolist() == [[16], [255]]  # 15.5 -> 16
    assert box_reduce_np(np.full((3, 5), 255, np.uint8), 3).tolist() == [[255]]
    assert box_reduce_np(np.array([[0, 1, 0]], np.uint8), 2).tolist() == [[0]]                 # 1/3 -> 0
    assert box_reduce_np(np.array([[0, 1, 1]], np.uint8), 2).tolist() == [[1]]                 # 2/3 -> 1


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_box_reduce_pitches_and_guards(mh, k):
    """A padded pitch on both sides: the input's padding is not read into a cell, and the output's
    guard bytes (row padding, rows below) survive."""
    from metalhuffman_amd import _native as N
    w, h, pitch, out_pitch = 13, 11, 19, 23
    s = 1 << k
    sw, sh = -(-w // s), -(-h // s)
    src = np.full((h + 2, pitch), 0xEE, np.uint8)
    img = np.random.default_rng(5 + k).integers(0, 256, (h, w), dtype=np.uint8)
    src[:h, :w] = img
    out = np.full((sh + 2, out_pitch), 0xA5, np.uint8)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    rc = N.lib().mh_box_reduce(src.ctypes.data_as(u8p), w, h, pitch, k, out.ctypes.data_as(u8p), out_pitch)
    assert rc == 0
    assert np.array_equal(out[:sh, :sw], box_reduce_np(img, k))
    assert (out[:sh, sw:] == 0xA5).all() and (out[sh:] == 0xA5).all()


def test_box_reduce_rejects_bad_arguments(mh):
    from metalhuffman_amd import _native as N
    L = N.lib()
    a = np.zeros(64, np.uint8)
    p = a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert L.mh_box_reduce(None, 8, 8, 8, 1, p, 4) == INVALID
    assert L.mh_box_reduce(p, 8, 8, 8, 1, None, 4) == INVALID
    assert L.mh_box_reduce(p, 0, 8, 8, 1, p, 4) == INVALID
    assert L.mh_box_reduce(p, 8, 0, 8, 1, p, 4) == INVALID
    assert L.mh_box_reduce(p, 8, 8, 8, 4, p, 4) == INVALID
    assert L.mh_box_reduce(p, 8, 8, 7, 1, p, 4) == CAPACITY
    assert L.mh_box_reduce(p, 7, 8, 8, 1, p, 3) == CAPACITY      # SW = 4
    for bad in (-1, 4, 1.5):
        with pytest.raises(ValueError):
            mh.box_reduce(np.zeros((8, 8), np.uint8), bad)
    with pytest.raises(ValueError):
        mh.box_reduce(np.zeros((0, 8), np.uint8), 1)


def test_rounding_exhaustive(mh):
    """The division the kernels' edge cells and mh_box_reduce share, through mh_box_reduce on
    one-cell images: every pixel count n = cw * ch with cw, ch in 1..8 and every sum 0..255 n
    (255 * 36^2 + 64 = 330,544 cases), against integer arithmetic."""
    from metalhuffman_amd import _native as N
    L = N.lib()
    cases = 0
    for ch in range(1, 9):
        for cw in range(1, 9):
            n = cw * ch
            buf = (ctypes.c_uint8 * n)()          # a cw x ch image, pitch cw: one cell at scale 8
            out = (ctypes.c_uint8 * 1)()
            got = np.empty(255 * n + 1, np.uint8)
            for total in range(255 * n + 1):
                if total:                         # one more grey level, spread round-robin over the pixels
                    buf[(total - 1) % n] += 1
                assert L.mh_box_reduce(buf, cw, ch, cw, 3, out, 1) == 0
                got[total] = out[0]
            assert sum(buf) == 255 * n
            S = np.arange(255 * n + 1, dtype=np.int64)
            want = (2 * S + n) // (2 * n)
            assert np.array_equal(got, want), (cw, ch, int(np.flatnonzero(got != want)[0]))
            cases += S.size
    assert cases == 255 * 36 * 36 + 64
