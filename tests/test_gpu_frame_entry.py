"""GPU parity of the single-frame entry (mh_decode_frame_kernel).

One frame with a prepared table and no frame-offset array takes the kernel whose whole
argument list is preloaded into SGPRs: 32-bit codes_bytes and pitch, bw and h packed
into one dword, tiles and the raster size derived in the kernel, and the 14-bit table
loaded before the lengths word is known (tables with a longer code reload the 13-bit
one). Every case here is such a launch (but the last), bit-exact against the oracle
and the input. Each decode goes through the C-ABI into a raster with a sentinel-filled
guard band behind it and, with a caller's pitch, beside it: nothing may be written
outside rows [0, H) x columns [0, round_up(W, 8)).
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from helpers import fibonacci_deltas, image_from_block_deltas, long_span_deltas

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _oracle_decode(O, ef):
    t1, t2 = ef.tables()
    return O.decode_frame_shader(ef.block_offsets, ef.codes, t1, t2, ef.width, ef.height,
                                 block_init=ef.block_init, delta=not (ef.flags & 1))


def _decode_one(ef, device, pitch=None, prepared=True):
    """One frame through mh_decode into a sentinel-filled buffer of H rows plus a guard
    band of 8 rows; returns the H x W raster after checking that the guard band and the
    columns from round_up(W, 8) on still hold the sentinel."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    t1, t2 = ef.tables()
    tabs = D.DeviceTables.upload(t1, t2, device, prepare_lut=prepared)
    assert (tabs.lut is not None) == prepared
    fr = D.DeviceFrames.pack([ef], device)
    assert fr.n_frames == 1 and fr.frame_code_offsets is None
    w, h = ef.width, ef.height
    w8 = (w + 7) // 8 * 8
    pitch = w8 if pitch is None else pitch
    buf = torch.full(((h + 8) * pitch,), SENTINEL, dtype=torch.uint8, device=device)
    st = D._frame_struct(fr, tabs)
    N.check(N.lib().mh_decode(ctypes.byref(st), buf.data_ptr(), pitch, h * pitch,
                              torch.cuda.current_stream(device).cuda_stream), "mh_decode")
    torch.cuda.synchronize(device)
    got = buf.cpu().numpy().reshape(h + 8, pitch)
    assert (got[h:] == SENTINEL).all(), "rows below H were written"
    assert (got[:, w8:] == SENTINEL).all(), "columns beyond the row's 8-byte padding were written"
    return got[:h, :w]


def _crop(bigbridge, h, w):
    reps = (-(-h // bigbridge.shape[0]), -(-w // bigbridge.shape[1]))
    return np.ascontiguousarray(np.tile(bigbridge, reps)[:h, :w])


# (h, w): smallest frame (one block, 63 dead lanes, three dead waves); narrow grid (bw 3: a
# tile spans five block rows); ragged last tile (65 blocks); padded rows (pitch 104, rows
# 52..55 dropped); widest bw (8192) and tallest h (65535) in their packed fields
@pytest.mark.parametrize("hw", [(1, 1), (40, 24), (8, 520), (52, 100), (3, 65535), (65535, 8)])
def test_shapes(mh, oracle, device, bigbridge, hw):
    h, w = hw
    img = _crop(bigbridge, h, w)
    ef = mh.encode_frame(img)
    out = _decode_one(ef, device)
    assert np.array_equal(out, img)
    assert np.array_equal(out, _oracle_decode(oracle, ef))


@pytest.mark.parametrize("kind", ["reload16", "common14"])
def test_table_reload(mh, oracle, device, bigbridge, kind):
    """A table with 16-bit codes copies the 13-bit two-level table over the 14-bit one
    the kernel loaded first; a table within 14 bits keeps it."""
    if kind == "reload16":
        img = image_from_block_deltas(fibonacci_deltas(17, 256 * 256, seed=17), 256, 256)
        ef = mh.encode_frame(img)
        assert ef.canon.max() == 16
    else:
        # the 256x256 crop at row 256, column 512: its longest code is exactly 14 bits, the
        # last length that keeps the 14-bit table (the crop at the origin has a 15-bit code)
        img = np.ascontiguousarray(bigbridge[256:512, 512:768])
        ef = mh.encode_frame(img)
        assert ef.canon.max() == 14
    out = _decode_one(ef, device)
    assert np.array_equal(out, img)
    assert np.array_equal(out, _oracle_decode(oracle, ef))


def test_init_byte(mh, oracle, device, bigbridge):
    """block_init as a preloaded pointer."""
    img = _crop(bigbridge, 128, 128)
    ef = mh.encode_frame(img, init_zero_delta=True)
    assert ef.block_init is not None
    out = _decode_one(ef, device)
    assert np.array_equal(out, img)
    assert np.array_equal(out, _oracle_decode(oracle, ef))


def test_oversize_tile(mh, oracle, device):
    """A tile whose span exceeds the LDS window: decode_halves through the new entry."""
    img = image_from_block_deltas(long_span_deltas(1024, 256), 1024, 256)
    ef = mh.encode_frame(img)
    assert (int(ef.block_offsets[64]) - int(ef.block_offsets[0])) // 8 > 4352
    out = _decode_one(ef, device)
    assert np.array_equal(out, img)
    assert np.array_equal(out, _oracle_decode(oracle, ef))


@pytest.mark.parametrize("pitch", [112, 4096, 1 << 20])
def test_callers_pitch(mh, oracle, device, bigbridge, pitch):
    """A pitch wider than round_up(W, 8) = 104, up to the API's 2^20: the u32 pitch."""
    img = _crop(bigbridge, 52, 100)
    ef = mh.encode_frame(img)
    out = _decode_one(ef, device, pitch=pitch)
    assert np.array_equal(out, img)
    assert np.array_equal(out, _oracle_decode(oracle, ef))


def test_no_prepared_table(mh, oracle, device, bigbridge):
    """Without a prepared table the launch is not routed to the new kernel (it would read
    the table through a null pointer) and still decodes."""
    img = _crop(bigbridge, 52, 100)
    ef = mh.encode_frame(img)
    out = _decode_one(ef, device, prepared=False)
    assert np.array_equal(out, img)
    assert np.array_equal(out, _oracle_decode(oracle, ef))
