"""GPU parity of the small-launch chain's row loop (decode_block's lazy step).

The single-frame and small-launch kernels decode a block's 8 rows in a real loop: the lane
state (window, cursor, next word, stage address) and the row's store offset, which advances
by the pitch, are carried from trip to trip, and a trip ends with the lookup of the next
row's first symbol. Every case decodes through the C-ABI with a prepared table, once as one
frame without a frame-offset array (mh_decode_frame_kernel) and once as a 2-frame launch
(mh_decode_small_kernel), into rasters laid out inside one pattern-filled buffer
(helpers.containment_plan); every byte of the buffer is checked: the pixels bit-exact
against the oracle's decode_frame_shader (itself equal to the image the frame was made
from), everything else against the fill.

Shapes (grid W x H, declared W x H), where a row loop can go wrong:
  one_block  8 x 8: one block, 63 dead lanes (their stores start at 2^31 and advance too)
  blocks65   520 x 8: 65 blocks, the second tile has one live lane
  edge       16 x 16 declared 12 x 13: partial edge blocks; rows 13..15 must be dropped
  rows9      64 x 72 at a pitch of 128 (twice the row): 72 blocks over 9 block rows, tile 0
             spans 8 of them; and once at the API's largest pitch, 2^20
A frame this small cannot carry a long Huffman code, so each frame is the first block rows
(EncodedFrame.band) of a taller frame on the same grid that can, with one of every symbol
of the table moved into its first block.

Tables: len14 (longest code 14 bits: the staged 14-bit chain), esc16 (a 16-bit code: the
13-bit table with escapes), flat8 (all 256 symbols at 8 bits: byte arithmetic, no chain),
long_tile (shapes with a whole tile only: 4,096 symbols of 14-16 bits fill blocks 0..63, so
the tile's span exceeds the 4,352-byte stage and decode_halves runs the chain twice).
Each with and without MH_FLAG_NO_DELTA; MH_FLAG_ANY_ORDER over three launches in a row.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import pytest

from helpers import check_containment, containment_plan, fibonacci_deltas

pytestmark = pytest.mark.gpu

# name: (grid W, grid H, declared W, declared H, pitch)
SHAPES = {"one_block": (8, 8, 8, 8, 8), "blocks65": (520, 8, 520, 8, 520), "edge": (16, 16, 12, 13, 16),
          "rows9": (64, 72, 64, 72, 128)}
STAGE_BYTES = 4352  # kStageBytes (mh_decode.hip)
N_FRAMES = 3        # distinct frames per case, one table


def _one_of_each_first(d):
    """The same multiset with one of every value at the front (the first block)."""
    first = np.array([np.flatnonzero(d == v)[0] for v in np.unique(d)])
    rest = np.setdiff1d(np.arange(d.size), first)
    return d[np.concatenate([first, rest])]


def _long_tile_symbols(nb, seed):
    """128 rare values x 32 under a geometric chain of 8 common ones (so 14-16 bits each), the
    rare ones first: they fill blocks 0..63."""
    n = nb * 64
    assert n >= 1 << 20
    rare = np.repeat(np.arange(128, 256, dtype=np.uint8), 32)
    chain = np.repeat(np.arange(8, dtype=np.uint8), [(1 << 20) >> (k + 1) for k in range(8)])
    rest = np.concatenate([chain, np.zeros(n - rare.size - chain.size, np.uint8)])
    r = np.random.default_rng(seed)
    r.shuffle(rare)
    r.shuffle(rest)
    return np.concatenate([rare, rest])


def _symbols(table, nb, seed):
    if table == "len14":
        return _one_of_each_first(fibonacci_deltas(15, nb * 64, seed=seed))
    if table == "esc16":
        return _one_of_each_first(fibonacci_deltas(17, nb * 64, seed=seed))
    if table == "flat8":
        assert nb % 4 == 0
        d = np.repeat(np.arange(256, dtype=np.uint8), nb // 4)
        np.random.default_rng(seed).shuffle(d)
        return d
    if table == "long_tile":
        return _long_tile_symbols(nb, seed)
    raise KeyError(table)


def _image(symbols, gw, gh, nodelta):
    """The raster whose blocks (block order, 64 symbols each) carry `symbols`: the symbols are
    the pixels (MH_FLAG_NO_DELTA) or the per-block deltas."""
    v = symbols.reshape(-1, 64)
    if not nodelta:
        v = (np.cumsum(v.astype(np.uint16), axis=1) & 0xFF).astype(np.uint8)
    return np.ascontiguousarray(v.reshape(gh // 8, gw // 8, 8, 8).transpose(0, 2, 1, 3).reshape(gh, gw))


_CASES: dict = {}


def _frames(mh, oracle, shape, table, nodelta):
    """[(EncodedFrame, expected H x W raster)] x N_FRAMES, built once per module."""
    key = (shape, table, nodelta)
    if key in _CASES:
        return _CASES[key]
    gw, gh, W, H, _ = SHAPES[shape]
    bw, bh = gw // 8, gh // 8
    if table == "long_tile":
        assert bw * bh >= 64
        rows = -(-(1 << 14) // bw)
    else:
        rows = max(bh, -(-128 // bw))
        rows = -(-rows // 4) * 4
    out = []
    for s in range(N_FRAMES):
        img = _image(_symbols(table, bw * rows, 7 + s), gw, 8 * rows, nodelta)
        ef = mh.encode_frame(img, flags=mh.MH_FLAG_NO_DELTA if nodelta else 0).band(0, bh)
        assert (ef.width, ef.height) == (gw, gh)
        ef = dataclasses.replace(ef, width=W, height=H)
        t1, t2 = ef.tables()
        want = oracle.decode_frame_shader(ef.block_offsets, ef.codes, t1, t2, W, H, block_init=ef.block_init,
                                          delta=not nodelta)
        assert np.array_equal(want, img[:H, :W]), key
        want.setflags(write=False)
        out.append((ef, want))
    L = out[0][0].canon
    assert all(np.array_equal(ef.canon, L) for ef, _ in out), "one table per case"
    assert len({ef.codes.tobytes() for ef, _ in out}) == N_FRAMES, "the frames of a case differ"
    lens = L[L > 0]
    if table == "len14":
        assert lens.max() == 14
    elif table == "esc16":
        assert lens.max() == 16
    elif table == "flat8":
        assert lens.size == 256 and lens.min() == lens.max() == 8
    else:
        assert 14 <= L[128:].min() and L[128:].max() <= 16 and lens.max() <= 16, (L[128:].min(), lens.max())
        for ef, _ in out:  # tile 0 (blocks 0..63) cannot be staged whole
            o = ef.block_offsets.astype(np.int64)
            assert (o[64] - o[0]) // 8 > STAGE_BYTES
    _CASES[key] = out
    return out


@pytest.fixture(scope="module")
def cus(device):
    import torch
    return torch.cuda.get_device_properties(device).multi_processor_count


def _launch(frames, device, cus, pitch, extra_flags=0):
    """One mh_decode of `frames` = [(EncodedFrame, expected)] into a guarded buffer, not yet
    synchronised; -> (device buffer, plan, expected rasters)."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    efs = [f[0] for f in frames]
    n, W, H = len(efs), efs[0].width, efs[0].height
    tabs = D.DeviceTables.upload(*efs[0].tables(), device)
    assert tabs.lut is not None
    fr = D.DeviceFrames.pack(efs, device)
    # launch() in mh_decode.hip: the single-frame entry / the small-launch kernel
    assert fr.n_frames == n and (fr.frame_code_offsets is None) == (n == 1)
    assert -(-fr.n_blocks // 64) * n <= 4 * cus
    w8 = (W + 7) // 8 * 8
    stride = H * pitch
    plan = containment_plan(n, W, H, pitch, stride, 4096, 8 * pitch + 4096, written_cols=w8)
    buf = torch.from_numpy(plan.pattern.copy()).to(device)
    st = D._frame_struct(fr, tabs, extra_flags)
    N.check(N.lib().mh_decode(ctypes.byref(st), buf.data_ptr() + plan.d_out, pitch, stride,
                              torch.cuda.current_stream(device).cuda_stream), "mh_decode")
    return buf, plan, [f[1] for f in frames], (fr, tabs)


def _check(launched, device):
    import torch
    torch.cuda.synchronize(device)
    buf, plan, want, _ = launched
    check_containment(buf.cpu().numpy(), plan, want)


CASES = [(s, t, nd) for s in SHAPES for t in ("len14", "esc16", "flat8") for nd in (False, True)]
CASES += [(s, "long_tile", nd) for s in ("blocks65", "rows9") for nd in (False, True)]
IDS = [f"{s}-{t}-{'nodelta' if nd else 'delta'}" for s, t, nd in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_single_frame(mh, oracle, device, cus, case):
    """mh_decode_frame_kernel: one frame, prepared table, no frame-offset array."""
    frames = _frames(mh, oracle, *case)
    _check(_launch(frames[:1], device, cus, SHAPES[case[0]][4]), device)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_two_frame_small_launch(mh, oracle, device, cus, case):
    """mh_decode_small_kernel: two frames of the case in one launch (a frame-offset array); a
    row of frame 0 at or below H that is not dropped lands in frame 1."""
    frames = _frames(mh, oracle, *case)
    _check(_launch(frames[1:3], device, cus, SHAPES[case[0]][4]), device)


def test_largest_pitch(mh, oracle, device, cus):
    """64 x 72 at a pitch of 2^20, the API's largest: the loop's store offset reaches
    (7 * 8 + 7) * 2^20 in tile 0, and dead lanes' 2^31 + 7 * 2^20 stays out of range. One
    table and flag only: the raster is 72 MiB. Its guard bands and row padding hold a
    sentinel (the pattern-filled plan would need the buffer several times over in host memory)."""
    import torch
    ef, want = _frames(mh, oracle, "rows9", "len14", False)[0]
    from metalhuffman_amd import _native as N, decoder as D
    pitch, W, H, lead = 1 << 20, ef.width, ef.height, 4096
    tabs = D.DeviceTables.upload(*ef.tables(), device)
    fr = D.DeviceFrames.pack([ef], device)
    assert fr.frame_code_offsets is None and tabs.lut is not None
    buf = torch.full((lead + (H + 8) * pitch,), 0xA5, dtype=torch.uint8, device=device)
    st = D._frame_struct(fr, tabs)
    N.check(N.lib().mh_decode(ctypes.byref(st), buf.data_ptr() + lead, pitch, H * pitch,
                              torch.cuda.current_stream(device).cuda_stream), "mh_decode")
    torch.cuda.synchronize(device)
    assert bool((buf[:lead] == 0xA5).all()), "bytes in front of d_out were written"
    got = buf[lead:].view(H + 8, pitch)
    assert bool((got[H:] == 0xA5).all()), "rows below H were written"
    assert bool((got[:, W:] == 0xA5).all()), "columns beyond the row were written"
    assert np.array_equal(got[:H, :W].cpu().numpy(), want)


@pytest.mark.parametrize("shape", ["blocks65", "rows9"])
def test_any_order_three_frames(mh, oracle, device, cus, shape):
    """MH_FLAG_ANY_ORDER: three single-frame launches in a row on one stream, each into a
    guarded raster of its own, checked after one synchronise."""
    from metalhuffman_amd import _native as N
    frames = _frames(mh, oracle, shape, "len14", False)
    launched = [_launch(frames[i:i + 1], device, cus, SHAPES[shape][4], extra_flags=N.MH_FLAG_ANY_ORDER)
                for i in range(N_FRAMES)]
    for l in launched:
        _check(l, device)
