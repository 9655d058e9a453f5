"""Write containment on the CPU: the harness of helpers.py itself, and mh_decode_frame_cpu.

include/metalhuffman.h says where a decode may store: frame f, row y < H, and of that row
round_up(W, 8) bytes (GPU) or W bytes (the CPU twin); "the rest of the pitch and rows >= H
are not touched". helpers.containment_plan lays a raster with a caller's pitch and frame
stride out inside a pattern-filled buffer with guards around it, helpers.check_containment
looks at every byte afterwards. The first half of this file shows that the checker rejects
a buffer that is wrong in exactly one byte, wherever that byte lies -- the evidence that
the GPU cases of test_gpu_write_containment.py can fail. The second half runs the CPU
frame decoder through it with out_pitch > W, which no other test does.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import pytest

from helpers import check_containment, containment_plan, fibonacci_deltas, image_from_block_deltas

# 3 frames of 93 x 50 (round_up(W, 8) = 96) at pitch 136, 3 rows + 40 bytes between frames
N, W, H, PITCH, LEAD, TAIL = 3, 93, 50, 136, 4096 + 8, 8 * 136 + 4096
STRIDE = H * PITCH + 3 * PITCH + 40


def _plan(written_cols=96):
    return containment_plan(N, W, H, PITCH, STRIDE, LEAD, TAIL, written_cols)


def _expected():
    r = np.random.default_rng(1)
    return [r.integers(0, 256, size=(H, W), dtype=np.uint8) for _ in range(N)]


def _correct(plan, expected):
    """What a correct decode leaves: the fill, the frames, and other bytes in [W, written_cols)."""
    buf = plan.pattern.copy()
    plan.frame_view(buf, plan.W)[...] = np.stack(expected)
    if plan.written_cols > plan.W:
        plan.frame_view(buf, plan.written_cols)[:, :, plan.W:] ^= 0x5A
    return buf


def test_plan_layout():
    plan = _plan()
    assert plan.d_out == LEAD and plan.size == LEAD + (N - 1) * STRIDE + H * PITCH + TAIL
    assert plan.pattern.shape == plan.may_write.shape == (plan.size,)
    assert len(np.unique(plan.pattern)) == 256 and plan.pattern[0] != plan.pattern[1]
    m = plan.may_write
    assert int(m.sum()) == N * H * 96
    assert not m[:LEAD].any() and not m[plan.size - TAIL:].any()
    for f in range(N):
        o = LEAD + f * STRIDE
        assert m[o] and m[o + 95] and not m[o + 96] and not m[o + PITCH - 1]
        assert m[o + (H - 1) * PITCH + 95] and not m[o + H * PITCH: o + H * PITCH + 96].any()
    # the CPU decoder's plan stops at W
    assert int(_plan(W).may_write.sum()) == N * H * W


def test_checker_accepts_a_correct_buffer():
    plan, exp = _plan(), _expected()
    buf = _correct(plan, exp)
    check_containment(buf, plan, exp)
    # any value in [W, round_up(W, 8)): written, but the header does not say with what
    for v in (0x00, 0xFF):
        plan.frame_view(buf, 96)[:, :, W:] = v
        check_containment(buf, plan, exp)
    plan.frame_view(buf, 96)[:, :, W:] = plan.frame_view(plan.pattern.copy(), 96)[:, :, W:]  # left untouched
    check_containment(buf, plan, exp)


# (case, byte offset relative to d_out, what the message must name)
ONE_BYTE = [
    ("before_d_out", -1, ["lead guard", f"offset {LEAD - 1}"]),
    ("row_padding", 7 * PITCH + 96, ["row padding", "frame 0", "row 7", "column 96"]),
    ("row_padding_last_column", STRIDE + 49 * PITCH + PITCH - 1, ["row padding", "frame 1", "row 49", "column 135"]),
    ("row_H_of_frame_0", H * PITCH, ["rows below H", "frame 0", f"row {H}", "column 0"]),
    ("row_55_of_last_frame", 2 * STRIDE + 55 * PITCH + 95, ["rows below H", "frame 2", "row 55", "column 95"]),
    ("inter_frame_gap", 51 * PITCH + 100, ["inter-frame gap", "frame 0", "row 51", "column 100"]),
    ("inter_frame_gap_last_byte", STRIDE - 1, ["rows below H", "frame 0", "row 53", "column 39"]),
    ("inter_frame_gap_beside_row_H", STRIDE + H * PITCH + 96, ["inter-frame gap", "frame 1", f"row {H}"]),
    ("tail_first_block_row_below", 2 * STRIDE + 56 * PITCH, ["tail guard", "frame 2", "row 56"]),
    ("tail_last_byte", 2 * STRIDE + H * PITCH + TAIL - 1, ["tail guard"]),
]


@pytest.mark.parametrize("case", ONE_BYTE, ids=[c[0] for c in ONE_BYTE])
def test_checker_rejects_one_stray_byte(case):
    _, rel, names = case
    plan, exp = _plan(), _expected()
    buf = _correct(plan, exp)
    i = LEAD + rel
    assert not plan.may_write[i]
    buf[i] ^= 0x01
    with pytest.raises(AssertionError) as e:
        check_containment(buf, plan, exp)
    msg = str(e.value)
    for name in names + [f"offset {i} "]:
        assert name in msg, (name, msg)
    buf[i] ^= 0x01
    check_containment(buf, plan, exp)


def test_checker_rejects_one_wrong_pixel():
    plan, exp = _plan(), _expected()
    buf = _correct(plan, exp)
    for f, y, x in ((0, 0, 0), (1, 49, 92), (2, 17, 5)):
        i = LEAD + f * STRIDE + y * PITCH + x
        buf[i] ^= 0x80
        with pytest.raises(AssertionError) as e:
            check_containment(buf, plan, exp)
        msg = str(e.value)
        for name in ("wrong pixel", f"frame {f}", f"row {y}", f"column {x}", f"offset {i}"):
            assert name in msg, (name, msg)
        buf[i] ^= 0x80
    check_containment(buf, plan, exp)


def test_checker_sees_a_store_that_equals_a_constant_fill():
    """Why the fill depends on the position: decoded bytes that land outside the raster are
    seen whatever their value, unless they equal the pattern at that very byte."""
    plan, exp = _plan(), _expected()
    i = LEAD + H * PITCH + 8
    for v in range(256):
        buf = _correct(plan, exp)
        buf[i: i + 8] = v            # an 8-byte row store one row too low
        with pytest.raises(AssertionError):
            check_containment(buf, plan, exp)


def test_tight_geometry_has_no_gap():
    """pitch = round_up(W, 8), stride = H * pitch: every byte between d_out and the tail may be
    written, and row H of frame 0 IS row 0 of frame 1 -- only its pixels can tell."""
    plan = containment_plan(2, W, H, 96, H * 96, 256, 4096, 96)
    assert plan.may_write[256: 256 + 2 * H * 96].all() and int(plan.may_write.sum()) == 2 * H * 96
    exp = _expected()[:2]
    buf = _correct(plan, exp)
    check_containment(buf, plan, exp)
    buf[256 + H * 96] ^= 1
    with pytest.raises(AssertionError, match="wrong pixel: frame 1, row 0, column 0"):
        check_containment(buf, plan, exp)
    buf[256 + H * 96] ^= 1
    buf[256 + 2 * H * 96] ^= 1
    with pytest.raises(AssertionError, match="rows below H"):
        check_containment(buf, plan, exp)


# ---- mh_decode_frame_cpu with a caller's pitch ----------------------------------------

_u8p = ctypes.POINTER(ctypes.c_uint8)
_u32p = ctypes.POINTER(ctypes.c_uint32)


def _decode_cpu_into(mh, ef, plan, threads):
    """mh_decode_frame_cpu through ctypes (as codec.decode_frame_cpu calls it) into the
    plan's pattern-filled buffer at d_out with plan.pitch; returns the buffer."""
    from metalhuffman_amd import _native as NAT
    t1, t2 = ef.tables()
    buf = plan.pattern.copy()
    offs = np.ascontiguousarray(ef.block_offsets, np.uint32)
    init = np.ascontiguousarray(ef.block_init, np.uint8) if ef.block_init is not None else None
    out = ctypes.cast(buf.ctypes.data + plan.d_out, _u8p)
    NAT.check(NAT.lib().mh_decode_frame_cpu(
        offs.ctypes.data_as(_u32p), ef.codes.ctypes.data_as(_u8p), ef.codes.size, t1.ctypes.data_as(_u8p),
        t2.ctypes.data_as(_u8p), t2.size // 2, init.ctypes.data_as(_u8p) if init is not None else None,
        ef.width, ef.height, ef.flags, out, plan.pitch, int(threads)), "mh_decode_frame_cpu")
    return buf


def _oracle_decode(O, ef):
    t1, t2 = ef.tables()
    return O.decode_frame_shader(ef.block_offsets, ef.codes, t1, t2, ef.width, ef.height,
                                 block_init=ef.block_init, delta=not (ef.flags & 1))


@pytest.fixture(scope="module")
def frame_93x50(mh, oracle):
    """A 96 x 56 block grid (84 blocks, 16-bit codes) declared 93 x 50: both edges cropped."""
    img = image_from_block_deltas(fibonacci_deltas(17, 84 * 64, seed=1), 96, 56)
    ef = mh.encode_frame(img)
    assert ef.canon.max() == 16
    ef = dataclasses.replace(ef, width=W, height=H)
    want = _oracle_decode(oracle, ef)
    assert np.array_equal(want, img[:H, :W])
    return ef, want


@pytest.fixture(scope="module")
def frame_wide(mh, oracle, bigbridge):
    """141 x 21: 18 blocks per block row = two groups of kGroup = 8 full-width blocks
    (decode_group), one single full block and a 5-pixel partial block (decode_block); three
    block rows, the last with 5 pixel rows; per-block init bytes."""
    img = np.ascontiguousarray(bigbridge[300:321, 500:641])
    ef = mh.encode_frame(img, init_zero_delta=True)
    assert (ef.block_width, ef.block_height) == (18, 3) and ef.width // 64 == 2
    # group_fast (mh_cpu.cpp): the group's last root is 144 bytes or more from the end
    for b in (0, 8, 18, 26):
        assert (int(ef.block_offsets[b: b + 8].max()) >> 3) + 8 + 136 <= ef.codes.size, b
    want = _oracle_decode(oracle, ef)
    assert np.array_equal(want, img)
    return ef, want


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("pitch", [93, 136])
def test_cpu_decoder_93x50(mh, frame_93x50, pitch, threads):
    """Rows 50..55 and columns 93..95 of the block grid are decoded but must not be stored."""
    ef, want = frame_93x50
    plan = containment_plan(1, W, H, pitch, H * pitch, 4096 + 8, 8 * pitch + 4096, written_cols=W)
    check_containment(_decode_cpu_into(mh, ef, plan, threads), plan, [want])


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("pitch", [141, 200])
def test_cpu_decoder_block_groups(mh, frame_wide, pitch, threads):
    """decode_group's 64-byte row copies and the single blocks beside them."""
    ef, want = frame_wide
    plan = containment_plan(1, ef.width, ef.height, pitch, ef.height * pitch, 4096 + 8, 8 * pitch + 4096,
                            written_cols=ef.width)
    check_containment(_decode_cpu_into(mh, ef, plan, threads), plan, [want])
