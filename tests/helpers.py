"""Shared helpers for the test suite (CPU and GPU)."""
from __future__ import annotations

import dataclasses
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden() -> dict:
    with open(os.path.join(GOLDEN, "golden.json")) as f:
        return json.load(f)


REF_HISTOGRAMS = os.path.join(GOLDEN, "ref_random_histograms.npz")


def random_histogram_streams(seed: int = 11, trials: int = 40):
    """(trial, symbols) of the tie-breaking stress: small alphabets with repeated
    frequencies, whole 64-symbol blocks. tests/golden/gen_golden.py records the reference
    encoder's output for each stream it accepts in REF_HISTOGRAMS (canon_<trial>,
    codes_<trial>, offsets_<trial>)."""
    r = np.random.default_rng(seed)
    for trial in range(trials):
        nsym = int(r.integers(1, 40))
        alphabet = r.choice(256, size=nsym, replace=False).astype(np.uint8)
        weights = r.integers(1, 6, size=nsym) ** r.integers(1, 4)
        yield trial, r.choice(alphabet, size=64 * int(r.integers(1, 50)), p=weights / weights.sum())


def image_from_block_deltas(deltas: np.ndarray, width: int, height: int) -> np.ndarray:
    """Integrate per-block deltas (block order, 64 per block) into a raster whose
    producer step (split + per-block delta) yields exactly `deltas`.
    width and height must be multiples of 8 (no pad region to reproduce)."""
    assert width % 8 == 0 and height % 8 == 0
    bw, bh = width // 8, height // 8
    d = deltas.reshape(bh * bw, 64).astype(np.uint16)
    vals = (np.cumsum(d, axis=1) & 0xFF).astype(np.uint8)
    return np.ascontiguousarray(vals.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(height, width))


def fibonacci_deltas(n_symbols: int, total: int, seed: int = 0) -> np.ndarray:
    """A delta stream whose histogram is Fibonacci-shaped over `n_symbols` symbols
    (deepest code = n_symbols - 1 bits), shuffled."""
    fib = [1, 1]
    while len(fib) < n_symbols:
        fib.append(fib[-1] + fib[-2])
    fib = np.array(fib[:n_symbols], dtype=np.int64)
    reps = max(1, total // int(fib.sum()))
    counts = fib * reps
    syms = np.repeat(np.arange(n_symbols, dtype=np.uint8)[::-1], counts)
    out = np.zeros(total, np.uint8)
    out[: min(total, syms.size)] = syms[:total]
    np.random.default_rng(seed).shuffle(out)
    return out


def long_span_deltas(width: int, height: int, seed: int = 0) -> np.ndarray:
    """Mostly-zero deltas with every rare symbol packed into the FIRST tile
    (64 blocks): that tile's code span exceeds the kernel's LDS window and takes the
    global-memory path, while every code stays <= 16 bits."""
    nb = (width // 8) * (height // 8)
    d = np.zeros(nb * 64, np.uint8)
    r = np.random.default_rng(seed)
    first = 64 * 64
    rare = r.integers(1, 256, size=first, dtype=np.uint8)
    d[:first] = rare
    return d


def shift_stream(ef, k: int):
    """The same frame with its code stream moved k bits later (k leading zero bits) and
    every block offset with it: blocks off the byte grid, which no reference producer
    writes but the buffer contract allows."""
    from metalhuffman_amd import _native as N
    bits = np.unpackbits(ef.codes[: ef.payload_bytes])
    moved = np.packbits(np.concatenate([np.zeros(k, np.uint8), bits]))
    codes = np.concatenate([moved, np.zeros(N.MH_CODES_PAD, np.uint8)])
    return dataclasses.replace(ef, codes=codes, block_offsets=(ef.block_offsets + np.uint32(k)).astype(np.uint32))


def lane_pair_oversize_deltas(seed: int = 0) -> np.ndarray:
    """512x512 deltas whose first 32 blocks hold 249 rare symbols x 8 (15-bit codes under
    a geometric chain of 7 common symbols): that 32-block lane-pair tile spans 3,735 B,
    more than round 2's 3,712-B lane-pair stage, with codes above 14 bits
    (the 13-bit table with escapes)."""
    n = 512 * 512
    r = np.random.default_rng(seed)
    rare = np.repeat(np.arange(7, 256, dtype=np.uint8), 8)
    head = np.zeros(2048, np.uint8)
    head[: rare.size] = rare
    r.shuffle(head)
    rest = np.repeat(np.arange(7, dtype=np.uint8), [n >> (k + 1) for k in range(7)])[: n - 2048]
    rest = np.concatenate([rest, np.zeros(n - 2048 - rest.size, np.uint8)])
    r.shuffle(rest)
    return np.concatenate([head, rest])


def refill_extreme_deltas(n_symbols: int, width: int, height: int, seed: int = 0) -> np.ndarray:
    """Deltas with a Fibonacci histogram over `n_symbols` symbols (deepest code
    n_symbols - 1 bits) rearranged so that many blocks hold a prefix of p short codes
    (p = 0..32, every bit alignment of the cursor) followed by a run of the LONGEST codes:
    the decoders' refill points then see the cursor at its deepest (sh up to 47 bits into
    the 64-bit window). The histogram, hence the code lengths, is unchanged."""
    nb = (width // 8) * (height // 8)
    d = fibonacci_deltas(n_symbols, nb * 64, seed=seed)
    vals, counts = np.unique(d, return_counts=True)
    order = np.argsort(counts, kind="stable")          # rarest (longest code) first
    rare = np.concatenate([np.full(counts[i], vals[i], np.uint8) for i in order])
    common = int(vals[order[-1]])                      # the 1-bit code
    out = np.empty(nb * 64, np.uint8)
    r_i = 0
    pool = []
    for b in range(nb):
        p = b % 33
        blk = np.full(64, common, np.uint8)
        take = min(64 - p, rare.size - r_i)
        blk[p:p + take] = rare[r_i:r_i + take]
        r_i += take
        out[b * 64:(b + 1) * 64] = blk
    # the histogram must match the Fibonacci one: the loop above used at most the rare
    # symbols once each; top up / trim the common symbol so the multiset is d's
    want = np.bincount(d, minlength=256)
    have = np.bincount(out, minlength=256)
    diff = want[common] - have[common]
    if diff < 0:  # too many common symbols: put the unused rare ones back in their place
        left = rare[r_i:]
        idx = np.nonzero(out == common)[0][-left.size:] if left.size else np.array([], np.int64)
        out[idx] = left
        pool = left
    assert np.array_equal(np.bincount(out, minlength=256), want), "histogram changed"
    return out


# ---- write containment (include/metalhuffman.h: where a decode may store) -------------
#
# A decode of n frames into d_out with a caller's pitch and frame stride may write frame
# f, row y < H, columns [0, written_cols) and nothing else. containment_plan lays such a
# raster out inside one buffer with guard bytes in front of and behind it, filled with a
# position-dependent pattern; check_containment then looks at every byte of the buffer.


@dataclasses.dataclass(frozen=True)
class ContainmentPlan:
    n_frames: int
    W: int
    H: int
    pitch: int
    stride: int
    lead: int
    tail: int
    written_cols: int
    size: int                 # bytes of the whole buffer
    d_out: int                # offset of d_out inside it (= lead)
    pattern: np.ndarray       # u8[size]: the fill
    may_write: np.ndarray     # bool[size]: frame f, row y < H, columns [0, written_cols)

    def frame_view(self, buf: np.ndarray, cols: int) -> np.ndarray:
        """[n_frames, H, cols] view of buf's rasters (no copy)."""
        return np.lib.stride_tricks.as_strided(buf[self.d_out:], (self.n_frames, self.H, cols),
                                               (self.stride, self.pitch, 1), writeable=buf.flags.writeable)


def containment_plan(n_frames: int, W: int, H: int, pitch: int, stride: int, lead: int, tail: int,
                     written_cols: int) -> ContainmentPlan:
    """Buffer layout for a decode of n_frames W x H frames at d_out = buffer + lead, rows
    `pitch` apart and frames `stride` apart, followed by `tail` guard bytes behind the last
    frame's last row. written_cols: round_up(W, 8) for the GPU decoder (whole 8-pixel block
    rows), W for the CPU decoder."""
    assert n_frames >= 1 and W >= 1 and H >= 1 and lead >= 0 and tail >= 0
    assert W <= written_cols <= pitch, "rows must not overlap"
    assert n_frames == 1 or stride >= H * pitch, "frames must not overlap"
    size = lead + (n_frames - 1) * stride + H * pitch + tail
    pattern = ((np.arange(size, dtype=np.uint64) * 167 + 13) & 0xFF).astype(np.uint8)
    may = np.zeros(size, bool)
    np.lib.stride_tricks.as_strided(may[lead:], (n_frames, H, written_cols), (stride, pitch, 1))[...] = True
    assert int(may.sum()) == n_frames * H * written_cols
    pattern.setflags(write=False)
    may.setflags(write=False)
    return ContainmentPlan(n_frames, W, H, pitch, stride, lead, tail, written_cols, size, lead, pattern, may)


def _containment_region(plan: ContainmentPlan, i: int) -> str:
    """Where byte i of the buffer (outside the may-write mask) lies, in words."""
    if i < plan.lead:
        return f"lead guard, {plan.lead - i} byte(s) in front of d_out"
    rel = i - plan.lead
    f = min(rel // plan.stride, plan.n_frames - 1) if plan.n_frames > 1 else 0
    r = rel - f * plan.stride
    y, x = divmod(r, plan.pitch)
    where = f"frame {f}, row {y}, column {x}"
    if y < plan.H:
        return f"row padding (columns >= {plan.written_cols}), {where}"
    if y < -(-plan.H // 8) * 8 and x < plan.written_cols:
        return f"rows below H (a block row's rows >= {plan.H}), {where}"
    if f < plan.n_frames - 1:
        return f"inter-frame gap behind frame {f}, {where}"
    return f"tail guard behind the last frame, {where}"


def check_containment(buf_after: np.ndarray, plan: ContainmentPlan, expected_frames) -> None:
    """Assert that buf_after (the plan's buffer after a decode) holds the fill pattern at
    every byte the decode may not write, and expected_frames[f] (H x W) in columns [0, W)
    of every frame row. Columns [W, written_cols) are written with unspecified bytes."""
    buf = np.asarray(buf_after)
    assert buf.dtype == np.uint8 and buf.shape == (plan.size,), (buf.dtype, buf.shape)
    assert len(expected_frames) == plan.n_frames
    bad = np.flatnonzero((buf != plan.pattern) & ~plan.may_write)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"write outside the raster: {_containment_region(plan, i)}; first offending byte at "
                             f"buffer offset {i} (d_out{i - plan.d_out:+d}): {int(buf[i]):#04x}, the fill is "
                             f"{int(plan.pattern[i]):#04x}; {bad.size} byte(s) in all, last at offset {int(bad[-1])}")
    got = plan.frame_view(buf, plan.W)
    for f in range(plan.n_frames):
        want = np.asarray(expected_frames[f])
        assert want.shape == (plan.H, plan.W), (f, want.shape)
        if not np.array_equal(got[f], want):
            ys, xs = np.nonzero(got[f] != want)
            y, x = int(ys[0]), int(xs[0])
            i = plan.d_out + f * plan.stride + y * plan.pitch + x
            raise AssertionError(f"wrong pixel: frame {f}, row {y}, column {x}, buffer offset {i}: "
                                 f"{int(got[f, y, x]):#04x}, expected {int(want[y, x]):#04x}; "
                                 f"{ys.size} wrong pixel(s) in this frame")
