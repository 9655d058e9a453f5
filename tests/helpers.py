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


def place_stream(ef, lead_bytes: int):
    """The same frame with `lead_bytes` zero bytes in front of its codes and 8 * lead_bytes added
    to every block offset -> (payload, offsets, total): the frame's own bytes (MH_CODES_PAD
    included), which belong at [lead_bytes, total) of an otherwise zero buffer of `total` bytes,
    and the u32 block offsets into that buffer. The lead is not materialised."""
    lead_bytes = int(lead_bytes)
    assert lead_bytes >= 0
    offs = ef.block_offsets.astype(np.uint64) + np.uint64(8 * lead_bytes)
    assert int(offs[-1]) < 2 ** 32, "block offsets are u32"
    return ef.codes, offs.astype(np.uint32), lead_bytes + int(ef.codes.size)


def placed_host_frame(ef, lead_bytes: int):
    """place_stream materialised on the host: an EncodedFrame over np.zeros(total) with only the
    tail written (the untouched lead costs no memory)."""
    payload, offs, total = place_stream(ef, lead_bytes)
    codes = np.zeros(total, np.uint8)
    codes[lead_bytes:] = payload
    return dataclasses.replace(ef, codes=codes, block_offsets=offs)


def lead_top(ef, aligned: bool = False) -> int:
    """The `top` placement: the largest lead at which the stream's last code bit still lies below
    2^32 and the lead is no multiple of 16 (the first tile's 16-byte aligned span start then
    differs from its first byte). The last block's offset lies in (2^32 - 1024, 2^32), so the
    u32 sum offset + 1024 wraps. One kind of frame cannot have both: a last block of exactly
    1024 bits (64 codes of 16 bits) ends below 2^32 only from offset 2^32 - 1024 down, where the
    sum wraps to exactly 0 and the lead is a multiple of 16 when the whole frame is 16-bit codes.
    For such a frame `top` keeps the odd lead (offset 2^32 - 1032, the largest sum that does not
    wrap) and aligned=True gives the other half, lead % 16 == 0 at offset 2^32 - 1024."""
    return lead_top_bits(int(ef.block_offsets[-1]), 8 * ef.payload_bytes, aligned)


def lead_top_bits(last: int, end_bits: int, aligned: bool = False) -> int:
    """lead_top from the last block's offset and the payload's bit count (whole bytes)."""
    assert 0 < end_bits - last <= 1024 + 7 and end_bits % 8 == 0
    lead = (2 ** 32 - end_bits) // 8
    full = end_bits - last == 1024
    if aligned:
        assert full and lead % 16 == 0 and 8 * lead + last == 2 ** 32 - 1024
        return lead
    if lead % 16 == 0:
        lead -= 1
    assert lead % 16 != 0 and 8 * lead + end_bits <= 2 ** 32
    if full:
        assert 8 * lead + last == 2 ** 32 - 1032
    else:
        assert 2 ** 32 - 1024 < 8 * lead + last < 2 ** 32
    return lead


def lead_mid(ef) -> int:
    """The `mid` placement: block offsets straddle 2^31 inside tile 0 -- the tile's first block
    starts below the boundary and its last block (block 63, or the frame's last) at or above it."""
    offs = ef.block_offsets.astype(np.int64)
    t0_last = min(63, offs.size - 1)
    lead = (2 ** 31 - int(offs[t0_last // 2 + 1])) // 8 + 1
    placed = offs + 8 * lead
    assert placed[0] < 2 ** 31 <= placed[t0_last] <= placed[-1] < 2 ** 32
    return lead


def exactly_uniform_image(width: int, height: int, seed: int, device=None):
    """A u8 [height, width] image in which every byte value occurs equally often (+-1 when the
    pixel count is no multiple of 256): every run of 256 pixels in raster order is the bijection
    j -> (j * odd_r + c_r) & 0xFF of 0..255 with a run's own odd multiplier and offset. A torch
    tensor on `device`, or (device=None) a numpy array. The counts are asserted."""
    import torch
    n = width * height
    runs = -(-n // 256)
    g = torch.Generator().manual_seed(seed)
    odd = (torch.randint(0, 128, (runs, 1), generator=g, dtype=torch.int32) * 2 + 1).to(torch.uint8)
    c = torch.randint(0, 256, (runs, 1), generator=g, dtype=torch.int32).to(torch.uint8)
    dev = torch.device("cpu") if device is None else device
    j = torch.arange(256, dtype=torch.int32).to(torch.uint8).to(dev)[None, :]
    flat = (j * odd.to(dev) + c.to(dev)).reshape(-1)[:n]      # u8 arithmetic: modulo 256
    assert flat.dtype == torch.uint8 and flat.numel() == n
    counts = torch.zeros(256, dtype=torch.int64, device=dev)
    for lo in range(0, n, 1 << 26):
        counts += torch.bincount(flat[lo: lo + (1 << 26)].to(torch.int32), minlength=256)
    assert int(counts.sum()) == n and int(counts.min()) >= n // 256 and int(counts.max()) <= -(-n // 256), \
        (int(counts.min()), int(counts.max()))
    img = flat.reshape(height, width)
    return img if device is not None else img.numpy()


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


# ---- frames under a chosen canonical header, and a zoo of headers ------------------------------
#
# The decoders are a function of the frame's 256 code lengths. The product's encoders only ever
# emit Huffman-optimal lengths; encode_with_header packs a frame under ANY valid header
# (lengths <= 16, Kraft sum <= 1), and header_zoo is a deterministic collection of such headers:
# random complete codes, incomplete ones, hand-written extremes and headers that must be rejected.

PREPARED_L13_BYTES = 18464                            # 13-bit table: 8192 first-level + 1040 second-level u16
PREPARED_L14_BYTES = 32768                            # single-level 14-bit table
PREPARED_WORD_OFF = PREPARED_L13_BYTES + PREPARED_L14_BYTES   # u32[4]: longest, shortest, flat8, 0
PREPARED_BYTES = PREPARED_WORD_OFF + 16


def encode_with_header(canon, deltas, width, height, *, no_delta=False, init_zero_delta=False):
    """An EncodedFrame of `deltas` (block order, 64 per block, as image_from_block_deltas takes
    them) under the canonical header `canon`, which need not be the Huffman code of the data:
    codes from oracle.canonical_codes, packed MSB-first, the last byte zero-filled, MH_CODES_PAD
    zero bytes behind it, one bit offset per 64 symbols. no_delta: the symbols are the pixels
    (the image is the block merge of `deltas`); init_zero_delta: the first delta of every block
    travels in block_init and a zero symbol takes its place. Every symbol that is encoded must
    have a code."""
    from oracle import oracle as O
    from metalhuffman_amd import _native as N
    from metalhuffman_amd.codec import EncodedFrame
    assert width % 8 == 0 and height % 8 == 0 and not (no_delta and init_zero_delta)
    canon = np.array(canon, np.uint8)   # a copy: the frame owns a writable header
    nb = (width // 8) * (height // 8)
    sym = np.array(deltas, np.uint8).reshape(nb, 64)
    init = None
    if init_zero_delta:
        init = sym[:, 0].copy()
        sym[:, 0] = 0
    sym = sym.reshape(-1)
    lens = canon[sym].astype(np.int64)
    assert canon.shape == (256,) and canon.max() <= 16 and (lens > 0).all(), "a symbol without a code"
    codes16 = O.canonical_codes(canon)[sym].astype(np.uint32)           # left-justified in 16 bits
    start = np.concatenate([[0], np.cumsum(lens)])
    k = np.arange(16, dtype=np.uint32)
    bits = ((codes16[:, None] >> (15 - k)[None, :]) & 1).astype(np.uint8)
    stream = bits[k[None, :] < lens[:, None]]                           # row-major: symbol order, MSB first
    assert stream.size == start[-1] < 2 ** 32
    payload = np.packbits(stream)                                       # zero-fills the last byte
    codes = np.concatenate([payload, np.zeros(N.MH_CODES_PAD, np.uint8)])
    flags = N.MH_FLAG_NO_DELTA if no_delta else 0
    return EncodedFrame(width, height, canon, codes, start[:-1:64].astype(np.uint32), init, flags)


def image_of_symbols(deltas, width, height, *, no_delta=False) -> np.ndarray:
    """The raster a frame of encode_with_header(canon, deltas, ...) decodes to."""
    if not no_delta:
        return image_from_block_deltas(np.asarray(deltas, np.uint8), width, height)
    bw, bh = width // 8, height // 8
    return np.ascontiguousarray(np.asarray(deltas, np.uint8).reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3)
                                .reshape(height, width))


def frame_under_header(canon, width, height, seed, *, no_delta=False, init_zero_delta=False):
    """(EncodedFrame, image): symbols drawn uniformly from the header's used symbols; with
    init_zero_delta every block's first delta is any byte (it travels outside the codes)."""
    r = np.random.default_rng(seed)
    used = np.flatnonzero(np.asarray(canon)).astype(np.uint8)
    nb = (width // 8) * (height // 8)
    d = r.choice(used, nb * 64)
    if init_zero_delta:
        d.reshape(nb, 64)[:, 0] = r.integers(0, 256, nb, dtype=np.uint8)
    ef = encode_with_header(canon, d, width, height, no_delta=no_delta, init_zero_delta=init_zero_delta)
    return ef, image_of_symbols(d, width, height, no_delta=no_delta)


def kraft_sum(canon) -> int:
    """Sum of 2^(16 - length) over the used lengths <= 16 (65536: a complete code)."""
    c = np.asarray(canon).astype(np.int64)
    c = c[(c > 0) & (c <= 16)]
    return int((1 << (16 - c)).sum())


def long_prefixes(canon) -> int:
    """13-bit prefixes taken by codes longer than 13 bits: ceil((4 n14 + 2 n15 + n16) / 8)."""
    c = np.asarray(canon)
    return -(-(4 * int((c == 14).sum()) + 2 * int((c == 15).sum()) + int((c == 16).sum())) // 8)


@dataclasses.dataclass(frozen=True)
class ZooHeader:
    name: str
    kind: str                 # "random", "incomplete", "hand", "rejected"
    canon: np.ndarray         # u8[256], read-only
    status: int               # what the device builders report: 0, -3 (a length over 16), -5 (Kraft sum over 1)

    @property
    def longest(self) -> int:
        return int(self.canon.max())


def _split_lengths(r, nsym, depth, bias):
    """Leaf depths of a random binary tree with nsym leaves, none deeper than `depth`: start
    with one leaf and split a leaf shallower than `depth` -- the deepest such with probability
    `bias`, else any -- until there are nsym. A full tree: the Kraft sum is exactly 1."""
    assert 2 <= nsym <= (1 << depth)
    count = np.zeros(depth + 1, np.int64)   # leaves per depth: which leaf of a depth splits makes no difference
    count[0] = 1
    for _ in range(nsym - 1):
        ok = np.flatnonzero(count[:depth])
        if r.random() < bias:
            d = int(ok[-1])
        else:
            d = int(r.choice(ok, p=count[ok] / count[ok].sum()))
        count[d] -= 1
        count[d + 1] += 2
    return np.repeat(np.arange(depth + 1, dtype=np.uint8), count)


def _deal(lengths, perm) -> np.ndarray:
    canon = np.zeros(256, np.uint8)
    canon[perm[: len(lengths)]] = lengths
    canon.setflags(write=False)
    return canon


HAND_HEADERS = {  # name -> {length: how many symbols}
    "14x2": {14: 2}, "14x256": {14: 256}, "15x256": {15: 256}, "16x256": {16: 256}, "15x1_16x2": {15: 1, 16: 2},
    "13x3": {13: 3}, "8x255": {8: 255}, "8x256": {8: 256}, "1x1": {1: 1}, "1x1_9x255": {1: 1, 9: 255},
    "8x255_16x1": {8: 255, 16: 1}, "1x1_16x255": {1: 1, 16: 255}, "2x3_16x253": {2: 3, 16: 253},
    "13_14_15_16x2": {13: 1, 14: 1, 15: 1, 16: 2},
    "1to15_16x2": {**{l: 1 for l in range(1, 16)}, 16: 2},
    "1to13_14x2": {**{l: 1 for l in range(1, 14)}, 14: 2},
}
ZOO_SEED = 8
ZOO_RANDOM = 400
_ZOO: dict = {}


def header_zoo(seed: int = ZOO_SEED) -> list:
    """The header zoo, the same list for the same seed: ZOO_RANDOM random complete codes
    ("rnd<i>"), an incomplete variant of every 8th ("inc<i>": a random quarter of its symbols
    dropped), the hand-written extremes under two dealings of the lengths to symbols ("<name>/a":
    ascending lengths on symbols 0, 1, ...; "/b": a random permutation), and rejected headers."""
    if seed in _ZOO:
        return _ZOO[seed]
    r = np.random.default_rng(seed)
    zoo = []
    for i in range(ZOO_RANDOM):
        nsym = int(r.integers(2, 257))
        depth = int(r.integers(max(1, int(np.ceil(np.log2(nsym)))), 17))
        lengths = _split_lengths(r, nsym, depth, float(r.random()))
        zoo.append(ZooHeader(f"rnd{i}", "random", _deal(lengths, r.permutation(256)), 0))
    for i in range(0, ZOO_RANDOM, 8):
        g = zoo[i].canon.copy()
        used = np.flatnonzero(g)
        g[r.choice(used, max(1, used.size // 4), replace=False)] = 0
        g.setflags(write=False)
        zoo.append(ZooHeader(f"inc{i}", "incomplete", g, 0))
    for name, spec in HAND_HEADERS.items():
        lengths = np.repeat(np.array(sorted(spec), np.uint8), [spec[l] for l in sorted(spec)])
        zoo.append(ZooHeader(name + "/a", "hand", _deal(lengths, np.arange(256)), 0))
        zoo.append(ZooHeader(name + "/b", "hand", _deal(lengths, r.permutation(256)), 0))

    def rejected(name, base, changes, status):
        g = np.array(base, np.uint8)
        for s, l in changes.items():
            g[s] = l
        g.setflags(write=False)
        zoo.append(ZooHeader(name, "rejected", g, status))

    room = next(z.canon for z in zoo if z.kind == "random" and 8 <= int((z.canon > 0).sum()) <= 200)
    free = np.flatnonzero(room == 0)
    rejected("complete+16", room, {int(free[0]): 16}, -5)              # Kraft sum 65537
    rejected("three_1bit", np.zeros(256), {1: 1, 2: 1, 3: 1}, -5)
    for long in (17, 32, 128, 255):                                    # one length over 16, the rest valid
        rejected(f"len{long}", room, {int(free[long % free.size]): long}, -3)
    rejected("len200_oversubscribed", room, {int(free[1]): 1, int(free[2]): 200}, -3)   # too-long wins
    _ZOO[seed] = zoo
    return zoo


def zoo_accepted(seed: int = ZOO_SEED) -> list:
    return [z for z in header_zoo(seed) if z.status == 0]


def prepared_table_reference(O, canon, status: int = 0) -> np.ndarray:
    """u8[PREPARED_BYTES]: what the prepared table of a header must contain, stated plainly from
    the oracle's 65,536-entry {symbol, length} table T (not from T1/T2). step(e) = ((symbol << 8)
    - length) & 0xFFFF for a length > 0, else 0.
      13-bit table, first level: P0 = the smallest 13-bit prefix p whose window p << 3 decodes a
        code longer than 13 bits (8192 when there is none); entry p < P0 is step(T[p << 3]); entry
        p >= P0 is the escape p - P0 + 1 while that is below 129, else 0.
      second level (1040 entries): 0..7 zero; 8 + j = step(T[(P0 << 3) + j]) for
        j < min((8192 - P0) * 8, 1024); the rest zero.
      14-bit table: entry q = step(T[q << 2]) when that length is <= 14, else 0.
      lengths word: [longest, shortest non-zero length over T[q << 2] (0 and 255 when there is
        none), flat8 = 1 only for all 256 symbols at 8 bits, 0].
    A rejected header (status != 0): all-zero tables and the word [0, 255, 0, 0]."""
    out = np.zeros(PREPARED_BYTES, np.uint8)
    word = out[PREPARED_WORD_OFF:].view(np.uint32)
    if status != 0:
        word[:] = [0, 255, 0, 0]
        return out
    canon = np.asarray(canon, np.uint8)
    T = O.single_table(canon).view(np.uint16).astype(np.uint32)
    sym, ln = T & 0xFF, T >> 8
    step = np.where(ln > 0, ((sym << 8) - ln) & 0xFFFF, 0).astype(np.uint16)
    p = np.arange(8192)
    long13 = np.flatnonzero(ln[p << 3] > 13)
    P0 = int(long13[0]) if long13.size else 8192
    l13 = out[:PREPARED_L13_BYTES].view(np.uint16)
    sub = p - P0 + 1
    l13[:8192] = np.where(p < P0, step[p << 3], np.where(sub < 129, sub, 0))
    n2 = min((8192 - P0) * 8, 1024)
    l13[8192 + 8: 8192 + 8 + n2] = step[(P0 << 3): (P0 << 3) + n2]
    q = np.arange(16384) << 2
    out[PREPARED_L13_BYTES:PREPARED_WORD_OFF].view(np.uint16)[:] = np.where(ln[q] <= 14, step[q], 0)
    seen = ln[q][ln[q] > 0]
    word[:] = [int(seen.max()) if seen.size else 0, int(seen.min()) if seen.size else 255,
               int((canon == 8).all()), 0]
    return out
