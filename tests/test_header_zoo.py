"""Host builders and CPU decoders over canonical headers that no Huffman construction emits.

Everything the decoders do is a function of the frame's 256 code lengths, and the contract
(include/metalhuffman.h) accepts any header with lengths <= 16 and a Kraft sum <= 1. The
product's encoders only produce Huffman-optimal complete codes, so these tests bring their own
producer (helpers.encode_with_header, pinned here against mh.encode_frame byte for byte) and
their own headers (helpers.header_zoo: random complete codes from leaf splitting, incomplete
ones, hand-written extremes, rejected ones). The zoo's class conditions are asserted here so
that an edit of the generator cannot empty a class that the GPU tests
(test_gpu_header_zoo.py) rely on.

The host table builder has no Kraft check by design (it mirrors the reference), so no host
status is asserted for the over-subscribed headers."""
from __future__ import annotations

import numpy as np
import pytest

from helpers import (HAND_HEADERS, ZOO_RANDOM, encode_with_header, fibonacci_deltas, frame_under_header,
                     header_zoo, image_from_block_deltas, kraft_sum, long_prefixes, zoo_accepted)


# ---- 1. the packer -----------------------------------------------------------------------------

def _huffman_frames(mh, bigbridge):
    """(image, kwargs of mh.encode_frame): natural and synthetic histograms, three sizes."""
    from metalhuffman_amd import frames as F
    return [(np.ascontiguousarray(bigbridge[:56, 300:396]), {}),
            (np.ascontiguousarray(bigbridge[100:356, 500:756]), {}),
            (np.ascontiguousarray(bigbridge[40:64, 700:740]), {}),
            (image_from_block_deltas(fibonacci_deltas(17, 256 * 256, seed=3), 256, 256), {}),
            (F.uniform_random(56, 96, 9), {}),
            (np.ascontiguousarray(bigbridge[100:356, 500:756]), {"init_zero_delta": True}),
            (np.ascontiguousarray(bigbridge[:56, 300:396]), {"init_zero_delta": True}),
            (np.ascontiguousarray(bigbridge[100:356, 500:756]), {"flags": 1}),
            (np.ascontiguousarray(bigbridge[40:64, 700:740]), {"flags": 1})]


def test_packer_reproduces_encode_frame(mh, oracle, bigbridge):
    """encode_with_header, given the header and the symbols of a Huffman frame, reproduces
    mh.encode_frame's code bytes (payload, zero-filled last byte, pad), block offsets and init
    bytes exactly: 9 frames at 96x56, 256x256 and 40x24, delta, init-byte and no-delta formats."""
    from metalhuffman_amd import codec as C
    for k, (img, kw) in enumerate(_huffman_frames(mh, bigbridge)):
        ef = mh.encode_frame(img, **kw)
        h, w = img.shape
        no_delta = bool(kw.get("flags", 0) & mh.MH_FLAG_NO_DELTA)
        blocks = C.split_blocks(img)
        d = blocks
        if not no_delta:  # per block: the first pixel, then the differences
            b = blocks.reshape(-1, 64).astype(np.int16)
            d = np.concatenate([b[:, :1], b[:, 1:] - b[:, :-1]], axis=1).astype(np.uint8).reshape(-1)
        got = encode_with_header(ef.canon, d, w, h, no_delta=no_delta,
                                 init_zero_delta=bool(kw.get("init_zero_delta")))
        assert np.array_equal(got.codes, ef.codes), k
        assert got.block_offsets.dtype == np.uint32 and np.array_equal(got.block_offsets, ef.block_offsets), k
        assert (got.block_init is None) == (ef.block_init is None), k
        if ef.block_init is not None:
            assert np.array_equal(got.block_init, ef.block_init), k
        assert (got.width, got.height, got.flags) == (ef.width, ef.height, ef.flags), k


def test_packer_refuses_a_symbol_without_a_code():
    canon = np.zeros(256, np.uint8)
    canon[[3, 4]] = 1
    with pytest.raises(AssertionError):
        encode_with_header(canon, np.full(64, 5, np.uint8), 8, 8)
    with pytest.raises(AssertionError):  # init bytes put a zero symbol in front of every block
        encode_with_header(canon, np.full(64, 3, np.uint8), 8, 8, init_zero_delta=True)


# ---- 2. the zoo's classes ------------------------------------------------------------------------

def _class_counts(heads):
    longest = [z.longest for z in heads]
    return {"<=12": sum(l <= 12 for l in longest), **{l: sum(x == l for x in longest) for l in (13, 14, 15, 16)}}


def test_zoo_is_deterministic_and_its_classes_are_filled():
    """The generator's conditions. Random complete codes: 400 headers, every Kraft sum exactly
    65536, at least 20 for each longest length 13, 14, 15, 16 and at least 20 with a longest
    length <= 12, at least 3 with 64 or more 13-bit prefixes of long codes. Incomplete variants
    (every 8th random header, a quarter of its symbols dropped: 50 headers): every Kraft sum
    below 65536, the lengths that stay unchanged; 50 headers cannot hold five classes of 20, so
    the classes -- by the longest length that REMAINS -- are asked of the random and incomplete
    headers together (at least 20 each) and of the incomplete ones alone at a count of the same
    ratio, 20 / 8 rounded up = 3 each. Hand-written and rejected headers as listed."""
    import helpers
    zoo = header_zoo()
    helpers._ZOO.pop(helpers.ZOO_SEED)  # generate it a second time
    fresh = header_zoo()
    assert [z.name for z in fresh] == [z.name for z in zoo]
    assert all(np.array_equal(a.canon, b.canon) and a.status == b.status for a, b in zip(zoo, fresh))
    assert len({z.name for z in zoo}) == len(zoo)

    rnd = [z for z in zoo if z.kind == "random"]
    assert len(rnd) == ZOO_RANDOM == 400
    assert all(kraft_sum(z.canon) == 65536 and z.status == 0 for z in rnd)
    assert all(2 <= int((z.canon > 0).sum()) <= 256 for z in rnd)
    counts = _class_counts(rnd)
    assert all(v >= 20 for v in counts.values()), counts
    assert sum(long_prefixes(z.canon) >= 64 for z in rnd) >= 3
    # a length's symbols lie in all four 64-symbol waves of the builders' ballots
    assert sum(len({int(s) >> 6 for s in np.flatnonzero(z.canon == z.longest)}) == 4 for z in rnd) >= 20

    inc = [z for z in zoo if z.kind == "incomplete"]
    assert len(inc) == 50
    for z in inc:
        base = rnd[int(z.name[3:])]
        kept = z.canon > 0
        dropped = int((base.canon > 0).sum()) - int(kept.sum())
        assert z.status == 0 and kraft_sum(z.canon) < 65536 and np.array_equal(z.canon[kept], base.canon[kept])
        assert dropped == max(1, int((base.canon > 0).sum()) // 4)
    both = _class_counts(rnd + inc)
    assert all(v >= 20 for v in both.values()), both
    alone = _class_counts(inc)
    assert all(v >= 3 for v in alone.values()), alone

    hand = [z for z in zoo if z.kind == "hand"]
    assert len(hand) == 2 * len(HAND_HEADERS) == 32
    for z in hand:
        spec = HAND_HEADERS[z.name[:-2]]
        assert {int(l): int((z.canon == l).sum()) for l in np.unique(z.canon[z.canon > 0])} == spec, z.name
        assert z.status == 0 and kraft_sum(z.canon) <= 65536, z.name
    assert long_prefixes(next(z.canon for z in hand if z.name == "14x256/a")) == 128

    rej = {z.name: z for z in zoo if z.kind == "rejected"}
    assert {n: z.status for n, z in rej.items()} == {
        "complete+16": -5, "three_1bit": -5, "len17": -3, "len32": -3, "len128": -3, "len255": -3,
        "len200_oversubscribed": -3}
    assert kraft_sum(rej["complete+16"].canon) == 65537 and rej["complete+16"].longest == 16
    assert kraft_sum(rej["three_1bit"].canon) == 3 * 32768
    for long in (17, 32, 128, 255):
        c = rej[f"len{long}"].canon
        assert int((c > 16).sum()) == 1 and c.max() == long and kraft_sum(c) == 65536
    c = rej["len200_oversubscribed"].canon
    assert c.max() == 200 and kraft_sum(c) > 65536
    assert len(zoo_accepted()) == 400 + 50 + 32


# ---- 3. host builders against the oracle ---------------------------------------------------------

def test_host_tables_equal_the_oracle_for_every_accepted_header(mh, oracle):
    """mh_build_tables == oracle.split_tables and mh_build_single_table == oracle.single_table,
    byte for byte, for all 482 accepted headers."""
    for z in zoo_accepted():
        t1, t2 = mh.Huffman.generateSplitLookupTables(z.canon)
        o1, o2 = oracle.split_tables(z.canon)
        assert np.array_equal(t1, o1) and np.array_equal(t2, o2), z.name
        assert np.array_equal(mh.Huffman.generateLookupTable(z.canon), oracle.single_table(z.canon)), z.name


# ---- 4. CPU decoders -----------------------------------------------------------------------------

def _cpu_cases():
    zoo = zoo_accepted()
    rnd = [z for z in zoo if z.kind == "random"]
    return [z for z in zoo if z.kind == "hand"] + rnd[::10]


@pytest.mark.parametrize("variant", ["delta", "init_zero_delta", "no_delta"])
def test_cpu_decoders_return_the_image(mh, oracle, variant):
    """Every hand-written header and every 10th random one: a 96x56 frame of uniformly drawn
    used symbols, decoded by mh_decode_frame_cpu on 1 and 3 threads, by the stream decoders
    mh_decode_huffman_bits (single table) and mh_decode_huffman_bits_from_tables (the frame's
    blocks are contiguous: one stream of 84 x 64 symbols), and by the oracle's
    decode_frame_shader. All equal the image / the symbols. The init-byte format needs a code
    for symbol 0; headers without one are left to the other two formats."""
    from metalhuffman_amd import codec as C
    w, h = 96, 56
    done = 0
    for k, z in enumerate(_cpu_cases()):
        kw = {"no_delta": variant == "no_delta", "init_zero_delta": variant == "init_zero_delta"}
        if kw["init_zero_delta"] and z.canon[0] == 0:
            continue
        ef, img = frame_under_header(z.canon, w, h, seed=100 + k, **kw)
        for threads in (1, 3):
            assert np.array_equal(C.decode_frame_cpu(ef, threads=threads), img), (z.name, threads)
        t1, t2 = oracle.split_tables(z.canon)
        assert np.array_equal(oracle.decode_frame_shader(ef.block_offsets, ef.codes, t1, t2, w, h,
                                                         block_init=ef.block_init, delta=not kw["no_delta"]),
                              img), z.name
        n = ef.n_blocks * 64
        sym, offs = mh.Huffman.decodeHuffmanBits(mh.Huffman.generateLookupTable(z.canon), n, ef.codes,
                                                 bitOffsets=True)
        assert np.array_equal(offs[::64], ef.block_offsets), z.name
        h1, h2 = ef.tables()
        sym2, offs2 = mh.Huffman.decodeHuffmanBitsFromTables(h1, h2, 8, 8, n, ef.codes, bitOffsets=True)
        assert np.array_equal(sym, sym2) and np.array_equal(offs, offs2), z.name
        # the symbols, back through the producer's own steps, are the image
        blocks = sym.reshape(-1, 64).copy()
        if ef.block_init is not None:
            blocks[:, 0] = ef.block_init
        if not kw["no_delta"]:
            blocks = (np.cumsum(blocks.astype(np.uint16), axis=1) & 0xFF).astype(np.uint8)
        assert np.array_equal(C.merge_blocks(blocks.reshape(-1), w, h), img), z.name
        done += 1
    # every case; with init bytes at least the 16 hand-written "/a" dealings, which use symbol 0
    assert done >= (16 if variant == "init_zero_delta" else 32 + ZOO_RANDOM // 10), done
