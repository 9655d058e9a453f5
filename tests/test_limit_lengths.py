"""Length-limited Huffman codes on the host (mh_code_lengths_limited, mh_encode_frame with
MH_ENCODE_LIMIT_LENGTHS): an optimal code of at most max_bits bits by package-merge where
the reference tree is deeper, the reference tree's own lengths where it fits. The cost
(sum of count x length) of an optimal code is unique, so it is compared with a textbook
package-merge that carries explicit item sets; the lengths themselves are pinned by the
rule in DESIGN.md ("Length-limited codes"), restated in limit_helpers.normative_lengths."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import limit_helpers as LH
from helpers import golden

LIMIT = 0x200


def _code_lengths(mh, freq):
    from metalhuffman_amd import _native as N
    f = np.ascontiguousarray(freq, np.uint64)
    canon = np.zeros(256, np.uint8)
    rc = N.lib().mh_code_lengths(f.ctypes.data_as(N._u64p), canon.ctypes.data_as(N._u8p))
    return rc, canon


def _limited(mh, freq, max_bits):
    from metalhuffman_amd import _native as N
    f = np.ascontiguousarray(freq, np.uint64)
    canon = np.zeros(256, np.uint8)
    rc = N.lib().mh_code_lengths_limited(f.ctypes.data_as(N._u64p), max_bits, canon.ctypes.data_as(N._u8p))
    return rc, canon


@pytest.fixture(scope="module")
def histograms():
    return LH.limit_histograms()


def test_histograms_are_mostly_deeper_than_16(mh, histograms):
    deep = sum(_code_lengths(mh, f)[0] == -3 for _, f in histograms)
    assert len(histograms) == 209 and deep >= 100, deep


@pytest.mark.parametrize("which", ["16", "13", "8", "log2n"])
def test_against_textbook_package_merge(mh, histograms, which):
    """Every length <= max_bits, Kraft sum exactly 65536/65536, the textbook's cost, and
    the normative lengths byte for byte (the reference tree's where those fit)."""
    ran = limited = 0
    for name, f in histograms:
        n = int(np.count_nonzero(f))
        max_bits = max(1, (n - 1).bit_length()) if which == "log2n" else int(which)
        if (1 << max_bits) < n:
            assert _limited(mh, f, max_bits)[0] == -1, name
            continue
        got = mh.code_lengths_limited(f, max_bits)
        assert np.array_equal(got > 0, f > 0), name
        assert int(got.max()) <= max_bits, name
        assert LH.kraft16(got) == 65536, (name, LH.kraft16(got))
        assert LH.cost(f, got) == LH.cost(f, LH.textbook_package_merge(f, max_bits)), name
        _, huff = _code_lengths(mh, f)
        if int(huff.max()) <= max_bits:
            assert np.array_equal(got, huff), name
        else:
            assert np.array_equal(got, LH.normative_lengths(f, max_bits)), name
            limited += 1
        ran += 1
    assert ran >= 100 and limited >= 100, (ran, limited)


def test_where_the_tree_fits_the_cost_is_huffmans(mh, histograms):
    """The rule alone (never the shortcut) costs what the Huffman tree costs where that
    fits 16 bits: both are optimal."""
    fits = 0
    for name, f in histograms:
        rc, huff = _code_lengths(mh, f)
        if rc == 0 and np.count_nonzero(f) >= 2:
            assert LH.cost(f, LH.normative_lengths(f, 16)) == LH.cost(f, huff), name
            assert np.array_equal(mh.code_lengths_limited(f, 16), huff), name
            fits += 1
    assert fits >= 10


def test_tight_limits_and_argument_checks(mh):
    f = np.arange(1, 257, dtype=np.uint64) ** 3
    assert (mh.code_lengths_limited(f, 8) == 8).all()           # 256 symbols in 8 bits
    assert (mh.code_lengths_limited(LH.chain_histogram(), 8) == 8).all()
    two = np.zeros(256, np.uint64)
    two[[3, 200]] = [1, 10 ** 12]
    assert mh.code_lengths_limited(two, 1)[[3, 200]].tolist() == [1, 1]
    one = np.zeros(256, np.uint64)
    one[77] = 5
    for bits in (1, 16):
        got = mh.code_lengths_limited(one, bits)
        assert got[77] == 1 and got.sum() == 1                  # one symbol: length 1, as today
    assert _limited(mh, np.zeros(256, np.uint64), 16)[0] == -8  # MH_ERR_EMPTY
    for bits in (0, 17, 7):                                     # 2^7 < 256 symbols
        assert _limited(mh, f, bits)[0] == -1
    big = np.zeros(256, np.uint64)
    big[[0, 1]] = [2 ** 58, 2 ** 58]                            # total 2^59
    assert _limited(mh, big, 16)[0] == -1
    big[1] -= 1
    assert _limited(mh, big, 16)[0] == 0
    big[0] = 2 ** 63
    assert _limited(mh, big, 16)[0] == -1
    with pytest.raises(mh.MHError):
        mh.code_lengths_limited(np.zeros(256, np.uint64))
    from metalhuffman_amd import _native as N
    assert N.lib().mh_code_lengths_limited(None, 16, None) == -1


def test_equal_counts_lower_symbol_not_shorter(mh, histograms):
    for name, f in histograms:
        got = mh.code_lengths_limited(f, 16).astype(int)
        present = np.flatnonzero(f)
        order = sorted(present, key=lambda s: (int(f[s]), s))
        assert all(got[a] >= got[b] for a, b in zip(order, order[1:])), name


def test_no_change_where_the_tree_fits(mh, bigbridge):
    """The golden workloads' frames (BigBridge, its block shuffle), a crop with partial
    blocks and a uniform frame: byte-identical with and without the flag, and
    mh_code_lengths_limited(freq, 16) is mh_code_lengths. (BigBridge's raw pixels, the
    no-delta format, make a tree deeper than 16: that format is checked on the uniform frame.)"""
    from metalhuffman_amd import frames as F
    g = golden()["workloads"]
    assert "bigbridge" in g and "bigbridge_shuffle_seed7" in g
    delta = ((0, False), (0, True))
    cases = [(bigbridge, delta), (F.block_shuffle(bigbridge, 7), delta),
             (np.ascontiguousarray(bigbridge[:520, :1000]), delta),
             (F.uniform_random(256, 256, 5), delta + ((1, False),))]
    for img, formats in cases:
        for flags, init in formats:
            a = mh.encode_frame(img, flags=flags, init_zero_delta=init)
            b = mh.encode_frame(img, flags=flags, init_zero_delta=init, limit_lengths=True)
            assert a.flags == b.flags == flags
            assert np.array_equal(a.canon, b.canon) and np.array_equal(a.codes, b.codes)
            assert np.array_equal(a.block_offsets, b.block_offsets)
            if init:
                assert np.array_equal(a.block_init, b.block_init)
            if img.shape[0] % 8 == 0 and img.shape[1] % 8 == 0:
                f = LH.frame_histogram(img, no_delta=bool(flags), init_zero_delta=init)
                assert _code_lengths(mh, f)[0] == 0
                assert np.array_equal(mh.code_lengths_limited(f, 16), a.canon)


def test_without_the_flag_a_depth_17_frame_is_still_rejected(mh):
    img = LH.image_from_histogram(LH.fib_histogram(18, 128 * 64, seed=1), 128, 64, 1)
    with pytest.raises(mh.MHError) as e:
        mh.encode_frame(img)
    assert e.value.status == -3
    rc, canon = _code_lengths(mh, LH.frame_histogram(img))
    assert rc == -3 and canon.max() == 17


FRAMES = {  # name -> (width, height, histogram)
    "fib18": (128, 64, lambda: LH.fib_histogram(18, 128 * 64, seed=18)),
    "fib19": (128, 64, lambda: LH.fib_histogram(19, 128 * 64, seed=19)),
    "chain256": (1024, 1024, LH.chain_histogram),
}


@pytest.mark.parametrize("fmt", list(LH.FORMATS))
@pytest.mark.parametrize("name", list(FRAMES))
def test_round_trip(mh, oracle, name, fmt):
    """encode_frame(limit_lengths=True) -> mh_build_tables -> decode_frame_cpu, and the
    oracle's shader decode, give the image back; the header is the limited code of the
    frame's own histogram."""
    w, h, hist = FRAMES[name]
    no_delta, init = LH.FORMATS[fmt]
    freq = hist()
    img = LH.image_from_histogram(freq, w, h, 3, no_delta=no_delta)
    coded = LH.frame_histogram(img, no_delta=no_delta, init_zero_delta=init)
    rc, huff = _code_lengths(mh, coded)
    assert rc == -3 and (huff.max() == 17 or name == "fib19")  # 18 Fibonacci symbols: the smallest that trips
    if name == "chain256":
        assert np.count_nonzero(coded) == 256
    ef = mh.encode_frame(img, flags=1 if no_delta else 0, init_zero_delta=init, limit_lengths=True)
    assert ef.flags == (1 if no_delta else 0)            # the keyword does not reach the decoders
    assert np.array_equal(ef.canon, LH.normative_lengths(coded, 16))
    assert np.array_equal(ef.canon, mh.code_lengths_limited(coded, 16))
    assert ef.canon.max() == 16 and LH.kraft16(ef.canon) == 65536
    assert np.array_equal(mh.decode_frame_cpu(ef), img)
    t1, t2 = ef.tables()
    got = oracle.decode_frame_shader(ef.block_offsets, ef.codes, t1, t2, w, h, block_init=ef.block_init,
                                     delta=not no_delta)
    assert np.array_equal(got, img)


def _device_encoders(N):
    """(name, call(width, height, flags, codes, workspace)) for the three device encoders with
    otherwise valid, never dereferenced pointers: only the argument checks run."""
    L = N.lib()
    p = 0x10000  # 64 KiB: aligned for every rule

    def one_async(w, h, flags, codes=p, ws=p):
        return L.mh_encode_frame_device_async(p, w, h, flags, p, codes, 1 << 20, p, p, None, p, ws, 1 << 30, None)

    def one_sync(w, h, flags, codes=p, ws=p):
        canon = (ctypes.c_uint8 * 256)()
        n = ctypes.c_uint64(0)
        return L.mh_encode_frame_device(p, w, h, flags, canon, codes, 1 << 20, ctypes.byref(n), p, None, ws,
                                        1 << 30, None)

    def batch(w, h, flags, codes=p, ws=p):
        return L.mh_encode_frames_device_async(p, w * h, 2, w, h, flags, p, codes, 1 << 20, p, p, p, None, p, ws,
                                               1 << 30, None)

    return [("async", one_async), ("sync", one_sync), ("batch", batch)]


def test_device_encoders_argument_checks(mh):
    """No GPU needed: with flag 0x200 a bad dimension or alignment is reported as such
    (the flag passed the mask), while 0x40 and the decoder's lane-pair flag 2 are refused."""
    from metalhuffman_amd import _native as N
    for name, call in _device_encoders(N):
        for flags in (LIMIT, LIMIT | 1, LIMIT | 0x100):
            assert call(0, 64, flags) == -2, name                       # MH_ERR_DIMS
            assert call(64, 70000, flags) == -2, name
            assert call(64, 64, flags, ws=0x10000 + 16) == -6, name     # MH_ERR_ALIGN
            assert call(64, 64, flags, codes=0x10000 + 2) == -6, name
        for flags in (0x40, 2, LIMIT | 0x40, LIMIT | 2):
            assert call(64, 64, flags) == -1, name                      # MH_ERR_INVALID_ARG
            assert call(0, 64, flags) == -1, name


def test_decoders_refuse_the_flag(mh):
    from metalhuffman_amd import _native as N
    fr = N.mh_frame()
    fr.d_block_offsets = fr.d_codes = fr.d_table1 = fr.d_table2 = fr.d_lut = 0x10000
    fr.codes_bytes, fr.table2_entries, fr.n_frames = 1024, 256, 1
    fr.dims = N.mh_dims(64, 64, 8, 8)
    fr.flags = LIMIT
    assert N.lib().mh_decode(ctypes.byref(fr), 0x10000, 64, 64 * 64, None) == -1


def test_python_keyword_does_not_leak_into_frame_flags(mh):
    import inspect

    from metalhuffman_amd import encoder as E
    img = LH.image_from_histogram(LH.fib_histogram(20, 128 * 64, seed=2), 128, 64, 2, no_delta=True)
    ef = mh.encode_frame(img, flags=mh.MH_FLAG_NO_DELTA, limit_lengths=True)
    assert ef.flags == mh.MH_FLAG_NO_DELTA and not ef.flags & LIMIT
    assert ef.band(0, 4).flags == mh.MH_FLAG_NO_DELTA
    assert mh.MH_ENCODE_LIMIT_LENGTHS == LIMIT
    for fn in (mh.encode_frame, E.Encoder.encode, E.Encoder.encode_async, E.BatchEncoder.encode_async,
               E.encode_frame_device):
        assert inspect.signature(fn).parameters["limit_lengths"].default is False, fn
