"""The host twins of the shared-table batch encoder (include/metalhuffman.h:
mh_frame_histogram, mh_encode_frame_with_header; codec.frame_histogram, shared_header,
encode_frame(header=)): the histogram against the oracle's split and deltas, the frame's own
header against mh_encode_frame (hence the reference encoder's golden hashes), foreign headers
against an independent numpy bit packer and the oracle's shader decode, and every error with
guard bytes around every output. CPU only."""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np
import pytest

from helpers import fibonacci_deltas, golden, image_from_block_deltas

OK, INVALID, TOO_LONG, CAPACITY, TABLE = 0, -1, -3, -4, -5
NO_DELTA = 1
FORMATS = [(0, False), (NO_DELTA, False), (0, True)]   # delta, no-delta, init-byte
_u8p = ctypes.POINTER(ctypes.c_uint8)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)


def _symbols(O, img, flags, init_zero):
    """(symbols in block order, init bytes or None) as mh_encode_frame would encode them, from
    the oracle's split and (per block) deltas."""
    blocks = O.split_blocks(img).reshape(-1, 64)
    init = None
    if not flags & NO_DELTA:
        blocks = np.stack([O.delta_encode(b) for b in blocks])
        if init_zero:
            init = blocks[:, 0].copy()
            blocks[:, 0] = 0
    elif init_zero:
        init = np.zeros(blocks.shape[0], np.uint8)
    return blocks.reshape(-1), init


def _pack(O, header, sym):
    """An independent bit packer on oracle.canonical_codes: MSB first, the last byte
    zero-filled, MH_CODES_PAD zero bytes, one bit offset per 64 symbols."""
    lens = np.asarray(header)[sym].astype(np.int64)
    assert (lens > 0).all()
    codes16 = O.canonical_codes(np.asarray(header, np.uint8))[sym].astype(np.uint32)
    k = np.arange(16, dtype=np.uint32)
    bits = ((codes16[:, None] >> (15 - k)[None, :]) & 1).astype(np.uint8)
    stream = bits[k[None, :] < lens[:, None]]
    start = np.concatenate([[0], np.cumsum(lens)])
    codes = np.concatenate([np.packbits(stream), np.zeros(4, np.uint8)])
    return codes, start[:-1:64].astype(np.uint32)


def _images(bigbridge):
    from metalhuffman_amd import frames as F
    return [np.ascontiguousarray(bigbridge[:256, 500:756]), F.uniform_random(256, 256, 5),
            image_from_block_deltas(fibonacci_deltas(15, 256 * 256, seed=4), 256, 256)]


@pytest.mark.parametrize("hw", [(1, 1), (9, 17), (72, 24)])
@pytest.mark.parametrize("flags,init_zero", FORMATS)
def test_frame_histogram_matches_oracle(mh, oracle, bigbridge, hw, flags, init_zero):
    from metalhuffman_amd import codec
    h, w = hw
    img = np.ascontiguousarray(bigbridge[100:100 + h, 300:300 + w])
    sym, _ = _symbols(oracle, img, flags, init_zero)
    want = np.bincount(sym, minlength=256).astype(np.uint64)
    got = codec.frame_histogram(img, flags, init_zero)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    # a second call adds to the first
    freq = got.copy()
    assert mh.lib().mh_frame_histogram(img.ctypes.data_as(_u8p), w, h, flags, int(init_zero),
                                       freq.ctypes.data_as(_u64p)) == OK
    assert np.array_equal(freq, 2 * want)
    assert mh.lib().mh_frame_histogram(None, w, h, flags, 0, freq.ctypes.data_as(_u64p)) == INVALID
    assert mh.lib().mh_frame_histogram(img.ctypes.data_as(_u8p), w, h, flags, 0, None) == INVALID


def test_shared_header_is_the_tree_of_the_summed_histogram(mh, oracle, bigbridge):
    from metalhuffman_amd import codec
    imgs = _images(bigbridge)
    sym = np.concatenate([_symbols(oracle, im, 0, False)[0] for im in imgs])
    rc, canon = oracle.code_lengths(sym)
    assert rc == 0
    assert np.array_equal(codec.shared_header(imgs), canon)
    assert np.array_equal(codec.shared_header(imgs, limit_lengths=True), canon)   # the tree fits: unchanged


@pytest.mark.parametrize("flags,init_zero", FORMATS)
def test_own_header_equals_encode_frame(mh, bigbridge, flags, init_zero):
    """BigBridge under its own header: mh_encode_frame's bytes, hence the reference's hashes.
    (Its raw pixels' tree is deeper than 16: limit_lengths, which changes no other format.)"""
    ref = mh.encode_frame(bigbridge, flags=flags, init_zero_delta=init_zero, limit_lengths=True)
    got = mh.encode_frame(bigbridge, flags=flags, init_zero_delta=init_zero, header=ref.canon)
    assert np.array_equal(got.canon, ref.canon)
    assert got.codes.size == ref.codes.size and np.array_equal(got.codes, ref.codes)
    assert np.array_equal(got.block_offsets, ref.block_offsets)
    if init_zero:
        assert np.array_equal(got.block_init, ref.block_init)
    else:
        assert got.block_init is None
    if flags == 0 and not init_zero:
        rec = golden()["workloads"]["bigbridge"]
        sha = lambda b: hashlib.sha256(np.ascontiguousarray(b).tobytes()).hexdigest()
        assert sha(got.canon) == rec["canon_sha256"]
        assert sha(got.codes) == rec["huffbuff_sha256"]
        assert sha(got.block_offsets.astype("<u4")) == rec["offsets_sha256"]


def _incomplete_header(sym):
    """Kraft sum < 1, every symbol of `sym` covered: the used symbols at 9 bits (<= 256 / 512)."""
    hdr = np.zeros(256, np.uint8)
    hdr[np.unique(sym)] = 9
    return hdr


@pytest.mark.parametrize("which", ["shared", "flat8", "incomplete"])
@pytest.mark.parametrize("flags,init_zero", FORMATS)
def test_foreign_headers(mh, oracle, bigbridge, which, flags, init_zero):
    from metalhuffman_amd import codec
    from helpers import kraft_sum
    imgs = _images(bigbridge)
    for img in imgs:
        sym, init = _symbols(oracle, img, flags, init_zero)
        header = {"shared": lambda: codec.shared_header(imgs, flags, init_zero),
                  "flat8": lambda: np.full(256, 8, np.uint8),
                  "incomplete": lambda: _incomplete_header(sym)}[which]()
        if which == "incomplete":
            assert kraft_sum(header) < 65536
        ef = mh.encode_frame(img, flags=flags, init_zero_delta=init_zero, header=header)
        codes, offs = _pack(oracle, header, sym)
        assert np.array_equal(ef.canon, header)
        assert ef.codes.size == codes.size and np.array_equal(ef.codes, codes)
        assert np.array_equal(ef.block_offsets, offs)
        if init_zero:
            assert np.array_equal(ef.block_init, init)
        t1, t2 = oracle.split_tables(header)
        dec = oracle.decode_frame_shader(ef.block_offsets, ef.codes, t1, t2, img.shape[1], img.shape[0],
                                         ef.block_init, delta=not flags & NO_DELTA)
        assert np.array_equal(dec, img)
        assert oracle.check_frame(ef.block_offsets, ef.codes, t1, t2).tolist() == [0, 0, 0, 0xFFFFFFFF]


GUARD = 64


def _guarded_call(mh, img, header, cap_delta=None, null=None, with_init=True):
    """mh_encode_frame_with_header into guard-filled outputs -> (status, every output untouched)."""
    h, w = img.shape
    nb = -(-w // 8) * -(-h // 8)
    # cap_delta: the capacity relative to mh_encode_frame's codes_len for the plain format (None: ample room)
    assert cap_delta is None or not with_init
    cap = 2 * nb * 64 + 8 if cap_delta is None else mh.encode_frame(img).codes.size + cap_delta
    codes = np.full(2 * nb * 64 + 8 + 2 * GUARD, 0xC3, np.uint8)
    offs = np.full(nb + 2 * GUARD, 0xC3C3C3C3, np.uint32)
    init = np.full(nb + 2 * GUARD, 0xC3, np.uint8)
    ln = ctypes.c_uint64(0xC3C3C3C3C3C3C3C3)
    hdr = np.ascontiguousarray(header, np.uint8)
    args = dict(gray=img.ctypes.data_as(_u8p), header=hdr.ctypes.data_as(_u8p),
                codes=codes[GUARD:].ctypes.data_as(_u8p), ln=ctypes.byref(ln),
                offs=offs[GUARD:].ctypes.data_as(_u32p), init=init[GUARD:].ctypes.data_as(_u8p))
    if null:
        args[null] = None
    if not with_init:
        args["init"] = None
    st = mh.lib().mh_encode_frame_with_header(args["gray"], w, h, 0, args["header"], args["codes"], cap, args["ln"],
                                              args["offs"], args["init"])
    clean = ((codes == 0xC3).all() and (offs == 0xC3C3C3C3).all() and (init == 0xC3).all()
             and ln.value == 0xC3C3C3C3C3C3C3C3)
    return st, bool(clean)


def test_errors_write_nothing(mh, bigbridge):
    from metalhuffman_amd import codec
    img = np.ascontiguousarray(bigbridge[40:40 + 72, 8:8 + 24])
    own = codec.shared_header([img])
    present = np.flatnonzero(codec.frame_histogram(img))
    # the frame's own header, with room: the guards stay, the outputs do not (the probe works)
    st, clean = _guarded_call(mh, img, own, cap_delta=None)
    assert st == OK and not clean
    # exactly enough room is accepted (codes_len == codes_cap), one byte less is not
    assert _guarded_call(mh, img, own, cap_delta=0, with_init=False)[0] == OK
    assert _guarded_call(mh, img, own, cap_delta=-1, with_init=False) == (CAPACITY, True)
    missing = own.copy()
    missing[present[-1]] = 0                                  # one present symbol without a code
    assert _guarded_call(mh, img, missing, cap_delta=None) == (TABLE, True)
    long17 = own.copy()
    long17[present[0]] = 17
    assert _guarded_call(mh, img, long17, cap_delta=None) == (TOO_LONG, True)
    over = own.copy()
    over[np.flatnonzero(own == 0)[0]] = 16                    # a complete code plus one: Kraft > 1
    assert _guarded_call(mh, img, over, cap_delta=None) == (TABLE, True)
    both = over.copy()
    both[present[0]] = 200                                    # too long wins over the Kraft sum
    assert _guarded_call(mh, img, both, cap_delta=None) == (TOO_LONG, True)
    for null in ("gray", "header", "codes", "ln", "offs"):
        assert _guarded_call(mh, img, own, cap_delta=None, null=null) == (INVALID, True), null
    st, clean = _guarded_call(mh, img, own, cap_delta=None, null="init")   # block_init is optional
    assert st == OK


def test_python_header_errors(mh, bigbridge):
    img = np.ascontiguousarray(bigbridge[:64, :64])
    with pytest.raises(mh.MHError) as e:
        mh.encode_frame(img, header=np.zeros(256, np.uint8))
    assert e.value.status == TABLE
    with pytest.raises(ValueError):
        mh.encode_frame(img, header=np.zeros(255, np.uint8))
