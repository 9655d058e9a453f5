"""Code-side addressing at the 32-bit edges, host side (the GPU half: test_gpu_code_addressing.py).

1. Streams placed high in a large buffer (helpers.place_stream): block offsets straddling 2^31
   (`mid`) and ending just below 2^32 (`top`, helpers.lead_top) must be valid frames under the
   reference's semantics before a GPU kernel sees them -- the product's CPU frame decoder on 1 and
   3 threads and the oracle's shader decode return the image, the oracle's check is clean.
2. The host encoder at 2^32 code bits: exactly uniform symbols (every code 8 bits) of length 2^29
   are rejected with MH_ERR_CAPACITY, of length 2^29 - 128 encoded -- codes equal to the symbols."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from helpers import (exactly_uniform_image, frame_under_header, header_zoo, lead_mid, lead_top, place_stream,
                     placed_host_frame)

W, H = 96, 56
CLEAN = [0, 0, 0, 0xFFFFFFFF]
MH_ERR_CAPACITY = -4


def _small_frames(mh, bigbridge):
    """(name, EncodedFrame, image): a BigBridge crop, {16: 256}, {1: 1} and uniformly drawn bytes
    under the flat 8-bit header."""
    from metalhuffman_amd import frames as F
    crop = F.crop(bigbridge, H, W)
    yield "bigbridge_crop", mh.encode_frame(crop), crop
    by_name = {z.name: z for z in header_zoo()}
    for k, name in enumerate(("16x256/a", "1x1/a", "8x256/a")):
        ef, img = frame_under_header(by_name[name].canon, W, H, seed=300 + k)
        yield name, ef, img


def test_placements_state_their_conditions(mh, bigbridge):
    """place_stream adds 8 * lead to every offset and keeps the payload; `mid` straddles 2^31
    inside tile 0; `top` puts the last block above 2^32 - 1024 with the last bit below 2^32 and
    a lead off the 16-byte grid (the 1024-bit last block of {16: 256}: see helpers.lead_top)."""
    for name, ef, _ in _small_frames(mh, bigbridge):
        for lead in (lead_mid(ef), lead_top(ef)):
            payload, offs, total = place_stream(ef, lead)
            assert payload is ef.codes and total == lead + ef.codes.size
            assert np.array_equal(offs.astype(np.int64) - 8 * lead, ef.block_offsets.astype(np.int64)), name
        offs = place_stream(ef, lead_mid(ef))[1].astype(np.int64)
        assert offs[0] < 2 ** 31 <= offs[63], name
        lead = lead_top(ef)
        offs = place_stream(ef, lead)[1].astype(np.int64)
        assert lead % 16 and 8 * lead + 8 * ef.payload_bytes <= 2 ** 32, name
        if name == "16x256/a":
            assert offs[-1] == 2 ** 32 - 1032
            assert place_stream(ef, lead_top(ef, aligned=True))[1][-1] == 2 ** 32 - 1024
        else:
            assert 2 ** 32 - 1024 < offs[-1] < 2 ** 32, name


@pytest.mark.parametrize("placement", ["mid", "top", "top_aligned"])
def test_placed_streams_through_the_cpu_decoders(mh, oracle, bigbridge, placement):
    for name, ef, img in _small_frames(mh, bigbridge):
        if placement == "top_aligned" and name != "16x256/a":
            continue
        lead = lead_mid(ef) if placement == "mid" else lead_top(ef, aligned=placement == "top_aligned")
        pf = placed_host_frame(ef, lead)
        assert pf.codes.size == lead + ef.codes.size and not pf.codes[max(0, lead - 4096): lead].any()
        t1, t2 = pf.tables()
        for threads in (1, 3):
            assert np.array_equal(mh.decode_frame_cpu(pf, threads), img), (name, placement, threads)
        got = oracle.decode_frame_shader(pf.block_offsets, pf.codes, t1, t2, W, H, block_init=pf.block_init,
                                         delta=not (pf.flags & 1))
        assert np.array_equal(got, img), (name, placement)
        assert oracle.check_frame(pf.block_offsets, pf.codes, t1, t2).tolist() == CLEAN, (name, placement)
        del pf


def _encode_huffman(mh, sym):
    """mh_encode_huffman with 64-symbol blocks -> (status, canon, codes buffer, codes_len, offsets)."""
    from metalhuffman_amd import _native as N
    L = N.lib()
    cap = int(L.mh_codes_bound(sym.size))
    canon = np.zeros(256, np.uint8)
    codes = np.zeros(cap, np.uint8)      # untouched pages cost nothing
    offs = np.zeros(sym.size // 64, np.uint32)
    ln = ctypes.c_uint64(0)
    u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    rc = L.mh_encode_huffman(sym.ctypes.data_as(u8p), sym.size, 8, canon.ctypes.data_as(u8p),
                             codes.ctypes.data_as(u8p), cap, ctypes.byref(ln), offs.ctypes.data_as(u32p))
    return rc, canon, codes, int(ln.value), offs


def test_host_encoder_rejects_2_pow_32_bits(mh):
    """2^29 exactly uniform symbols: 256 codes of 8 bits, 2^32 code bits -- one more than a u32
    block offset can address -> MH_ERR_CAPACITY."""
    sym = exactly_uniform_image(1 << 15, 1 << 14, seed=21).reshape(-1)
    assert sym.size == 1 << 29
    rc = _encode_huffman(mh, sym)[0]
    assert rc == MH_ERR_CAPACITY, rc


def test_host_encoder_accepts_2_pow_32_minus_1024_bits(mh):
    """2^29 - 128 exactly uniform symbols (counts differ by one: still 256 codes of 8 bits, so
    code c is symbol c): MH_OK, offsets[b] = 512 b, the codes are the symbols, two zero bytes
    behind them."""
    n = (1 << 29) - 128
    sym = exactly_uniform_image(n // 8, 8, seed=22).reshape(-1)
    assert sym.size == n
    rc, canon, codes, ln, offs = _encode_huffman(mh, sym)
    assert rc == 0, rc
    assert (canon == 8).all()
    assert ln == n + 2
    assert np.array_equal(offs, (512 * np.arange(n // 64, dtype=np.uint64)).astype(np.uint32))
    assert int(offs[-1]) == 2 ** 32 - 1024 - 512
    assert np.array_equal(codes[:n], sym)
    assert not codes[n: n + 2].any()
