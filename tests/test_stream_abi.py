"""The flag rule of the stream create functions (include/metalhuffman.h: mh_stream_create,
mh_stream_create_headers): MH_FLAG_NO_DELTA is the only flag a stream takes. Any other bit --
MH_FLAG_ANY_ORDER above all, which would send a slot's decode out without the barrier behind the
slot's own H2D copy -- is MH_ERR_INVALID_ARG, with the other argument checks and before any HIP
call: fake pointers, no device. CPU only."""
from __future__ import annotations

import ctypes

import pytest

INVALID, DIMS = -1, -2
T1, T2, LUT, INIT = 0x30000, 0x40000, 0x60000, 0x70000     # never dereferenced
NO_DELTA = 0x1
# MH_FLAG_LANE_PAIRS, MH_FLAG_ANY_ORDER, MH_ENCODE_WORKSPACE_ZEROED, MH_ENCODE_LIMIT_LENGTHS
OTHER_FLAGS = (0x2, 0x4, 0x100, 0x200)


def _proto(flags, dims=(16, 16, 2, 2), init=False):
    from metalhuffman_amd import _native as N
    fr = N.mh_frame()
    fr.d_table1, fr.d_table2, fr.table2_entries, fr.d_lut = T1, T2, 256, LUT
    fr.d_block_init = INIT if init else None
    fr.dims = N.mh_dims(*dims)
    fr.n_frames = 1
    fr.flags = flags
    return fr


def _create(mh, mode):
    L = mh.lib()
    return L.mh_stream_create if mode == "table" else L.mh_stream_create_headers


def test_the_flag_values_are_the_headers(mh):
    from metalhuffman_amd import _native as N
    assert (N.MH_FLAG_NO_DELTA, N.MH_FLAG_LANE_PAIRS, N.MH_FLAG_ANY_ORDER, N.MH_ENCODE_WORKSPACE_ZEROED,
            N.MH_ENCODE_LIMIT_LENGTHS) == (NO_DELTA,) + OTHER_FLAGS


@pytest.mark.parametrize("mode", ["table", "headers"])
@pytest.mark.parametrize("flag", OTHER_FLAGS, ids=[hex(f) for f in OTHER_FLAGS])
def test_create_refuses_every_flag_but_no_delta(mh, mode, flag):
    """Alone, beside MH_FLAG_NO_DELTA, with init bytes, with caller rasters: MH_ERR_INVALID_ARG,
    and *out is left as it was (no stream was made)."""
    create = _create(mh, mode)
    outs = (ctypes.c_void_p * 2)(0x50000, 0x58000)
    for flags in (flag, flag | NO_DELTA):
        for init in (False, True):
            for d_outputs in (None, outs):
                h = ctypes.c_void_p(0x1234)
                assert create(ctypes.byref(_proto(flags, init=init)), 4096, 2, d_outputs, ctypes.byref(h)) == INVALID
                assert h.value == 0x1234


@pytest.mark.parametrize("mode", ["table", "headers"])
def test_high_bits_and_all_bits_are_refused(mh, mode):
    create = _create(mh, mode)
    h = ctypes.c_void_p()
    for flags in (0x8, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFE, 0x6):
        assert create(ctypes.byref(_proto(flags)), 4096, 2, None, ctypes.byref(h)) == INVALID


@pytest.mark.parametrize("mode", ["table", "headers"])
def test_the_flag_rule_stands_with_the_argument_checks(mh, mode):
    """A refused flag is reported as an argument error, ahead of the dims rule; with legal flags the
    dims rule still answers (so the flag check did not swallow it)."""
    create = _create(mh, mode)
    h = ctypes.c_void_p()
    bad_dims = (16, 16, 3, 2)
    assert create(ctypes.byref(_proto(0x4, bad_dims)), 4096, 2, None, ctypes.byref(h)) == INVALID
    for flags in (0, NO_DELTA):
        assert create(ctypes.byref(_proto(flags, bad_dims)), 4096, 2, None, ctypes.byref(h)) == DIMS
    assert create(ctypes.byref(_proto(0x4)), 4096, 0, None, ctypes.byref(h)) == INVALID
    assert create(ctypes.byref(_proto(0x4)), 2, 2, None, ctypes.byref(h)) == INVALID
