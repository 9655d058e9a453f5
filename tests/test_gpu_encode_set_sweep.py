"""A seeded sweep over mh_encode_set_device_async (set_encode_helpers.sweep_case; the cases' coverage
is asserted on the CPU in test_encode_set_sweep_cases.py): sets of 1..12 frames on grids of 1..300 x
1..24 blocks with an edge size in every set, as planar allocations, planes (all or a suffix) of
interleaved images, windows of shared pictures or samples 5..255 bytes apart, now and then with one
record that breaks the dword mode; both formats and the init bytes, MH_ENCODE_LIMIT_LENGTHS, a zeroed
or a garbage workspace, d_codes_len or d_status as NULL, roomy, exact and too small slots per frame,
and now and then a frame whose tree is deeper than 16.

Every case runs once through the raw ABI into guard-filled outputs, is checked against the host codec
byte for byte and guard for guard (set_encode_helpers.check), and is decoded straight back on the
device from the plan's own geometry records and the encoder's status words (decode_back). The default
range is fixed -- MH_ENCODE_SET_SWEEP_CASES cases from MH_ENCODE_SET_SWEEP_FIRST on, 48 from 0 -- so it
is the same on every machine; a failure names the case index i, which replays alone with
MH_ENCODE_SET_SWEEP_FIRST=i MH_ENCODE_SET_SWEEP_CASES=1."""
from __future__ import annotations

import pytest

import set_encode_helpers as SH

pytestmark = pytest.mark.gpu

FIRST, COUNT = SH.sweep_range()
CHUNK = 8


@pytest.mark.parametrize("start", range(FIRST, FIRST + COUNT, CHUNK))
def test_encode_set_sweep(mh, device, bigbridge, start):
    assert COUNT >= 1
    for i in range(start, min(start + CHUNK, FIRST + COUNT)):
        SH.run_sweep_case(mh, device, SH.sweep_case(i), bigbridge)
