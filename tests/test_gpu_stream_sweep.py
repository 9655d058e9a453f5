"""A seeded sweep over the two stream front ends (stream_helpers.sweep_case): 32 cases a mode over
widths and heights from 1 to 264 with the 8-pixel and 64-pixel edges, 1..4 slots, 2..9 frames of
different code lengths in the order longest, shortest, rest per slot, the three formats, host buffers
in slot layout or apart, pinned or pageable, the stream's rasters or guarded caller rasters, graph
replays or direct launches, with or without a prepared table, waiting for every frame or back to
back (the values come from fixed lists taken in turn; what the default range covers is asserted on
the CPU in test_stream_sweep_cases.py).

Every case goes through stream_helpers.Driver: each submit's raster is copied out on the slot's
stream and compared with a direct decode, the image and (one frame) the oracle. The default range is
fixed -- MH_STREAM_SWEEP_CASES cases from MH_STREAM_SWEEP_FIRST on, 32 from 0 -- so it is the same on
every machine; a failure names (mode, i), which replays alone with MH_STREAM_SWEEP_FIRST=i
MH_STREAM_SWEEP_CASES=1."""
from __future__ import annotations

import pytest

import stream_helpers as SH

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", SH.MODES)
def test_stream_sweep(mh, oracle, device, mode):
    first, count = SH.sweep_range()
    assert count >= 1
    for i in range(first, first + count):
        SH.run_sweep_case(mh, oracle, device, SH.sweep_case(mode, i))
