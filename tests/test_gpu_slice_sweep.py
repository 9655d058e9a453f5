"""A seeded sweep over the seven decode entries that go through slice_decode: frames, headers, region,
region_scaled, windows, windows_scaled and crops, over grids of 1..200 x 1..24 blocks with every
declared size, every step flavour, shared tables and table sets, 1..5 rectangles pinned to the
frame's edges or anywhere, scales 1/2..1/8 and both raster geometries (slice_helpers.sweep_case; the
cases' coverage is asserted on the CPU in test_slice_sweep_cases.py).

Every case is one launch through the C ABI into a pattern-guarded buffer of which every byte is
checked (slice_helpers.run_contained); expected pixels are numpy slices of the oracle's full-frame
decode. The default range is fixed -- MH_SLICE_SWEEP_CASES cases from MH_SLICE_SWEEP_FIRST on, 40
from 0 -- not time-boxed, so it is the same on every machine; a failure names (entry, i), which
replays alone with MH_SLICE_SWEEP_FIRST=i MH_SLICE_SWEEP_CASES=1."""
from __future__ import annotations

import pytest

import slice_helpers as SH

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("entry", SH.ENTRIES)
def test_slice_sweep(mh, oracle, device, entry):
    first, count = SH.sweep_range()
    assert count >= 1
    for i in range(first, first + count):
        case = SH.sweep_case(entry, i)
        up, tabs = SH.upload(device, SH.sweep_frames(mh, oracle, case), case.tables, entry)
        try:
            SH.run_contained(entry, device, case.geom, up, tabs, case.what, case.k)
        except Exception as e:   # a case the host layer rejects fails the sweep like a wrong pixel
            raise AssertionError(f"{case.describe()}\n{type(e).__name__}: {e}") from e
