"""A defective frame harms only its own undecodable blocks (include/metalhuffman.h, mh_frame; DESIGN.md
section 1), through every decode entry: mh_decode with in-kernel tables, at a batch size that takes the
batch kernel, at one that takes the small kernel and through the single-frame entry, and frames,
headers, region, region_scaled, windows, windows_scaled, crops, crops_norm and crops_norm_planes.

Every case (defect_helpers.defect_case; the cases' coverage and caps are asserted on the CPU in
test_defect_cases.py) is a batch of 2..5 frames on a grid of 1..80 x 1..6 blocks, at least one of them
clean, the others with flipped, overwritten or replaced code bits, a moved or doubled offset or a slot
cut short. It is ONE launch through the C ABI into a pattern-guarded buffer (the single-frame entry:
one launch per frame). Every pixel of a specified block -- one whose reference walk ends at or before
the next block's offset -- is compared with the oracle's decode of that frame's own slot, clean frames in
full; every guard byte is compared; the pixels of the other blocks may hold anything, but only where the
entry may write. The normalised entries are compared on bit patterns (norm_helpers.table_bits).

The default range is fixed -- MH_DEFECT_SWEEP_CASES cases from MH_DEFECT_SWEEP_FIRST on, 40 from 0 -- not
time-boxed; a failure names (entry, i), which replays alone with MH_DEFECT_SWEEP_FIRST=i
MH_DEFECT_SWEEP_CASES=1."""
from __future__ import annotations

import pytest

import defect_helpers as DH

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("entry", DH.ENTRIES)
def test_defect_isolation(mh, oracle, device, entry):
    first, count = DH.sweep_range()
    assert count >= 1
    for i in range(first, first + count):
        case = DH.defect_case(mh, oracle, entry, i)
        try:
            DH.run_case(device, case)
        except Exception as e:
            raise AssertionError(f"{case.describe()}\n{type(e).__name__}: {e}") from e
