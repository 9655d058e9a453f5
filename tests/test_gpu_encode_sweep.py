"""A seeded sweep over the GPU encoders: mh_encode_frame_device_async (n calls over one workspace),
mh_encode_frames_device_async and mh_encode_frames_shared_device_async with a built and with a
supplied header, over grids of 1..200 x 1..24 blocks with W and H anywhere in the last block, 1..5
frames, the pixels at any byte offset and frame stride inside garbage, both formats and the init
bytes, MH_ENCODE_LIMIT_LENGTHS, a zeroed or garbage workspace, every output at its own offset inside
guards, a roomy, exactly fitting or too small slot, and now and then a frame whose tree is deeper
than 16 (encode_helpers.sweep_case; the cases' coverage is asserted on the CPU in
test_encode_sweep_cases.py).

Every case is checked against the host codec byte for byte and guard for guard
(encode_helpers.check) and decoded back on the device. The default range is fixed --
MH_ENCODE_SWEEP_CASES cases from MH_ENCODE_SWEEP_FIRST on, 48 from 0 -- so it is the same on every
machine; a failure names (entry, i), which replays alone with MH_ENCODE_SWEEP_FIRST=i
MH_ENCODE_SWEEP_CASES=1."""
from __future__ import annotations

import pytest

import encode_helpers as EH

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("entry", EH.ENTRIES)
def test_encode_sweep(mh, device, bigbridge, entry):
    first, count = EH.sweep_range()
    assert count >= 1
    for i in range(first, first + count):
        EH.run_sweep_case(mh, device, EH.sweep_case(entry, i), bigbridge)
    print(f"{entry}: seen so far: {EH.SEEN}")
