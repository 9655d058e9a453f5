"""A seeded sweep over the image encoders: mh_encode_images_device_async and
mh_encode_images_shared_device_async with a built and with a supplied header, 14 cases each
(encode_images_helpers.sweep_case): grids of 1..40 x 1..6 blocks with W and H anywhere in the last
block, 1..3 images, 1..4 planes in turn, both frame orders, every other case on an aligned layout of
pixel stride 2..4 (the dword loads) and the rest at any stride, pitch, base offset and image gap (the
byte loads), both formats and the init bytes, MH_ENCODE_LIMIT_LENGTHS, a zeroed or garbage
workspace. That the cases reach both load paths, every C and both orders is asserted on the CPU in
test_encode_images_abi.py.

Every case is checked against the host codec on codec.image_planes byte for byte and guard for
guard, twice over one workspace, and decoded back on the device; a failure names its case."""
from __future__ import annotations

import pytest

import encode_images_helpers as IH

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("entry", IH.ENTRIES)
def test_encode_images_sweep(mh, device, bigbridge, entry):
    for i in range(IH.SWEEP_CASES):
        case = IH.sweep_case(entry, i)
        pix = IH.natural_pixels(bigbridge, case.W, case.H, case.n, case.px, seed=100 * IH.ENTRIES.index(entry) + i)
        try:
            IH.run_checked(mh, device, entry, pix, case.px, flags=case.flags, init_zero=case.init_zero, ws_fill=case.ws_fill)
        except AssertionError as err:
            raise AssertionError(f"{case}: {err}") from err
