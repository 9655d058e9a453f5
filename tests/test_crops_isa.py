"""The register and LDS budget of mh_decode_crops_kernel, read from the linked
library's code-object metadata (isa_guard.resources / isa_guard.kernels). CPU only."""
from __future__ import annotations

import pytest


def test_crops_kernel_budget(mh):
    """Exactly two instantiations (raw and delta): no scratch, no spill, at most 80 VGPRs and 53,280 B
    of static LDS -- the windows kernel's budget, three workgroups of 8 waves per CU."""
    from metalhuffman_amd import isa_guard
    if not isa_guard.available():
        pytest.skip("ROCm llvm tools not found")
    res, spills = isa_guard.resources(mh.LIB_PATH), isa_guard.kernels(mh.LIB_PATH)
    crops = sorted(k for k in res if "mh_decode_crops_kernel" in k)
    assert len(crops) == 2, crops
    assert any("ILb0E" in k for k in crops) and any("ILb1E" in k for k in crops), crops
    windows = sorted(k for k in res if "mh_decode_windows_kernel" in k)
    for k in crops:
        print(k, res[k], spills[k])
        assert res[k]["scratch"] == 0, (k, res[k])
        assert spills[k][:3] == (0, 0, 0), (k, spills[k])
        assert res[k]["vgpr"] <= 80, (k, res[k])
        assert res[k]["lds"] == 53280 == res[windows[0]]["lds"], (k, res[k])


def test_crops_kernel_name_collides_with_no_neighbour(mh):
    """The other frame-slice kernels are counted by substring: the new name adds to none of the counts."""
    from metalhuffman_amd import isa_guard
    if not isa_guard.available():
        pytest.skip("ROCm llvm tools not found")
    res = isa_guard.resources(mh.LIB_PATH)
    for name, count in (("mh_decode_kernel", 2), ("mh_decode_region_kernel", 2), ("mh_decode_windows_kernel", 2),
                        ("mh_decode_region_scaled_kernel", 6), ("mh_decode_windows_scaled_kernel", 6)):
        assert len([k for k in res if name in k]) == count, name
