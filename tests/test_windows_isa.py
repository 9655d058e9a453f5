"""The register and LDS budget of mh_decode_windows_kernel, read from the
linked library's code-object metadata (isa_guard.resources). CPU only."""
from __future__ import annotations

import pytest


def test_windows_kernel_budget(mh):
    """Both instantiations (raw and delta): no scratch, at most 80 VGPRs, and 53,280 B of static LDS
    -- three workgroups of 8 waves per CU, as the region kernel."""
    from metalhuffman_amd import isa_guard
    if not isa_guard.available():
        pytest.skip("ROCm llvm tools not found")
    res = isa_guard.resources(mh.LIB_PATH)
    windows = sorted(k for k in res if "mh_decode_windows_kernel" in k)
    region = sorted(k for k in res if "mh_decode_region_kernel" in k)
    assert len(windows) == 2 and len(region) == 2, (windows, region)
    assert any("ILb0E" in k for k in windows) and any("ILb1E" in k for k in windows), windows
    for k in windows:
        print(k, res[k])
        assert res[k]["scratch"] == 0, (k, res[k])
        assert res[k]["vgpr"] <= 80, (k, res[k])
        assert res[k]["lds"] == 53280 == res[region[0]]["lds"], (k, res[k])
    spills = isa_guard.kernels(mh.LIB_PATH)
    for k in windows:
        assert spills[k][:3] == (0, 0, 0), (k, spills[k])
