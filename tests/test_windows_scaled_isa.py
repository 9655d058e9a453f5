"""The register and LDS budget of mh_decode_windows_scaled_kernel, read from
the linked library's code-object metadata (isa_guard.resources / isa_guard.kernels), and the figures
of the kernels it was built from, which must stay those of section 3f's table. CPU only."""
from __future__ import annotations

import re

import pytest

# DESIGN.md section 3f's budget table: (VGPRs, SGPRs) by (kernel, delta[, log2_scale])
REGION_SCALED = {(0, 1): (80, 106), (0, 2): (80, 103), (0, 3): (76, 104),
                 (1, 1): (80, 106), (1, 2): (80, 102), (1, 3): (76, 102)}
WINDOWS = {0: (70, 106), 1: (70, 100)}


def _res(mh):
    from metalhuffman_amd import isa_guard
    if not isa_guard.available():
        pytest.skip("ROCm llvm tools not found")
    return isa_guard.resources(mh.LIB_PATH), isa_guard.kernels(mh.LIB_PATH)


def _inst(name):
    """(delta, log2_scale or None) from a kernel's mangled template arguments."""
    m = re.search(r"kernelILb([01])E(?:Li(\d)E)?EE", name)
    assert m, name
    return int(m.group(1)), int(m.group(2)) if m.group(2) else None


def test_windows_scaled_kernel_budget(mh):
    """Exactly six instantiations, raw and delta for each k: no scratch, no spill, at most 80 VGPRs and
    53,280 B of static LDS -- three workgroups of 8 waves per CU, as the kernels it is made of."""
    res, spills = _res(mh)
    mine = sorted(k for k in res if "mh_decode_windows_scaled_kernel" in k)
    assert len(mine) == 6, mine
    assert sorted(_inst(k) for k in mine) == [(d, k) for d in (0, 1) for k in (1, 2, 3)]
    for k in mine:
        print(k, res[k], spills[k])
        assert res[k]["scratch"] == 0, (k, res[k])
        assert spills[k][:3] == (0, 0, 0), (k, spills[k])
        assert res[k]["vgpr"] <= 80, (k, res[k])
        assert res[k]["lds"] == 53280, (k, res[k])


def test_neighbour_kernels_unchanged(mh):
    """The new name collides with neither selection by substring, and the windows and scaled-region
    kernels keep their counts and their figures."""
    res, spills = _res(mh)
    windows = sorted(k for k in res if "mh_decode_windows_kernel" in k)
    scaled = sorted(k for k in res if "mh_decode_region_scaled_kernel" in k)
    assert len(windows) == 2 and len(scaled) == 6, (windows, scaled)
    for k in windows:
        d, _ = _inst(k)
        assert (res[k]["vgpr"], res[k]["sgpr"]) == WINDOWS[d], (k, res[k])
    for k in scaled:
        assert (res[k]["vgpr"], res[k]["sgpr"]) == REGION_SCALED[_inst(k)], (k, res[k])
    for k in windows + scaled:
        assert res[k]["scratch"] == 0 and res[k]["lds"] == 53280 and spills[k][:3] == (0, 0, 0), (k, res[k], spills[k])
