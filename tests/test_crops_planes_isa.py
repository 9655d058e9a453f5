"""The register and LDS budget of mh_decode_planes_kernel, read from the
linked library's code-object metadata (isa_guard.resources / isa_guard.kernels). CPU only."""
from __future__ import annotations

import pytest

NAME = "mh_decode_planes_kernel"


def _tools():
    from metalhuffman_amd import isa_guard
    if not isa_guard.available():
        pytest.skip("ROCm llvm tools not found")
    return isa_guard


def test_planes_kernel_budget(mh):
    """Exactly six instantiations (raw and delta, times the three formats): no scratch, no spill, at
    most 80 VGPRs and the crops kernel's 53,280 B of static LDS -- three workgroups of 8 waves per
    CU, as mh_decode_normcrops_kernel."""
    isa_guard = _tools()
    res, spills = isa_guard.resources(mh.LIB_PATH), isa_guard.kernels(mh.LIB_PATH)
    planes = sorted(k for k in res if NAME in k)
    assert len(planes) == 6, planes
    for delta in ("ILb0E", "ILb1E"):
        for fmt in ("Lj0E", "Lj1E", "Lj2E"):
            assert len([k for k in planes if delta + fmt in k]) == 1, (delta, fmt, planes)
    crops = sorted(k for k in res if "mh_decode_crops_kernel" in k)
    assert len(crops) == 2
    for k in planes:
        print(k, res[k], spills[k])
        assert res[k]["scratch"] == 0, (k, res[k])
        assert spills[k][:3] == (0, 0, 0), (k, spills[k])
        assert res[k]["vgpr"] <= 80, (k, res[k])
        assert res[k]["lds"] == 53280 == res[crops[0]]["lds"], (k, res[k])


def test_planes_kernel_name_collides_with_no_neighbour(mh):
    """The other frame-slice kernels are counted by substring: the new name adds to none of the counts."""
    isa_guard = _tools()
    res = isa_guard.resources(mh.LIB_PATH)
    for name, count in (("mh_decode_kernel", 2), ("mh_decode_region_kernel", 2), ("mh_decode_windows_kernel", 2),
                        ("mh_decode_region_scaled_kernel", 6), ("mh_decode_windows_scaled_kernel", 6),
                        ("mh_decode_crops_kernel", 2), ("mh_decode_normcrops_kernel", 6),
                        ("mh_decode_multitable_kernel", 2), ("mh_decode_headers_kernel", 2)):
        assert len([k for k in res if name in k]) == count, name
        assert name not in NAME and NAME not in name


def test_planes_stage_is_the_normalised_crops(mh):
    """The output stage is NormRows, unchanged: bytes to floats by v_cvt_f32_ubyte*, the row reversed
    by v_perm_b32, a fused multiply-add, round-to-nearest-even narrowing, 16-byte stores."""
    isa_guard = _tools()
    lst = isa_guard.listings(mh.LIB_PATH)
    planes = {k: "\n".join(v) for k, v in lst.items() if NAME in k}
    assert len(planes) == 6
    for k, text in planes.items():
        for ins in ("v_cvt_f32_ubyte0", "v_cvt_f32_ubyte3", "v_perm_b32", "buffer_store_dwordx4"):
            assert ins in text, (k, ins)
        assert "v_cvt_pkrtz" not in text, k
        assert ("v_fma_f32" in text) or ("v_pk_fma_f32" in text), k
        if "Lj0E" in k:
            assert "v_cvt_pk_f16_f32" in text or "v_cvt_f16_f32" in text, k
        if "Lj1E" in k:
            assert "v_cvt_pk_bf16_f32" in text, k
