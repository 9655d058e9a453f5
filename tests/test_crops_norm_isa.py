"""The register and LDS budget of mh_decode_normcrops_kernel, read from the
linked library's code-object metadata (isa_guard.resources / isa_guard.kernels). CPU only."""
from __future__ import annotations

import pytest


def _tools():
    from metalhuffman_amd import isa_guard
    if not isa_guard.available():
        pytest.skip("ROCm llvm tools not found")
    return isa_guard


def test_normcrops_kernel_budget(mh):
    """Exactly six instantiations (raw and delta, times the three formats): no scratch, no spill, at
    most 80 VGPRs and 53,280 B of static LDS -- the crops kernel's budget, three workgroups of 8 waves
    per CU, for binary32 too."""
    isa_guard = _tools()
    res, spills = isa_guard.resources(mh.LIB_PATH), isa_guard.kernels(mh.LIB_PATH)
    norm = sorted(k for k in res if "mh_decode_normcrops_kernel" in k)
    assert len(norm) == 6, norm
    for delta in ("ILb0E", "ILb1E"):
        for fmt in ("Lj0E", "Lj1E", "Lj2E"):
            assert len([k for k in norm if delta + fmt in k]) == 1, (delta, fmt, norm)
    crops = sorted(k for k in res if "mh_decode_crops_kernel" in k)
    for k in norm:
        print(k, res[k], spills[k])
        assert res[k]["scratch"] == 0, (k, res[k])
        assert spills[k][:3] == (0, 0, 0), (k, spills[k])
        assert res[k]["vgpr"] <= 80, (k, res[k])
        assert res[k]["lds"] == 53280 == res[crops[0]]["lds"], (k, res[k])


def test_normcrops_kernel_name_collides_with_no_neighbour(mh):
    """The other frame-slice kernels are counted by substring: the new name adds to none of the counts."""
    isa_guard = _tools()
    res = isa_guard.resources(mh.LIB_PATH)
    for name, count in (("mh_decode_kernel", 2), ("mh_decode_region_kernel", 2), ("mh_decode_windows_kernel", 2),
                        ("mh_decode_region_scaled_kernel", 6), ("mh_decode_windows_scaled_kernel", 6),
                        ("mh_decode_crops_kernel", 2), ("mh_decode_multitable_kernel", 2),
                        ("mh_decode_headers_kernel", 2)):
        assert len([k for k in res if name in k]) == count, name


def test_normcrops_stage_instructions(mh):
    """The output stage as DESIGN 3j describes it, in every instantiation: the bytes become floats by
    v_cvt_f32_ubyte*, the row is reversed by v_perm_b32, the 16-bit formats narrow by the packed
    round-to-nearest-even conversions (never the round-toward-zero v_cvt_pkrtz), and the rows leave in
    16-byte stores."""
    isa_guard = _tools()
    lst = isa_guard.listings(mh.LIB_PATH)
    norm = {k: "\n".join(v) for k, v in lst.items() if "mh_decode_normcrops_kernel" in k}
    assert len(norm) == 6
    for k, text in norm.items():
        for ins in ("v_cvt_f32_ubyte0", "v_cvt_f32_ubyte3", "v_perm_b32", "buffer_store_dwordx4"):
            assert ins in text, (k, ins)
        assert "v_cvt_pkrtz" not in text, k
        assert ("v_fma_f32" in text) or ("v_pk_fma_f32" in text), k
        if "Lj0E" in k:
            assert "v_cvt_pk_f16_f32" in text or "v_cvt_f16_f32" in text, k
        if "Lj1E" in k:
            assert "v_cvt_pk_bf16_f32" in text, k
        assert "v_mul_f32" not in text or "v_rcp" in text, k   # (the tile division's only: no unfused multiply-add)
