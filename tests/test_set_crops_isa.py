"""The register and LDS budget of the frame-set kernels, mh_decode_setcrops_kernel and
mh_decode_setplanes_kernel, read from the linked library's code-object metadata
(isa_guard.resources / isa_guard.kernels). CPU only."""
from __future__ import annotations

import pytest

CROPS, PLANES = "mh_decode_setcrops_kernel", "mh_decode_setplanes_kernel"
PARENTS = {CROPS: "mh_decode_crops_kernel", PLANES: "mh_decode_planes_kernel"}


def _tools():
    from metalhuffman_amd import isa_guard
    if not isa_guard.available():
        pytest.skip("ROCm llvm tools not found")
    return isa_guard


def _pair(k):
    """The (delta, format) template arguments in a mangled kernel name."""
    return tuple(t for t in ("ILb0E", "ILb1E", "Lj0E", "Lj1E", "Lj2E") if t in k)


def test_set_kernels_budget(mh):
    """Exactly 2 and 6 instantiations; each has no scratch, no spill, at most its parent's VGPRs (the
    planes kernel's limit is 80) and the same 53,280 B of static LDS -- three workgroups of eight
    waves per CU, as the parents."""
    isa_guard = _tools()
    res, spills = isa_guard.resources(mh.LIB_PATH), isa_guard.kernels(mh.LIB_PATH)
    crops = sorted(k for k in res if CROPS in k)
    planes = sorted(k for k in res if PLANES in k)
    assert len(crops) == 2 and len(planes) == 6, (crops, planes)
    assert sorted(_pair(k) for k in crops) == [("ILb0E",), ("ILb1E",)]
    assert sorted(_pair(k) for k in planes) == [(d, f) for d in ("ILb0E", "ILb1E") for f in ("Lj0E", "Lj1E", "Lj2E")]
    for name, mine in ((CROPS, crops), (PLANES, planes)):
        parents = {_pair(k): k for k in res if PARENTS[name] in k}
        assert len(parents) == len(mine)
        for k in mine:
            parent = res[parents[_pair(k)]]
            print(k, res[k], spills[k], "parent", parent)
            assert res[k]["scratch"] == 0, (k, res[k])
            assert spills[k][:3] == (0, 0, 0), (k, spills[k])
            assert res[k]["vgpr"] <= parent["vgpr"] <= 80, (k, res[k], parent)
            assert res[k]["lds"] == 53280 == parent["lds"], (k, res[k])


def test_set_kernel_names_collide_with_no_neighbour(mh):
    """The other frame-slice kernels are counted by substring (tests/test_crops_planes_isa.py): the new
    names add to none of those counts, nor to each other's."""
    isa_guard = _tools()
    res = isa_guard.resources(mh.LIB_PATH)
    for name, count in (("mh_decode_kernel", 2), ("mh_decode_region_kernel", 2), ("mh_decode_windows_kernel", 2),
                        ("mh_decode_region_scaled_kernel", 6), ("mh_decode_windows_scaled_kernel", 6),
                        ("mh_decode_crops_kernel", 2), ("mh_decode_normcrops_kernel", 6),
                        ("mh_decode_planes_kernel", 6), ("mh_decode_multitable_kernel", 2),
                        ("mh_decode_headers_kernel", 2)):
        assert len([k for k in res if name in k]) == count, name
        for mine in (CROPS, PLANES):
            assert name not in mine and mine not in name
    assert CROPS not in PLANES and PLANES not in CROPS


def test_set_planes_stage_is_the_normalised_crops(mh):
    """The output stage is NormRows, unchanged: bytes to floats by v_cvt_f32_ubyte*, the row reversed
    by v_perm_b32, a fused multiply-add, round-to-nearest-even narrowing, 16-byte stores."""
    isa_guard = _tools()
    lst = isa_guard.listings(mh.LIB_PATH)
    planes = {k: "\n".join(v) for k, v in lst.items() if PLANES in k}
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


def test_set_entries_load_the_record_behind_the_descriptor(mh):
    """Both entries make two 16-byte loads ahead of the body's prologue -- the descriptor, then the
    geometry record (the planes entry: one per plane) -- and the crops entry's body is the crops
    kernel's: the same count of row stores."""
    isa_guard = _tools()
    lst = isa_guard.listings(mh.LIB_PATH)
    count = lambda k, ins: sum(1 for line in lst[k] if line.split()[0] == ins)
    for k in lst:
        if CROPS in k:
            parent = next(q for q in lst if PARENTS[CROPS] in q and _pair(q) == _pair(k))
            assert count(k, "buffer_load_dwordx4") == count(parent, "buffer_load_dwordx4") + 1, k
            assert count(k, "buffer_store_dwordx2") == count(parent, "buffer_store_dwordx2"), k
        if PLANES in k:
            parent = next(q for q in lst if PARENTS[PLANES] in q and _pair(q) == _pair(k))
            assert count(k, "buffer_load_dwordx4") == count(parent, "buffer_load_dwordx4") + 4, k
            assert count(k, "buffer_store_dwordx4") == count(parent, "buffer_store_dwordx4"), k
