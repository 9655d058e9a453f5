"""The walk kernels of mh_check_frames / mh_check_headers in the linked library's
metadata: which kernels there are, that none spills or uses scratch, their LDS against the decode kernels',
and that their names add to none of the substring counts the other ISA tests assert."""
from __future__ import annotations

import pytest

WALKS = ("mh_walk_frames_kernel", "mh_walk_headers_kernel")


@pytest.fixture(scope="module")
def meta(mh):
    from metalhuffman_amd import isa_guard
    if not isa_guard.available():
        pytest.skip("ROCm llvm tools not found")
    return isa_guard.kernels(mh.LIB_PATH), isa_guard.resources(mh.LIB_PATH)


def test_exactly_four_walk_kernels_and_their_init(meta):
    """Each walk kernel with and without a frame-offset array -- four instantiations -- and the one init
    kernel that writes the clean reports ahead of them; nothing else carries the prefix."""
    ks, res = meta
    walk = sorted(k for k in ks if "mh_walk_" in k)
    for name in WALKS:
        assert len([k for k in walk if name in k]) == 2, (name, walk)
    assert len([k for k in walk if "mh_walk_init_kernel" in k]) == 1
    assert len(walk) == 5, walk
    assert sorted(k for k in res if "mh_walk_" in k) == walk


def test_no_scratch_no_spills_and_the_lds_budget(meta, mh):
    ks, res = meta
    multi = [k for k in res if "mh_decode_multitable_kernel" in k]
    headers = [k for k in res if "mh_decode_headers_kernel" in k]
    assert len(multi) == 2 and len(headers) == 2
    lut_bytes = 18464
    for k in (k for k in ks if "mh_walk_" in k):
        assert ks[k][:3] == (0, 0, 0), (k, ks[k])
        assert res[k]["scratch"] == 0 and res[k]["vgpr"] == ks[k][3]
        # 8 waves per SIMD: the walk hides its code loads behind other waves
        assert res[k]["vgpr"] <= 64, (k, res[k])
    for k in (k for k in res if WALKS[0] in k):
        assert res[k]["lds"] == lut_bytes <= res[multi[0]]["lds"], (k, res[k])     # the table alone
    for k in (k for k in res if WALKS[1] in k):
        assert lut_bytes < res[k]["lds"] <= res[headers[0]]["lds"], (k, res[k])     # ... and the builder's scratch
    assert [res[k]["lds"] for k in res if "mh_walk_init_kernel" in k] == [0]


def test_walk_names_collide_with_no_counted_name(meta):
    """The substring counts the other ISA tests assert are what they were."""
    ks, _ = meta
    for name, count in (("mh_decode_kernel", 2), ("mh_decode_region_kernel", 2), ("mh_decode_windows_kernel", 2),
                        ("mh_decode_region_scaled_kernel", 6), ("mh_decode_windows_scaled_kernel", 6),
                        ("mh_decode_crops_kernel", 2), ("mh_decode_normcrops_kernel", 6),
                        ("mh_decode_planes_kernel", 6), ("mh_decode_multitable_kernel", 2),
                        ("mh_decode_headers_kernel", 2), ("mh_decode_small_kernel", 2), ("mh_decode_frame_kernel", 2),
                        ("mh_check_kernel", 1), ("mh_check_init_kernel", 1)):
        got = [k for k in ks if name in k]
        assert len(got) == count, (name, got)
        assert not any("mh_walk_" in k for k in got), (name, got)
