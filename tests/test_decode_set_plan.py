"""The host planner of mh_decode_set_frames (mh_decode_set_plan, codec.decode_set_plan; CPU only): the
rasters dense, disjoint and aligned in frame order; the groups shared out by
clamp(round(budget * tiles_f / sum tiles), 1, ceil(tiles_f / 8)) with first_group the running sum and
a map that agrees with every share; the sizing call; every refusal; and a seeded sweep whose records
must pass a NumPy restatement of the DEVICE's validation rules with the reported out_bytes."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

INVALID, DIMS, CAPACITY = -1, -2, -4
WAVES = 8


def up(v, a):
    return (v + a - 1) // a * a


def geoms_of(sizes, first=None):
    g = np.zeros((len(sizes), 4), np.uint32)
    fb = 0
    for i, (w, h) in enumerate(sizes):
        g[i] = (fb if first is None else first[i], w, h, 0)
        fb += -(-w // 8) * -(-h // 8)
    return g


def tiles_of(w, h):
    return -(-(-(-w // 8) * -(-h // 8)) // 64)


def expected_groups(sizes, budget):
    t = [tiles_of(w, h) for w, h in sizes]
    s = sum(t)
    return [min(max((2 * budget * x + s) // (2 * s), 1), -(-x // WAVES)) for x in t]   # half rounds up


def device_accepts(geoms, plan, total_blocks, n_groups=None):
    """The device's validation (include/metalhuffman.h, mh_decode_set_frames) restated: every workgroup
    of the map must name a frame, be one of its share's, and the frame's records must pass."""
    n = len(geoms)
    n_groups = plan.n_groups if n_groups is None else n_groups
    slices = [[] for _ in range(n)]
    for g in range(n_groups):
        f = int(plan.group_frame[g])
        if f >= n:
            return False
        first, groups, r0, r1 = (int(v) for v in plan.shares[f])
        if r0 or r1 or not 1 <= groups <= 1 << 20 or g < first or g - first >= groups:
            return False
        fb, W, H, res = (int(v) for v in geoms[f])
        nb = -(-W // 8) * -(-H // 8)
        if res or not 1 <= W <= 65535 or not 1 <= H <= 65535 or nb > total_blocks or fb > total_blocks - nb:
            return False
        lo, hi, pitch, rres = (int(v) for v in plan.rasters[f])
        off, rw = lo | hi << 32, up(W, 8)
        if rres or off % 8 or pitch % 8 or pitch < rw or pitch > 1 << 20 or off + (H - 1) * pitch + rw > plan.out_bytes:
            return False
        slices[f].append(g - first)
    # every frame's slices are exactly 0 .. groups - 1: no tile lost, none repeated
    return all(sorted(s) == list(range(int(plan.shares[f][1]))) for f, s in enumerate(slices))


def check_plan(mh, sizes, budget, align=0):
    g = geoms_of(sizes)
    p = mh.decode_set_plan(g, budget, align)
    n, A = len(sizes), max(8, align)
    assert p.rasters.shape == (n, 4) and p.shares.shape == (n, 4) and p.group_frame.shape == (p.n_groups,)
    end = 0
    for f, (w, h) in enumerate(sizes):
        off, pitch = int(p.offsets[f]), int(p.pitches[f])
        assert pitch == up(w, A) and off == up(end, A) and p.rasters[f, 3] == 0, f     # dense, aligned, in order
        end = off + h * pitch
    assert p.out_bytes == end
    want = expected_groups(sizes, budget)
    assert p.shares[:, 1].tolist() == want
    assert p.shares[:, 0].tolist() == np.concatenate([[0], np.cumsum(want)[:-1]]).tolist()
    assert not p.shares[:, 2:].any()
    assert p.n_groups == sum(want)
    assert p.group_frame.tolist() == [f for f, k in enumerate(want) for _ in range(k)]
    assert device_accepts(g, p, int(g[-1, 0]) + -(-sizes[-1][0] // 8) * -(-sizes[-1][1] // 8))
    return p


def test_exported_and_python_surface(mh):
    lib = ctypes.CDLL(mh.LIB_PATH)
    assert hasattr(lib, "mh_decode_set_plan") and "mh_decode_set_plan" in mh.EXPORTS
    assert "decode_set_plan" in mh.__all__ and "DecodeSetPlan" in mh.__all__
    assert "decode_set_frames" in mh.__doc__ and "decode_set_plan" in mh.__doc__
    p = mh.decode_set_plan([(0, 9, 7, 0)], 4)
    assert isinstance(p, mh.DecodeSetPlan) and p.n_groups == 1 and p.out_bytes == 7 * 16


@pytest.mark.parametrize("budget", [1, 7, 256, 2048, 100000])
def test_layout_and_shares(mh, budget):
    sizes = [(1, 1), (8, 8), (9, 7), (512, 8), (520, 8), (8, 520), (264, 40), (1024, 512), (2048, 1536), (65535, 9)]
    check_plan(mh, sizes, budget)


def test_the_clamp_holds_at_both_ends(mh):
    # a 1x1 frame beside a large one still gets its one group, whatever the budget
    for budget in (1, 3, 1000):
        p = check_plan(mh, [(1, 1), (4096, 4096)], budget)
        assert p.shares[0, 1] == 1
    # no frame gets more groups than ceil(tiles / waves): the budget is not spent on idle workgroups
    p = check_plan(mh, [(512, 8), (520, 8), (1024, 512)], 1 << 20)
    assert p.shares[:, 1].tolist() == [1, 1, 16]             # 1, 2 and 128 tiles
    p = check_plan(mh, [(1024, 512)], 2)
    assert p.shares[0, 1] == 2 and p.n_groups == 2
    # half rounds up: two equal frames under a budget of 3 get round(1.5) = 2 each
    assert check_plan(mh, [(1024, 512), (1024, 512)], 3).shares[:, 1].tolist() == [2, 2]


@pytest.mark.parametrize("align", [0, 1, 2, 8, 16, 64, 256, 4096])
def test_pitch_align(mh, align):
    p = check_plan(mh, [(9, 7), (264, 40), (1, 1), (4097, 3)], 16, align)
    A = max(8, align)
    assert all(int(o) % A == 0 for o in p.offsets) and all(int(x) % A == 0 for x in p.pitches)


def _raw(mh, n, geoms, budget=8, align=0, cap=None, null=()):
    from metalhuffman_amd import _native as N
    g = np.ascontiguousarray(geoms, np.uint32).reshape(-1, 4)
    cap = 1 << 16 if cap is None else cap
    r, s, m = np.zeros((max(n, 1), 4), np.uint32), np.zeros((max(n, 1), 4), np.uint32), np.zeros(max(cap, 1), np.uint32)
    r[:], s[:], m[:] = 0xEE, 0xEE, 0xEE
    ng, ob = ctypes.c_uint32(0xABCD), ctypes.c_uint64(0xABCD)
    ptr = lambda name, a: None if name in null else a.ctypes.data
    rc = N.lib().mh_decode_set_plan(n, ptr("geoms", g), budget, align, ptr("rasters", r), ptr("shares", s),
                                    ptr("map", m), cap, None if "n_groups" in null else ctypes.byref(ng),
                                    None if "out_bytes" in null else ctypes.byref(ob))
    untouched = bool((r == 0xEE).all() and (s == 0xEE).all() and (m == 0xEE).all())
    return rc, ng.value, ob.value, untouched


def test_sizing_call_and_capacity(mh):
    g = geoms_of([(1024, 512), (9, 7), (2048, 1536)])
    want = expected_groups([(1024, 512), (9, 7), (2048, 1536)], 64)
    rc, ng, ob, untouched = _raw(mh, 3, g, 64, cap=0, null=("rasters", "shares", "map"))
    assert rc == CAPACITY and ng == sum(want) and ob == 1024 * 512 + 16 * 7 + 2048 * 1536
    rc, ng2, ob2, untouched = _raw(mh, 3, g, 64, cap=ng - 1)
    assert rc == CAPACITY and (ng2, ob2) == (ng, ob) and untouched            # reported, and no array written
    rc, ng3, ob3, untouched = _raw(mh, 3, g, 64, cap=ng)
    assert rc == 0 and (ng3, ob3) == (ng, ob) and not untouched


def test_refusals(mh):
    g = geoms_of([(64, 64), (9, 7)])
    assert _raw(mh, 2, g)[0] == 0
    for null in ("geoms", "n_groups", "out_bytes", "rasters", "shares", "map"):
        assert _raw(mh, 2, g, null=(null,))[0] == INVALID, null
    assert _raw(mh, 0, g)[0] == INVALID
    assert _raw(mh, 2, g, budget=0)[0] == INVALID
    for align in (3, 24, 8192, 0x80000000, 4097):
        assert _raw(mh, 2, g, align=align)[0] == INVALID, align
    for bad in ((0, 0, 8, 0), (0, 8, 0, 0), (0, 65536, 8, 0), (0, 8, 65536, 0), (0, 0xFFFFFFFF, 1, 0), (0, 8, 8, 1)):
        gg = g.copy()
        gg[1] = bad
        rc, ng, ob, untouched = _raw(mh, 2, gg)
        assert rc == DIMS and untouched, bad
    gg = g.copy()
    gg[1] = (0xFFFFFFFF, 9, 7, 0)                                  # first_block + NB does not fit 32 bits
    assert _raw(mh, 2, gg)[0] == DIMS
    gg[1] = (0xFFFFFFFF, 8, 8, 0)                                  # ... and the last block that does
    assert _raw(mh, 2, gg)[0] == 0
    # order: invalid arguments before the records are read
    gg[1] = (0, 0, 0, 0)
    assert _raw(mh, 2, gg, budget=0)[0] == INVALID
    assert _raw(mh, 2, gg, cap=0, null=("rasters", "shares", "map"))[0] == DIMS
    with pytest.raises(mh.MHError) as e:
        mh.decode_set_plan(gg, 8)
    assert e.value.status == DIMS
    with pytest.raises(mh.MHError) as e:
        mh.decode_set_plan(g, 8, 24)
    assert e.value.status == INVALID


def test_seeded_sweep_of_200_sets(mh):
    rng = np.random.default_rng(20261021)
    edge = [(1, 1), (8, 8), (9, 7), (512, 8), (520, 8), (8, 520), (264, 40), (65535, 1), (1, 65535), (4096, 4096)]
    for k in range(200):
        n = int(rng.integers(1, 300 if k % 10 == 0 else 12))
        sizes = [edge[int(rng.integers(len(edge)))] if rng.random() < 0.25
                 else (int(rng.integers(1, 2100)), int(rng.integers(1, 1600))) for _ in range(n)]
        budget = int(rng.choice([1, 2, 31, 256, 1024, 2048, 1 << 16]))
        align = int(rng.choice([0, 8, 16, 64, 4096]))
        p = check_plan(mh, sizes, budget, align)
        # the rasters are disjoint: each ends at or before the next one starts
        ends = [int(p.offsets[f]) + h * int(p.pitches[f]) for f, (_, h) in enumerate(sizes)]
        assert all(ends[f] <= int(p.offsets[f + 1]) for f in range(n - 1)) and ends[-1] == p.out_bytes
        g = geoms_of(sizes)
        total = int(g[-1, 0]) + -(-sizes[-1][0] // 8) * -(-sizes[-1][1] // 8)
        # ... and the restated device rules do reject what they should: one byte less, one block less
        short = p._replace(out_bytes=p.out_bytes - (int(p.pitches[-1]) - up(sizes[-1][0], 8)) - 1)
        assert not device_accepts(g, short, total)
        assert not device_accepts(g, p, total - 1)
