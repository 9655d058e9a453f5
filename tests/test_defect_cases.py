"""The defect sweep's cases (defect_helpers.defect_case), checked on the CPU: over the default range of
every entry -- the cases test_gpu_defect_isolation.py and test_gpu_check_sweep.py run -- the generator
hits what the sweep is there for and keeps its caps, and the CPU decoders, which have no staging window
and read bytes past codes_bytes as zero, equal the reference on EVERY block, specified or not.

A category or cap the default range misses is mended in the generator's seeds or rates, never here.

The caps:
  * in every frame that is neither clean nor wholly replaced at least 3/4 of the blocks are specified;
  * over the default range every flavour has at least 20 damaged blocks that are specified;
  * of these at least 5 contain a zero-width stall -- under the three incomplete headers (the single
    symbol, the natural header with a quarter of its lengths zeroed, and 16x256, whose 256 codes fill
    256 of the 65536 windows). A complete code (Kraft sum 1, defect_helpers.complete) matches every
    16-bit window, so under the six other flavours no stream at all has a zero-width lookup (a truncated
    T2 is given to mh_check only), and the test asserts exactly that: no block of those flavours stalls;
  * every case leaves at least one frame asserted in full."""
from __future__ import annotations

import numpy as np
import pytest

import defect_helpers as DH

N = DH.DEFAULT_CASES


@pytest.fixture(scope="module")
def cases(mh, oracle):
    return {e: [DH.defect_case(mh, oracle, e, i) for i in range(N)] for e in DH.ALL}


def _decode_cases(cases):
    return [c for e in DH.ENTRIES for c in cases[e]]


def test_a_case_follows_from_its_name_alone(mh, oracle, cases):
    for e in ("windows", "crops_norm_planes", DH.CHECK):
        again = DH._make(oracle, e, 7)
        assert again.describe() == cases[e][7].describe()
        for a, b in zip(again.frames, cases[e][7].frames):
            assert np.array_equal(a.ef.codes, b.ef.codes) and np.array_equal(a.ef.block_offsets, b.ef.block_offsets)
    for e in DH.ALL:
        assert len({c.describe() for c in cases[e]}) == N


@pytest.mark.parametrize("entry", DH.ALL)
def test_cases_keep_the_preconditions_and_the_caps(cases, entry):
    for c in cases[entry]:
        gw, gh, W, H = c.grid
        assert 1 <= gw // 8 <= 80 and 1 <= gh // 8 <= 6 and gw - 8 < W <= gw and gh - 8 < H <= gh, c.describe()
        assert (len(c.frames) == 2) if entry == "frame" else 2 <= len(c.frames) <= 5
        assert any(f.clean for f in c.frames), c.describe()
        if c.tables == "shared":
            assert len({f.header for f in c.frames}) == 1
        for f in c.frames:
            offs, slot = f.ef.block_offsets.astype(np.int64), f.ef.codes.size
            assert slot % 16 == 0
            if f.clean and not c.t2_entries:
                assert f.report.tolist() == [0, 0, 0, 0xFFFFFFFF] and f.spec.all() and not f.damaged.any()
            if f.kind in DH.CHECK_KINDS:
                assert entry == DH.CHECK and ((np.diff(offs) < 0).any() or offs.max() > 8 * slot), c.describe()
                continue
            # what a decode entry is given: offsets in order and inside the slot
            assert (np.diff(offs) >= 0).all() and offs[-1] <= 8 * slot, c.describe()
            if not f.clean and f.kind != "replace":
                assert 4 * int(f.spec.sum()) >= 3 * f.spec.size, c.describe()
        if entry != DH.CHECK:
            assert c.t2_entries == 0
            # asserted in full: a clean frame, all of whose pixels are compared
            assert any(f.clean and f.care.all() for f in c.frames)
            for f, _ in c.rect_blocks():
                assert 0 <= f < len(c.frames)


def test_every_kind_meets_every_flavour_group(cases):
    seen = {(f.kind, DH.group_of(c.flavour)) for c in _decode_cases(cases) for f in c.frames
            if f.header == DH.FLAVOURS[c.flavour][0]}
    missing = [(k, g) for k in DH.DECODE_KINDS for g in DH.GROUPS if (k, g) not in seen]
    assert not missing, missing
    check = {(f.kind, DH.group_of(c.flavour)) for c in cases[DH.CHECK] for f in c.frames}
    assert {k for k, _ in check} >= set(DH.CHECK_KINDS) | {"none", "flip", "cut", "replace"}
    assert {g for _, g in check} == set(DH.GROUPS)
    t2 = [c for c in cases[DH.CHECK] if c.t2_entries]
    assert len(t2) >= 3 and all(c.t2_entries == 512 for c in t2)
    assert any(int(f.report[1]) > 0 for c in t2 for f in c.frames), "no escape lands past the truncated T2"
    for e in DH.ENTRIES:
        assert {c.flavour for c in cases[e]} == set(DH.FLAVOURS), e
    assert {c.tables for c in _decode_cases(cases)} == {"shared", "set"}


def test_damage_meets_tile_boundaries_and_last_blocks(cases):
    boundary = last = halves = 0
    for c in _decode_cases(cases):
        for f in c.frames:
            if f.clean or f.kind == "replace":
                continue
            d = f.damaged
            boundary += bool(d.size > 64 and d[63] and d[64])
            last += bool(d[-1])
            halves += bool(c.flavour == "16x256" and d.size > 33 and d[31:34].any())
    assert boundary >= 5 and last >= 20 and halves >= 1, (boundary, last, halves)


def test_cut_slots_lie_in_front_of_a_neighbour_at_the_end_and_alone(cases):
    """frame_code_offsets[f + 1] lowered in front of the next frame's bytes and behind the last frame,
    and codes_bytes lowered for the single-frame entry's one frame."""
    inner = sum(1 for c in _decode_cases(cases) if c.entry != "frame" for f in c.frames[:-1] if f.kind == "cut")
    final = sum(1 for c in _decode_cases(cases) if c.entry != "frame" and c.frames[-1].kind == "cut")
    alone = sum(1 for c in cases["frame"] if c.frames[0].kind == "cut")
    assert inner >= 20 and final >= 10 and alone >= 3, (inner, final, alone)
    for c in _decode_cases(cases):
        for f in c.frames:
            if f.kind == "cut":
                # (the single-symbol stream is all zero bits, so its cut-off rest is too)
                assert f.tail.size >= 16 and (f.tail.any() or f.header == "single"), c.describe()
                assert f.damaged[-1] and not f.damaged[:-1].any(), c.describe()


@pytest.mark.parametrize("flavour", list(DH.FLAVOURS))
def test_each_flavour_has_damaged_blocks_that_are_specified(cases, flavour):
    good = stalled = stalls_anywhere = 0
    for c in _decode_cases(cases):
        if c.flavour != flavour:
            continue
        for f in c.frames:
            if f.header != DH.FLAVOURS[flavour][0]:
                continue
            m = f.damaged & f.spec
            good += int(m.sum())
            stalled += int((m & (f.stalls > 0)).sum())
            stalls_anywhere += int((f.stalls > 0).sum())
    assert good >= 20, (flavour, good)
    if not DH.complete(DH.FLAVOURS[flavour][0]):
        assert stalled >= 5, (flavour, stalled)
    else:
        assert stalls_anywhere == 0, "a complete code has no zero-width lookup"


@pytest.mark.parametrize("entry", ("region", "region_scaled", "windows", "windows_scaled", "crops") + DH.NORMS)
def test_rectangles_lie_in_clean_frames_across_damage_and_inside_it(cases, entry):
    clean = mixed = inside = 0
    for c in cases[entry]:
        gbw = c.grid[0] // 8
        for f, blocks in c.rect_blocks():
            d = c.frames[f].damaged.reshape(-1, gbw)[blocks]
            clean += bool(c.frames[f].clean)
            mixed += bool(d.any() and not d.all())
            inside += bool(d.all())
    assert clean >= 10 and mixed >= 10 and inside >= 3, (entry, clean, mixed, inside)


def test_plane_samples_mix_a_clean_and_a_damaged_frame(cases):
    for c in cases["crops_norm_planes"]:
        assert any(len({c.frames[s[0] + p].clean for p in range(DH.PLANES)}) == 2 for s in c.what[0]), c.describe()
    fmts = {c.norm[0] for e in DH.NORMS for c in cases[e]}
    assert len(fmts) == 3
    for e in DH.NORMS:
        plain = [c for c in cases[e] if c.norm == (2, [(1.0, 0.0)] * len(c.norm[1]))]
        assert len(plain) == N // 2, e
        assert sum(1 for c in cases[e] for s in c.what[0] if s[3]) >= 5, "mirrored samples"


@pytest.mark.parametrize("entry", DH.ENTRIES)
def test_cpu_decoders_equal_the_reference_on_every_block(mh, cases, entry):
    """mh_decode_frame_cpu on one thread and on three, over the slot alone (codes_bytes = the slot)."""
    for c in cases[entry]:
        for j, f in enumerate(c.frames):
            for threads in (1, 3):
                got = mh.decode_frame_cpu(f.ef, threads)
                assert np.array_equal(got, f.want), (c.describe(), j, threads)
