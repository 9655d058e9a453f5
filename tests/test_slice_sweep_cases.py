"""The seeded slice sweep's cases (slice_helpers.sweep_case), checked on the CPU: over the default
range of every entry -- the cases test_gpu_slice_sweep.py runs -- every case builds and is one the
host check accepts, its frames decode (oracle) to their source images, and the categories the sweep
is there for are all hit. A category the default range misses is mended in the generator's seed or
weights, never here."""
from __future__ import annotations

import pytest

import slice_helpers as SH

N = SH.SWEEP_DEFAULT_CASES
CASES = {e: [SH.sweep_case(e, i) for i in range(N)] for e in SH.ENTRIES}


def _segments(c):
    _, _, W, H = c.grid
    return SH.counts(c.entry, W, H, c.what)["S"]


def test_a_case_follows_from_its_name_alone():
    for e in SH.ENTRIES:
        assert [SH.sweep_case(e, i) for i in range(N)] == CASES[e]
        assert len({c.describe() for c in CASES[e]}) == N
    assert SH.sweep_case("crops", 3) != SH.sweep_case("windows", 3)


@pytest.mark.parametrize("entry", SH.ENTRIES)
def test_cases_are_accepted_by_the_host_rules(entry):
    """Every rectangle is non-empty and inside the grid (windows, regions) or the declared frame
    (crops); every window and crop names a frame of the launch."""
    for c in CASES[entry]:
        gw, gh, W, H = c.grid
        gbw, gbh = gw // 8, gh // 8
        assert 1 <= gbw <= 200 and 1 <= gbh <= 24 and gw - 8 < W <= gw and gh - 8 < H <= gh, c.describe()
        assert 1 <= len(c.frames) <= 3 and c.geom in ("tight", "loose") and c.tables in ("shared", "set")
        assert c.frames[0][0] == SH.FLAVOURS[c.flavour][0]
        if c.tables == "shared":
            assert len({h for h, _ in c.frames}) == 1
        assert (c.k in (1, 2, 3)) if entry in SH.SCALED else c.k == 0
        if entry in ("region", "region_scaled"):
            bx0, by0, bw, bh = c.what
            assert bw >= 1 and bh >= 1 and 0 <= bx0 and bx0 + bw <= gbw and 0 <= by0 and by0 + bh <= gbh, c.describe()
        elif entry in ("windows", "windows_scaled", "crops"):
            rects, (w, h) = c.what
            tw, th = (W, H) if entry == "crops" else (gbw, gbh)
            assert 1 <= len(rects) <= 5 and 1 <= w <= tw and 1 <= h <= th
            for f, x0, y0 in rects:
                assert 0 <= f < len(c.frames) and 0 <= x0 and x0 + w <= tw and 0 <= y0 and y0 + h <= th, c.describe()
        else:
            assert c.what is None


@pytest.mark.parametrize("entry", SH.ENTRIES)
def test_every_case_builds(mh, oracle, entry):
    """slice_helpers.one_frame asserts that the oracle's decode of each declared frame is the image."""
    for c in CASES[entry]:
        frames = SH.sweep_frames(mh, oracle, c)
        _, _, W, H = c.grid
        assert len(frames) == len(c.frames)
        for (ef, want), (header, _) in zip(frames, c.frames):
            assert (ef.width, ef.height) == (W, H) and want.shape == (H, W)
            assert (ef.canon == SH.headers()[header].canon).all()


def test_the_entries_together_hit_every_flavour():
    seen = {c.flavour for e in SH.ENTRIES for c in CASES[e]}
    assert seen == set(SH.FLAVOURS)
    assert {h for e in SH.ENTRIES for c in CASES[e] for h, _ in c.frames} == set(SH.HEADERS)
    assert {c.tables for e in SH.ENTRIES for c in CASES[e]} == {"shared", "set"}


def _ends_right(c):
    _, _, W, _ = c.grid
    return W % 8 != 0 and any(x0 + w == W for _, x0, _, w, _ in c.rects())


def _ends_bottom(c):
    _, _, _, H = c.grid
    return H % 8 != 0 and any(y0 + h == H for _, _, y0, _, h in c.rects())


CATEGORIES = {
    "S >= 3": lambda c: _segments(c) >= 3,
    "GBW in {63, 64, 65}": lambda c: c.grid[0] // 8 in (63, 64, 65),
    "a rectangle ends on the right edge, W % 8 != 0": _ends_right,
    "a rectangle ends on the bottom edge, H % 8 != 0": _ends_bottom,
    "GBH == 1": lambda c: c.grid[1] == 8,
}


@pytest.mark.parametrize("entry", SH.ENTRIES)
@pytest.mark.parametrize("category", list(CATEGORIES))
def test_category_is_hit_twice(entry, category):
    hits = [c.i for c in CASES[entry] if CATEGORIES[category](c)]
    assert len(hits) >= 2, (entry, category, hits)


def test_crops_hit_every_sub_block_origin_twice():
    dx, dy = [0] * 8, [0] * 8
    for c in CASES["crops"]:
        for _, x0, y0 in c.what[0]:
            dx[x0 & 7] += 1
            dy[y0 & 7] += 1
    assert min(dx) >= 2 and min(dy) >= 2, (dx, dy)


@pytest.mark.parametrize("entry", SH.SCALED)
@pytest.mark.parametrize("k", [1, 2, 3])
def test_scaled_entries_hit_every_scale_with_an_odd_last_cell(entry, k):
    """A rectangle whose width or height is no multiple of 2^k: its last cell averages fewer pixels."""
    s = 1 << k
    hits = [c.i for c in CASES[entry] if c.k == k and any(w % s or h % s for _, _, _, w, h in c.rects())]
    assert len(hits) >= 2, (entry, k, hits)
