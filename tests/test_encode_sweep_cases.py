"""The seeded encode sweep's cases (encode_helpers.sweep_case), checked on the CPU: over the default
range of every entry -- the cases test_gpu_encode_sweep.py runs -- every case follows from its name,
the host codec gives every frame's expected status (a rejection is an expected value, never a reason
to drop a case), and the categories the sweep is there for are all hit. A category the default range
misses is mended in the generator's seed or weights, never here."""
from __future__ import annotations

import pytest

import encode_helpers as EH

N = EH.SWEEP_DEFAULT_CASES
CASES = {e: [EH.sweep_case(e, i) for i in range(N)] for e in EH.ENTRIES}
_PLANS: dict = {}


def _plan(mh, bigbridge, c):
    if (c.entry, c.i) not in _PLANS:
        _PLANS[c.entry, c.i] = EH.sweep_plan(mh, c, bigbridge)
    return _PLANS[c.entry, c.i]


def _statuses(mh, bigbridge, c):
    return [s for s, _ in _plan(mh, bigbridge, c)[3].frames]


def test_a_case_follows_from_its_name_alone():
    for e in EH.ENTRIES:
        assert [EH.sweep_case(e, i) for i in range(N)] == CASES[e]
        assert len({c.describe() for c in CASES[e]}) == N
    assert EH.sweep_case("batch", 3) != EH.sweep_case("single", 3)


@pytest.mark.parametrize("entry", EH.ENTRIES)
def test_cases_are_inside_the_drawn_ranges(entry):
    g = 4 if entry == "single" else 16
    for c in CASES[entry]:
        assert 1 <= c.bw <= 200 and 1 <= c.bh <= 24 and 8 * c.bw - 8 < c.W <= 8 * c.bw and 8 * c.bh - 8 < c.H <= 8 * c.bh
        assert 1 <= c.n <= 5 and 0 <= c.layout.delta <= 15 and c.pad_kind in EH.PAD_KINDS and c.fit in EH.FITS
        pad = c.stride - c.W * c.H
        assert {"none": pad == 0, "8": pad == 8, "odd": pad % 2 == 1 and pad < 64, "large": pad >= 4096}[c.pad_kind]
        assert c.layout.codes_off % g == 0 and c.layout.offs_off % 4 == 0 and c.layout.len_off % 8 == 0
        assert c.layout.status_off % 4 == 0
        if c.deep is not None:
            assert 0 <= c.deep < c.n and c.W % 8 == 0 and c.H % 8 == 0 and c.bw * c.bh >= EH.DEEP_MIN_BLOCKS


@pytest.mark.parametrize("entry", EH.ENTRIES)
def test_the_host_codec_gives_every_expected_status(mh, bigbridge, entry):
    """Every case has a plan; the deep frame is -3 without the limit flag where the frame has its
    own tree, and encodes under lengths of at most 16 with it; a slot is never larger than roomy."""
    for c in CASES[entry]:
        imgs, header, slot, exp = _plan(mh, bigbridge, c)
        assert len(imgs) == c.n == len(exp.frames) and all(im.shape == (c.H, c.W) for im in imgs)
        assert len({im.tobytes() for im in imgs}) == c.n or c.W * c.H < 64, c.describe()
        assert (header is not None) == (entry == "shared_supplied")
        assert 0 < slot <= EH.roomy_slot(c.W, c.H) and slot % (4 if entry == "single" else 16) == 0
        for f, (s, ef) in enumerate(exp.frames):
            assert s in (EH.OK, EH.TOO_LONG, EH.CAPACITY, EH.TABLE) and (ef is not None) == (s == EH.OK)
            if s == EH.OK:
                assert EH.r4(ef.codes.size) <= slot and ef.canon.max() <= 16
        if c.fit == "exact" and any(s == EH.OK for s, _ in exp.frames):
            g = 4 if entry == "single" else 16
            assert max(-(-EH.r4(ef.codes.size) // g) * g for s, ef in exp.frames if s == EH.OK) == slot
        if c.deep is not None and entry in ("single", "batch"):
            s, ef = exp.frames[c.deep]
            if not c.limit:
                assert s == EH.TOO_LONG, c.describe()
            else:
                assert s == EH.CAPACITY or ef.canon.max() == 16, c.describe()


def _rejected_beside_accepted(mh, bigbridge, c):
    st = _statuses(mh, bigbridge, c)
    return any(s == EH.OK for s in st) and any(s != EH.OK for s in st)


CATEGORIES = {
    "byte loads (vec 0)": lambda c: not c.vec(),
    "8-byte loads (vec 1)": lambda c: c.vec() and not c.pair(),
    "delta % 8 != 0 with W % 8 == 0": lambda c: c.layout.delta % 8 != 0 and c.W % 8 == 0,
    "stride padding none": lambda c: c.pad_kind == "none",
    "stride padding 8": lambda c: c.pad_kind == "8",
    "stride padding odd": lambda c: c.pad_kind == "odd",
    "stride padding large": lambda c: c.pad_kind == "large",
    "exact-fit slot": lambda c: c.fit == "exact",
    "width in blocks < 16": lambda c: c.bw < 16,
    "garbage workspace": lambda c: c.ws_fill is not None,
    "limit flag": lambda c: c.limit,
    "init bytes": lambda c: c.init_zero,
    "no delta": lambda c: c.no_delta,
}


@pytest.mark.parametrize("entry", EH.ENTRIES)
@pytest.mark.parametrize("category", list(CATEGORIES))
def test_category_is_hit_twice(entry, category):
    hits = [c.i for c in CASES[entry] if CATEGORIES[category](c)]
    assert len(hits) >= 2, (entry, category, hits)


@pytest.mark.parametrize("entry", EH.BATCHED)
def test_batched_entries_hit_the_pair_loads_twice(entry):
    """kPair: 8-byte aligned rows and an even width in blocks; also at a frame address that is
    only 8-byte aligned (delta or stride = 8 mod 16), where the 16-byte load is not aligned."""
    hits = [c.i for c in CASES[entry] if c.pair()]
    odd8 = [c.i for c in CASES[entry] if c.pair() and (c.layout.delta % 16 == 8 or (c.n > 1 and c.stride % 16 == 8))]
    assert len(hits) >= 2 and len(odd8) >= 1, (entry, hits, odd8)


@pytest.mark.parametrize("entry", EH.ENTRIES)
def test_a_rejected_frame_beside_accepted_ones_twice(mh, bigbridge, entry):
    hits = [c.i for c in CASES[entry] if _rejected_beside_accepted(mh, bigbridge, c)]
    assert len(hits) >= 2, (entry, hits)


def test_deep_frames_are_rejected_and_limited():
    """One case in six or so brings a deep frame; both expectations (-3, limited lengths) occur."""
    deep = [c for e in EH.ENTRIES for c in CASES[e] if c.deep is not None]
    assert len(deep) >= 12 and {c.limit for c in deep if c.entry in ("single", "batch")} == {False, True}
    assert {c.entry for c in deep} == set(EH.ENTRIES)


# ---- the threshold shapes of test_gpu_encode_layouts.py ---------------------------------------------------

@pytest.mark.parametrize("entry", EH.ENTRIES)
def test_threshold_shapes_produce_the_counts(entry):
    """Per width in blocks, the block counts bracket each of kStepBlocks = 16, one tile (kCodeTile =
    128 fused, kBatchTile = 256 batched) and kPackWaves = 4 tiles as tightly as that width allows:
    on it, one block row below and one above where the width divides it, else the two counts around
    it. Every shape is bw blocks wide with W % 8 in {0, 1}; over all widths every target is hit
    exactly and the tile count takes 1, 2, kPackWaves and kPackWaves + 1."""
    tile = EH.tile_blocks(entry)
    assert tile == (128 if entry == "single" else 256)
    assert EH.threshold_targets(entry) == (16, tile, 4 * tile)
    exact, tiles = set(), set()
    for bw in EH.THRESHOLD_WIDTHS:
        shapes = EH.threshold_shapes(entry, bw)
        assert all(EH.blocks(w, h)[0] == bw for w, h in shapes)
        assert {w % 8 for w, _ in shapes} == {0, 1}
        assert {h % 8 for _, h in shapes} <= {0, 3}
        counts = sorted({bw * EH.blocks(w, h)[1] for w, h in shapes})
        tiles.update(-(-c // tile) for c in counts)
        for t in EH.threshold_targets(entry):
            if t % bw == 0:
                exact.add(t)
                assert t in counts and t + bw in counts and (t - bw in counts or t == bw), (bw, t, counts)
            else:
                assert t // bw * bw + bw in counts and (t // bw * bw in counts or t < bw), (bw, t, counts)
    assert exact == set(EH.threshold_targets(entry))
    assert {1, 2, EH.K_PACK_WAVES, EH.K_PACK_WAVES + 1} <= tiles
    assert {15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257} <= set(EH.THRESHOLD_WIDTHS)


def test_the_constants_are_the_kernels():
    """encode_helpers names mh_encode.hip's constants; the source says the same."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metalhuffman_amd", "csrc",
                            "mh_encode.hip")).read()
    for name, value in (("kStepBlocks", EH.K_STEP_BLOCKS), ("kCodeTile", EH.K_CODE_TILE), ("kBatchTile", EH.K_BATCH_TILE),
                        ("kPackWaves", EH.K_PACK_WAVES), ("kReduceTiles", EH.K_REDUCE_TILES),
                        ("kFusedMaxTiles", EH.K_FUSED_MAX_TILES)):
        m = re.search(rf"constexpr uint32_t {name} = ([^;]+);", src)
        expr = re.sub(r"kReduceDepth", re.search(r"constexpr uint32_t kReduceDepth = (\d+);", src).group(1), m.group(1))
        assert re.fullmatch(r"[\d *]+", expr) and eval(expr) == value, name
