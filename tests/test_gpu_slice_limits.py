"""The seven decode entries that go through slice_decode -- frames, headers, region, region_scaled,
windows, windows_scaled, crops -- at the limits of the frame dimensions: a 65535 x 11 frame (8192 x 2
blocks), an 11 x 65535 one (2 x 8192), a one-block 5 x 3 one, a 513 x 1 one, and rasters at the
largest pitch the host check admits (2^20). These are the values at which the geometry words the
kernels pack into registers fill: a scaled region's (W - 8 bx0) | (H - 8 by0) << 16, a crop's
dx | dy << 4 | OW << 8 with OW = 8192 and 131 segments, block rows up to 8191, bw = 8192.

Every case is one launch through the C ABI into a pattern-guarded buffer of which every byte is
checked (slice_helpers.run_contained); expected pixels are numpy slices of the oracle's decode of the
full declared frame, box-reduced at a scale. Two frames per launch, a table set for every other case
and one shared table for the rest. Each case states the segments, tiles and block rows it claims, and
the test asserts them against the host layer's rules (slice_helpers.counts)."""
from __future__ import annotations

import pytest

import region_helpers as R
import slice_helpers as SH

pytestmark = pytest.mark.gpu

CASES = []   # (geometry, label, entry, flavour, what, k, tables, expected counts)


def _add(name, label, entry, what=None, k=0, flavour="escapes", **expect):
    tables = ("set", "shared")[len(CASES) % 2]
    CASES.append((name, f"{name}-{entry}{k or ''}-{label}-{flavour}", entry, flavour, what, k, tables, expect))


def _add_scales(name, label, entry, what, **kw):
    """`entry` (region or windows) at full scale and its scaled twin at k = 1, 2, 3."""
    _add(name, label, entry, what, **kw)
    for k in (1, 2, 3):
        _add(name, label, entry + "_scaled", what, k, **kw)


def _both(f0):
    """One rectangle per frame of a two-frame launch."""
    return [(0, *f0), (1, *f0)]


# ---- wide: 65535 x 11, 8192 x 2 blocks ------------------------------------------------------------------
for e in ("frames", "headers"):
    _add("wide", "whole", e, S=128, tiles=256, rows=2)
_add_scales("wide", "whole", "region", (0, 0, 8192, 2), S=128, tiles=256)
_add_scales("wide", "last64", "region", (8128, 0, 64, 2), S=1, tiles=2)
_add_scales("wide", "w65_to_last_block", "region", (8127, 1, 65, 1), S=2, tiles=2)   # tile 2 = the frame's last block
_add_scales("wide", "last_block", "region", (8191, 1, 1, 1), S=1, tiles=1)
_add_scales("wide", "from_block_1", "region", (1, 0, 8191, 2), S=128, tiles=256)
_add_scales("wide", "whole", "windows", (_both((0, 0)), (8192, 2)), S=128, tiles=256)
WIDE_130 = ([(i % 2, bx0, by0) for i, (bx0, by0) in enumerate((bx0, by0) for bx0 in (0, 4097, 8062) for by0 in (0, 1))],
            (130, 1))
_add_scales("wide", "130x1", "windows", WIDE_130, S=3, tiles=3)
_add("wide", "whole", "crops", (_both((0, 0)), (65535, 11)), OW=8192, S=131, NB=8192, rows=3)
WIDE_DX = ([((x0 + y0) % 2, x0, y0) for y0 in (0, 7) for x0 in range(1, 9)], (65527, 4))   # dx = 1..7, 0; dy = 0, 7
_add("wide", "every_dx", "crops", WIDE_DX, OW=8191, S=131, NB=8192, rows=2)
_add("wide", "right_edge_in_bottom_row", "crops", (_both((65030, 8)), (505, 3)), OW=64, S=2, NB=64)
_add("wide", "corner", "crops", (_both((65516, 6)), (19, 5)), OW=3, S=1, NB=3)

# ---- tall: 11 x 65535, 2 x 8192 blocks ------------------------------------------------------------------
for e in ("frames", "headers"):
    _add("tall", "whole", e, S=1, tiles=256, rows=8192)
_add_scales("tall", "whole", "region", (0, 0, 2, 8192), S=1, tiles=8192, rows=8192)
_add_scales("tall", "last_block", "region", (1, 8191, 1, 1), S=1, tiles=1)
_add_scales("tall", "last_192_rows", "region", (0, 8000, 2, 192), S=1, tiles=192)
_add_scales("tall", "whole", "windows", (_both((0, 0)), (2, 8192)), S=1, tiles=8192)
TALL_100 = ([(i % 2, i % 2, by0) for i, by0 in enumerate((0, 4001, 8092))], (1, 100))
_add_scales("tall", "1x100", "windows", TALL_100, S=1, tiles=100)
_add("tall", "whole", "crops", (_both((0, 0)), (11, 65535)), OW=2, S=1, rows=8193, tiles=8193)
_add("tall", "every_dy", "crops", ([(y0 % 2, 6, y0) for y0 in range(1, 8)], (5, 65528)), OW=1, S=1, rows=8192)
_add("tall", "corner", "crops", (_both((8, 65526)), (3, 9)), OW=1, S=1, rows=2)

# ---- tiny (5 x 3, one block) and one_row (513 x 1, 65 x 1 blocks) ------------------------------------------
for name, (gbw, W, H, S_) in {"tiny": (1, 5, 3, 1), "one_row": (65, 513, 1, 2)}.items():
    for e in ("frames", "headers"):
        _add(name, "whole", e, S=S_, tiles=S_, rows=1)
    _add_scales(name, "whole", "region", (0, 0, gbw, 1), S=S_, tiles=S_)
    _add_scales(name, "whole", "windows", (_both((0, 0)), (gbw, 1)), S=S_, tiles=S_)
    _add(name, "last_pixel", "crops", (_both((W - 1, H - 1)), (1, 1)), OW=1, S=1, NB=1)
    _add(name, "whole", "crops", (_both((0, 0)), (W, H)), OW=gbw, S=S_)
_add("one_row", "449_wide", "crops", ([(x0 % 2, x0, 0) for x0 in range(57, 65)], (449, 1)), OW=57, S=1, NB=57)

# ---- the other step flavours: one case per entry and geometry -----------------------------------------------
REPRESENTATIVE = {
    "wide": {"region": (1, 0, 8191, 2), "windows": WIDE_130, "crops": WIDE_DX},
    "tall": {"region": (0, 8000, 2, 192), "windows": TALL_100, "crops": ([(y0 % 2, 6, y0) for y0 in (3, 7)], (5, 65528))},
    "tiny": {"region": (0, 0, 1, 1), "windows": (_both((0, 0)), (1, 1)), "crops": (_both((1, 1)), (4, 2))},
    "one_row": {"region": (0, 0, 65, 1), "windows": (_both((0, 0)), (65, 1)),
                "crops": ([(x0 % 2, x0, 0) for x0 in (57, 60, 64)], (449, 1))},
}
for name, rep in REPRESENTATIVE.items():
    for flavour in ("16x256", "8x256"):
        for i, e in enumerate(SH.ENTRIES):
            what = rep.get(e.replace("_scaled", ""))
            _add(name, "flavour", e, what, 1 + i % 3 if e in SH.SCALED else 0, flavour)
    for flavour in ("block_init", "no_delta"):
        _add(name, "flavour", "region", rep["region"], flavour=flavour)
        _add(name, "flavour", "crops", rep["crops"], flavour=flavour)


def test_case_list_covers_what_it_claims():
    for name in REPRESENTATIVE:
        mine = [c for c in CASES if c[0] == name]
        assert {c[2] for c in mine if c[3] == "escapes"} == set(SH.ENTRIES)
        for flavour in ("16x256", "8x256"):
            assert sorted(c[2] for c in mine if c[3] == flavour) == sorted(SH.ENTRIES)
        for flavour in ("block_init", "no_delta"):
            assert sorted(c[2] for c in mine if c[3] == flavour) == ["crops", "region"]
        assert {(c[2], c[5]) for c in mine if c[2] in SH.SCALED and c[3] == "escapes"} == \
            {(e, k) for e in SH.SCALED for k in (1, 2, 3)}
    assert len({c[1] for c in CASES}) == len(CASES)
    assert {c[6] for c in CASES} == {"set", "shared"}
    assert {c[1] & 7 for c in WIDE_DX[0]} == set(range(8)) and {c[2] & 7 for c in WIDE_DX[0]} == {0, 7}


@pytest.mark.parametrize("geom", ["tight", "loose"])
@pytest.mark.parametrize("case", CASES, ids=[c[1] for c in CASES])
def test_limit(mh, oracle, device, case, geom):
    name, _, entry, flavour, what, k, tables, expect = case
    _, _, W, H = SH.GEOMETRIES[name]
    have = SH.counts(entry, W, H, what)
    assert {key: have[key] for key in expect} == expect, (have, expect)
    frames = SH.limit_frames(mh, oracle, name, flavour, 2)
    up, tabs = SH.upload(device, frames, tables, entry)
    assert (up.frames.width, up.frames.height, up.frames.n_frames) == (W, H, 2)
    SH.run_contained(entry, device, geom, up, tabs, what, k)


# ---- the largest pitch ---------------------------------------------------------------------------------------

MAX_PITCH = 1 << 20
PITCH_CASES = {
    # entry, what, k, frames of the launch. Crops: dy = 7 and dy = 1 -- the rows of the first block row
    # above a crop, dy x pitch bytes in front of it, would land in the lead guard (slot 0) or in slot 0
    # (slot 1)
    "crops": ("crops", ([(0, 3, 7), (1, 520, 57)], (77, 3)), 0, 2),
    "windows_scaled": ("windows_scaled", ([(0, 0, 0), (1, 65, 6), (2, 30, 2)], (10, 3)), 3, 3),
    "region": ("region", R.REGIONS["bottom_edge"], 0, 1),
}


@pytest.mark.parametrize("name", list(PITCH_CASES))
def test_maximum_pitch(mh, oracle, device, name):
    """pitch = 2^20, the largest check_decode_args admits, on region_helpers' base frame; lead and tail
    guards of 8 x pitch, so a row stored one block row above or below a raster still lands inside the
    checked buffer. One geometry, d_out % 16 == 8; the slots are exactly rows x pitch apart."""
    entry, what, k, n = PITCH_CASES[name]
    if entry == "crops":
        assert [c[2] & 7 for c in what[0]] == [7, 1] and all(c[1] + 77 <= R.W and c[2] + 3 <= R.H for c in what[0])
    frames = R.frame_set(mh, oracle, "general")[:n]
    up, tabs = SH.upload(device, frames, "shared", entry)
    _, rows, _ = SH.slots_of(entry, up, what, k)
    lead = 8 * MAX_PITCH + 8
    SH.run_contained(entry, device, (MAX_PITCH, rows * MAX_PITCH, lead, 8 * MAX_PITCH), up, tabs, what, k)
