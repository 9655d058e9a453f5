"""mh_decode_region_scaled: a region of every frame at 1/2, 1/4 or 1/8 scale in one launch. Expected
values are scaled_helpers.box_reduce_np (the numpy statement of the definition: in-frame means,
halves rounded up) of the region's crop of the oracle's decode of the FULL frame -- never another
GPU decode alone. Every raster is prefilled with 0xA5. Bit-exact.

The base frame is region_helpers' 600 x 72 grid declared 597 x 67: its right-edge block has 5
columns and its bottom block row 3 rows, so partial cells have n = 2, 1 (k = 1), 4, 12, 3 (k = 2)
and 40, 24, 15 (k = 3) pixels. The second size, 595 x 70, has 3 columns and 6 rows there."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

import region_helpers as R
import scaled_helpers as S
from region_helpers import FLAVOURS, REGIONS

pytestmark = pytest.mark.gpu

KS = (1, 2, 3)


def _efs(frames):
    return [f[0] for f in frames]


def _wants(frames):
    return [f[1] for f in frames]


# ---- 1. the base frame: every region, scale and step flavour ---------------------------------------

@pytest.mark.parametrize("flavour", FLAVOURS)
def test_flavours(mh, oracle, device, flavour):
    """Every region of the base frame at k = 1, 2, 3 under each step flavour, three frames of one
    shared table per launch: both loops (batch_loop's three steps, flat8_loop), both slow paths
    (off_grid, oversize: decode_halves), no_delta and block_init all end in the reducing stage."""
    frames = R.frame_set(mh, oracle, flavour)
    fr, tabs = R.upload(device, _efs(frames))
    assert fr.n_frames == 3
    for name, region in REGIONS.items():
        for k in KS:
            got = S.decode_scaled_host(device, fr, tabs, region, k)
            S.check_scaled(got, region, k, _wants(frames), R.W, R.H)


def test_partial_cell_counts():
    """The pixel counts of the base frame's partial cells named above (pure arithmetic)."""
    def counts(w, h, k):
        s = 1 << k
        ones = S.box_reduce_np(np.full((h, w), 1, np.uint8), 0).astype(np.int64)
        pad = np.zeros((-(-h // s) * s, -(-w // s) * s), np.int64)
        pad[:h, :w] = ones
        n = pad.reshape(pad.shape[0] // s, s, pad.shape[1] // s, s).sum(axis=(1, 3))
        return set(np.unique(n).tolist()) - {s * s}
    assert counts(R.W, R.H, 1) == {2, 1} and counts(R.W, R.H, 2) == {4, 12, 3} and counts(R.W, R.H, 3) == {40, 24, 15}


# ---- 2. the other residues: 595 x 70 ---------------------------------------------------------------

@pytest.mark.parametrize("name", ["full", "right_edge", "bottom_edge", "last_block"])
def test_second_size(mh, oracle, device, name):
    """Declared 595 x 70: 3 columns in the right-edge block (cell widths 2, 1 / 3 / 3) and 6 rows in
    the bottom block row (cell heights 2 x 3 / 4, 2 / 6)."""
    W2, H2 = 595, 70
    frames = R.frame_set(mh, oracle, "general", width=W2, height=H2)
    fr, tabs = R.upload(device, _efs(frames))
    assert (fr.width, fr.height) == (W2, H2)
    for k in KS:
        got = S.decode_scaled_host(device, fr, tabs, REGIONS[name], k)
        S.check_scaled(got, REGIONS[name], k, _wants(frames), W2, H2)


# ---- 3. saturation and ties --------------------------------------------------------------------------

def _flat8_raw(mh, oracle, img):
    """A no_delta frame of `img` (grid sized) under the flat 8-bit header, declared 597 x 67."""
    from helpers import encode_with_header
    ef = encode_with_header(np.full(256, 8, np.uint8), mh.split_blocks(img), R.GRID_W, R.GRID_H, no_delta=True)
    ef = dataclasses.replace(ef, width=R.W, height=R.H)
    want = R.oracle_decode(oracle, ef)
    assert np.array_equal(want, img[:R.H, :R.W])
    return ef, want


@pytest.mark.parametrize("pattern", ["all255", "checker"])
def test_saturation_and_ties(mh, oracle, device, pattern):
    """All 255: every mean is 255, partial cells included (no carry out of a byte, no darkened
    edge). A 0 / 255 checkerboard: every full cell is a tie, 127.5 -> 128."""
    yy, xx = np.mgrid[0:R.GRID_H, 0:R.GRID_W]
    img = np.full((R.GRID_H, R.GRID_W), 255, np.uint8) if pattern == "all255" else (((yy + xx) & 1) * 255).astype(np.uint8)
    ef, want = _flat8_raw(mh, oracle, img)
    fr, tabs = R.upload(device, [ef])
    for k in KS:
        got = S.decode_scaled_host(device, fr, tabs, REGIONS["full"], k)
        S.check_scaled(got, REGIONS["full"], k, [want], R.W, R.H)
        sw, sh, _ = S.scaled_size(REGIONS["full"], k, R.W, R.H)
        if pattern == "all255":
            assert (got[0, :, :sw] == 255).all()
        else:
            assert (got[0, : R.H >> k, : R.W >> k] == 128).all()      # the full cells


# ---- 4. relations ------------------------------------------------------------------------------------

def test_scale_one_is_decode_region(mh, oracle, device):
    """k = 0 forwards to mh_decode_region: byte-identical rasters, the pitch padding included."""
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames))
    for name in ("full", "w65", "last_block"):
        assert np.array_equal(S.decode_scaled_host(device, fr, tabs, REGIONS[name], 0),
                              R.decode_region_host(device, fr, tabs, REGIONS[name])), name


@pytest.mark.parametrize("k", KS)
def test_scaled_region_is_rectangle_of_scaled_frame(mh, oracle, device, k):
    """A region starts on a block and s divides 8: its cells are the whole frame's cells."""
    frames = R.frame_set(mh, oracle, "general14")
    fr, tabs = R.upload(device, _efs(frames))
    full = S.decode_scaled_host(device, fr, tabs, REGIONS["full"], k)
    c = 8 >> k
    for name, region in REGIONS.items():
        got = S.decode_scaled_host(device, fr, tabs, region, k)
        bx0, by0, bw, bh = region
        assert np.array_equal(got, full[:, by0 * c: by0 * c + got.shape[1], bx0 * c: (bx0 + bw) * c]), name


def _three_tables(mh, oracle):
    frames = [R.frame_set(mh, oracle, fl)[i] for i, fl in enumerate(("general", "noesc", "flat4"))]
    assert len({f[0].canon.tobytes() for f in frames}) == 3
    return frames


@pytest.mark.parametrize("k", KS)
def test_table_per_frame(mh, oracle, device, k):
    """Three frames with three distinct headers (a DeviceTableSet): three step flavours in one launch."""
    frames = _three_tables(mh, oracle)
    fr, ts = R.upload(device, _efs(frames), "set")
    assert ts.status.cpu().tolist() == [0, 0, 0]
    for name in ("w65", "right_edge", "bottom_edge", "last_block"):
        S.check_scaled(S.decode_scaled_host(device, fr, ts, REGIONS[name], k), REGIONS[name], k, _wants(frames), R.W, R.H)


def test_skips_rejected_frame(mh, oracle, device):
    """A non-zero status word on the middle frame keeps its fill; skip_rejected=False decodes it."""
    frames = _three_tables(mh, oracle)
    fr, ts = R.upload(device, _efs(frames), "set")
    ts.status[1] = -3
    region = REGIONS["w70"]
    for k in KS:
        got = S.decode_scaled_host(device, fr, ts, region, k)
        assert (got[1] == R.FILL).all()
        S.check_scaled(got[[0, 2]], region, k, [frames[0][1], frames[2][1]], R.W, R.H)
        S.check_scaled(S.decode_scaled_host(device, fr, ts, region, k, skip_rejected=False), region, k, _wants(frames),
                       R.W, R.H)


def test_decode_scaled_view_and_arguments(mh, oracle, device):
    """decode_scaled: the [n, ceil(H / s), ceil(W / s)] view of the whole frame; Region.scaled_size;
    the launch shape; the wrappers' ValueErrors."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "noesc")
    fr, tabs = R.upload(device, _efs(frames))
    full = D.Region(*REGIONS["full"])
    for k in (0,) + KS:
        s = 1 << k
        got = D.decode_scaled(fr, tabs, k)
        torch.cuda.synchronize(device)
        assert tuple(got.shape) == (3, -(-R.H // s), -(-R.W // s)) == (3,) + full.scaled_size(R.W, R.H, k)[::-1]
        for f, want in enumerate(_wants(frames)):
            assert np.array_equal(got[f].cpu().numpy(), S.box_reduce_np(want, k)), (k, f)
            assert np.array_equal(got[f].cpu().numpy(), mh.box_reduce(want, k)), (k, f)
        G, waves = D.decode_region_scaled_shape(fr, full, k)
        assert waves == 8 and 1 <= G <= -(-9 * 2 // 8)
    for bad in (-1, 4, 1.5):
        with pytest.raises(ValueError):
            D.decode_region_scaled(fr, tabs, full, bad)
    with pytest.raises(ValueError):
        D.decode_region_scaled(fr, tabs, full, 1, extra_flags=mh.MH_FLAG_LANE_PAIRS)
    with pytest.raises(ValueError):
        D.decode_region_scaled(fr, D.DeviceTables(tabs.table1, tabs.table2, None), full, 1)
    with pytest.raises(ValueError):
        D.decode_region_scaled(fr, tabs, (70, 0, 8, 1), 1)


# ---- 5. write containment ------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", ["tight", "loose"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["w65", "bottom_edge", "last_block"])
def test_write_containment(mh, oracle, device, name, k, geom):
    """Three frames through the C ABI into a guarded buffer: bw * c bytes of every row Y < SH may be
    written and nothing else -- not the lead guard, the row padding, rows >= SH of a bottom-edge
    region (tight: the next frame's first rows), the gap between frames or the tail guard. loose:
    d_out, the pitch and the stride are multiples of c and of no more. Every byte is checked."""
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames))
    S.decode_scaled_contained(device, geom, fr, tabs, REGIONS[name], k, _wants(frames))


# ---- 6. the pipelined loop -----------------------------------------------------------------------------

def test_pipelined_loop_many_frames(mh, oracle, device):
    """test_gpu_region.py's multi-tile case at k = 2: 768 frames of the 1037 x 91 pair (two tables),
    region {1, 0, 129, 12}, S = 3 tiles per row -- every wave owns >= 3 tiles, so headers, span
    prefetch and the reducing decode of different tiles overlap, and the region's last segment and
    last block row are edge tiles."""
    from metalhuffman_amd import decoder as D
    kw = dict(grid_w=1040, grid_h=96, width=1037, height=91)
    a = R.frame_set(mh, oracle, "general", n=4, **kw)
    b = R.frame_set(mh, oracle, "noesc", n=3, **kw)
    distinct = [a[0], b[0], a[1], b[1], a[2], b[2], a[3]]
    n, k, region = 768, 2, (1, 0, 129, 12)
    frames = [distinct[i % 7] for i in range(n)]
    fr, ts = R.upload(device, _efs(frames), "set")
    G, waves = D.decode_region_scaled_shape(fr, D.Region(*region), k)
    assert waves == 8 and (region[3] * 3) // (G * waves) >= 3, (G, waves)
    got = S.decode_scaled_host(device, fr, ts, region, k)
    sw, sh, cols = S.scaled_size(region, k, 1037, 91)
    exp = np.stack([S.expected_scaled(f[1], region, k, 1037, 91) for f in distinct])
    assert got.shape == (n, sh, cols) and np.array_equal(got[:, :, :sw], exp[np.arange(n) % 7])
    assert (got[:, :, sw:] == 0).all()
