"""mh_decode_region: a block-aligned region of every frame in one launch, into a raster of the
region's own size. Every raster is prefilled with 0xA5; expected pixels are the region's rectangle
of the oracle's decode_frame_shader of the FULL frame (which region_helpers.frame_set also checks
against the image each frame was made from) -- never another GPU decode alone. Bit-exact.

The base frame is a 600 x 72 grid declared 597 x 67 (75 x 9 blocks, partial right and bottom
blocks); region_helpers.REGIONS names its ten regions. A tile of the region kernel is a run of
<= 64 blocks inside one block row of the region: S = ceil(bw / 64) tiles per row."""
from __future__ import annotations

import numpy as np
import pytest

import region_helpers as R
from region_helpers import REGIONS

pytestmark = pytest.mark.gpu

ALL = list(REGIONS)


def _efs(frames):
    return [f[0] for f in frames]


def _wants(frames):
    return [f[1] for f in frames]


# ---- 1. the base frame's regions ----------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_base_frame_regions(mh, oracle, device, name):
    """One frame (NULL frame_code_offsets), the general flavour, one shared table."""
    frames = R.frame_set(mh, oracle, "general")[:1]
    fr, tabs = R.upload(device, _efs(frames))
    assert fr.frame_code_offsets is None
    got = R.decode_region_host(device, fr, tabs, REGIONS[name])
    R.check_region(got, REGIONS[name], _wants(frames))
    x0, y0, rw, rh = R.region_pixels(REGIONS[name])
    assert {"right_edge": rw == 509, "bottom_edge": rh == 35}.get(name, True)


def test_full_region_is_decode_frames(mh, oracle, device):
    """The region {0, 0, block_width, block_height} is byte-identical to mh_decode_frames, the
    pitch padding of the right-edge blocks included (both rasters prefilled alike)."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    fr, ts = R.upload(device, _efs(frames), "set")
    got = R.decode_region_host(device, fr, ts, REGIONS["full"])
    ref = torch.full((fr.n_frames, R.H, 8 * R.GBW), R.FILL, dtype=torch.uint8, device=device)
    D.decode_frames(fr, ts, out=ref)
    torch.cuda.synchronize(device)
    assert got.shape == tuple(ref.shape) and np.array_equal(got, ref.cpu().numpy())
    R.check_region(got, REGIONS["full"], _wants(frames))


# ---- 2. step flavours -----------------------------------------------------------------------------

FLAVOURS = ["general", "general14", "noesc", "flat4", "flat8", "off_grid", "no_delta", "block_init"]


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_flavours(mh, oracle, device, flavour):
    """Every region of the base frame under each step flavour (their preconditions on the canonical
    lengths are asserted by region_helpers.build_set): general -> batch_loop<Lut13>; general14 ->
    <Lut13> (14-bit codes escape); noesc -> <Lut13NoEsc>; flat4 -> <Lut13Flat>; flat8 -> flat8_loop's
    byte loop; off_grid -> its slow loop (decode_halves<Batch8>); no_delta; block_init. Three frames
    of one table per launch (frame_code_offsets), the table shared (stride 0)."""
    frames = R.frame_set(mh, oracle, flavour)
    mn, mx, nsym = R.lens(frames[0][0])
    assert {"general": mx == 16, "no_delta": mx == 16, "general14": mx == 14, "block_init": 13 <= mx <= 14,
            "noesc": mx == 13 and mn < mx, "flat4": mn == mx == 4,
            "flat8": (mn, mx, nsym) == (8, 8, 256), "off_grid": (mn, mx, nsym) == (8, 8, 256)}[flavour]
    assert bool(frames[0][0].flags & 1) == (flavour == "no_delta")
    assert (frames[0][0].block_init is not None) == (flavour == "block_init")
    fr, tabs = R.upload(device, _efs(frames))
    assert fr.n_frames == 3 and fr.frame_code_offsets is not None
    for name in ALL:
        got = R.decode_region_host(device, fr, tabs, REGIONS[name])
        R.check_region(got, REGIONS[name], _wants(frames))


# ---- 3. oversize runs: decode_halves ---------------------------------------------------------------

@pytest.mark.parametrize("bw", [35, 48, 64, 65])
def test_oversize_runs(mh, oracle, device, bw):
    """The {16: 256} header: every block is 128 bytes, so a run of >= 35 blocks exceeds the
    4,352-byte stage window and decodes as two halves: second halves of 3, 16 and 32 lanes, and (65)
    a one-lane second tile beside an oversize first one."""
    frames = R.frame_set(mh, oracle, "oversize")
    region = (3, 2, bw, 5)
    for ef, _ in frames:
        o = ef.block_offsets.astype(np.int64)
        for r in range(region[3]):
            b0 = (region[1] + r) * R.GBW + region[0]
            assert (o[b0 + min(bw, 64)] - o[b0]) // 8 > R.STAGE_BYTES        # the run's span: oversize
            assert (o[b0 + 32] - o[b0]) // 8 + 40 <= R.STAGE_BYTES           # a half fits the window
    fr, tabs = R.upload(device, _efs(frames))
    got = R.decode_region_host(device, fr, tabs, region)
    R.check_region(got, region, _wants(frames))


# ---- 4. batches ------------------------------------------------------------------------------------

def _three_tables(mh, oracle):
    frames = [R.frame_set(mh, oracle, fl)[i] for i, fl in enumerate(("general", "noesc", "flat4"))]
    assert len({f[0].canon.tobytes() for f in frames}) == 3
    return frames


@pytest.mark.parametrize("name", ["w65", "right_edge", "bottom_edge", "last_block"])
def test_batch_three_tables(mh, oracle, device, name):
    """Three frames with three distinct tables (a DeviceTableSet): three flavours in one launch."""
    frames = _three_tables(mh, oracle)
    fr, ts = R.upload(device, _efs(frames), "set")
    assert ts.status.cpu().tolist() == [0, 0, 0]
    R.check_region(R.decode_region_host(device, fr, ts, REGIONS[name]), REGIONS[name], _wants(frames))


@pytest.mark.parametrize("name", ["w65", "right_edge", "bottom_edge", "last_block"])
def test_batch_shared_table(mh, oracle, device, name):
    """Three frames of one header decoded with ONE prepared table (lut_stride_bytes == 0), and the
    same three through a table per frame: the same bytes."""
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames))
    got = R.decode_region_host(device, fr, tabs, REGIONS[name])
    R.check_region(got, REGIONS[name], _wants(frames))
    fr2, ts = R.upload(device, _efs(frames), "set")
    assert np.array_equal(R.decode_region_host(device, fr2, ts, REGIONS[name]), got)


def test_batch_skips_rejected_frame(mh, oracle, device):
    """A non-zero status word on the middle frame: its region raster keeps the fill; without the
    status array (skip_rejected=False) it decodes."""
    frames = _three_tables(mh, oracle)
    fr, ts = R.upload(device, _efs(frames), "set")
    ts.status[1] = -3
    region = REGIONS["w70"]
    got = R.decode_region_host(device, fr, ts, region)
    assert (got[1] == R.FILL).all()
    R.check_region(got[[0, 2]], region, [frames[0][1], frames[2][1]])
    R.check_region(R.decode_region_host(device, fr, ts, region, skip_rejected=False), region, _wants(frames))


def test_one_frame_behind_offset_array(mh, oracle, device):
    """One frame WITH a two-entry frame_code_offsets array that places it 48 bytes into the buffer."""
    import torch
    frames = R.frame_set(mh, oracle, "general14")[1:2]
    fr, tabs = R.upload(device, _efs(frames))
    lead = 48
    fr.codes = torch.cat([torch.full((lead,), 0xFF, dtype=torch.uint8, device=device), fr.codes])
    fr.frame_code_offsets = torch.tensor([lead, fr.codes.numel()], dtype=torch.int64, device=device)
    for name in ("w65", "last_block", "full"):
        R.check_region(R.decode_region_host(device, fr, tabs, REGIONS[name]), REGIONS[name], _wants(frames))


def test_decode_rect_view(mh, oracle, device):
    """decode_rect: the [n, h, w] pixel view of the covering region."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "noesc")
    fr, tabs = R.upload(device, _efs(frames))
    for (x0, y0, w, h) in ((29, 13, 300, 41), (590, 60, 7, 7), (0, 0, 597, 67), (8, 8, 8, 8)):
        got = D.decode_rect(fr, tabs, x0, y0, w, h)
        torch.cuda.synchronize(device)
        assert tuple(got.shape) == (3, h, w)
        for f, want in enumerate(_wants(frames)):
            assert np.array_equal(got[f].cpu().numpy(), want[y0: y0 + h, x0: x0 + w]), (x0, y0, w, h, f)
    with pytest.raises(ValueError):
        D.decode_region(fr, D.DeviceTables(tabs.table1, tabs.table2, None), D.Region(0, 0, 1, 1))


@pytest.mark.parametrize("flavour", ["general", "no_delta"])
@pytest.mark.parametrize("n", [1, 3])
def test_scale_zero_is_the_unscaled_entry(mh, oracle, device, n, flavour):
    """The six frame-slice entries are rows of one kernel table, and scale 0 of a region or of windows
    is the unscaled kernel: the same launch shape and the same bytes from either entry. Every shape
    entry at every scale reports 8 waves and 1 <= G <= ceil(tiles / 8), tiles counted as the decode
    entries count them: ceil(NB / 64) of a frame, bh * ceil(bw / 64) of a region or a window."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, flavour)[:n]
    assert bool(frames[0][0].flags & mh.MH_FLAG_NO_DELTA) == (flavour == "no_delta")
    fr, tabs = R.upload(device, _efs(frames))
    assert fr.n_frames == n and (fr.frame_code_offsets is None) == (n == 1)

    def ok(shape, tiles):
        G, waves = shape
        assert waves == 8 and 1 <= G <= -(-tiles // 8), (shape, tiles)

    ok(D.decode_frames_shape(fr), -(-R.NB // 64))
    ok(D.decode_headers_shape(fr), -(-R.NB // 64))
    n_windows = 2
    for name in ("full", "w65"):
        rg = D.Region(*REGIONS[name])
        size = (rg.bw, rg.bh)
        tiles = rg.bh * -(-rg.bw // 64)
        assert D.decode_region_shape(fr, rg) == D.decode_region_scaled_shape(fr, rg, 0)
        assert D.decode_windows_shape(fr, n_windows, size) == D.decode_windows_scaled_shape(fr, n_windows, size, 0)
        ok(D.decode_region_shape(fr, rg), tiles)
        ok(D.decode_windows_shape(fr, n_windows, size), tiles)
        for k in range(4):
            ok(D.decode_region_scaled_shape(fr, rg, k), tiles)
            ok(D.decode_windows_scaled_shape(fr, n_windows, size, k), tiles)

    region = REGIONS["w65"]
    got = R.decode_region_host(device, fr, tabs, region)
    R.check_region(got, region, _wants(frames))
    out0 = torch.full(got.shape, R.FILL, dtype=torch.uint8, device=device)
    D.decode_region_scaled(fr, tabs, D.Region(*region), 0, out=out0)
    windows = [(0, 3, 2), (n - 1, 10, 4)]
    size = (region[2], region[3])
    w_plain = D.decode_windows(fr, tabs, windows, size)
    w_zero = D.decode_windows_scaled(fr, tabs, windows, size, 0)
    torch.cuda.synchronize(device)
    assert np.array_equal(out0.cpu().numpy(), got)
    assert tuple(w_plain.shape) == (2, 8 * size[1], 8 * size[0])
    assert np.array_equal(w_zero.cpu().numpy(), w_plain.cpu().numpy())
    assert np.array_equal(w_plain[0].cpu().numpy(), got[0])  # window 0 is w65 of frame 0, no edge block in it


# ---- 5. the pipelined loop -------------------------------------------------------------------------

def test_pipelined_loop_many_frames(mh, oracle, device):
    """768 frames of a 1040 x 96 grid (130 x 12 blocks, declared 1037 x 91) cycled from 7 distinct
    ones of two tables, region {1, 0, 129, 12}: S = 3 tiles per row, 36 per frame. With that many
    frames a frame gets few workgroups, so every wave owns >= 3 tiles (asserted from
    decode_region_shape): header, span prefetch and decode of different tiles overlap in
    batch_loop's steady state, and consecutive tiles of a wave change row and segment."""
    import torch
    from metalhuffman_amd import decoder as D
    kw = dict(grid_w=1040, grid_h=96, width=1037, height=91)
    a = R.frame_set(mh, oracle, "general", n=4, **kw)
    b = R.frame_set(mh, oracle, "noesc", n=3, **kw)
    distinct = [a[0], b[0], a[1], b[1], a[2], b[2], a[3]]
    assert len({f[0].canon.tobytes() for f in distinct}) == 2
    n = 768
    frames = [distinct[i % 7] for i in range(n)]
    region = (1, 0, 129, 12)
    S = -(-region[2] // 64)
    tiles = region[3] * S
    fr, ts = R.upload(device, _efs(frames), "set")
    G, waves = D.decode_region_shape(fr, D.Region(*region))
    assert S >= 2 and waves == 8 and tiles // (G * waves) >= 3, (S, G, waves, tiles)
    got = R.decode_region_host(device, fr, ts, region)
    _, _, rw, rh = R.region_pixels(region, 1037, 91)
    exp = np.stack([R.crop(f[1], region, 1037, 91) for f in distinct])
    assert np.array_equal(got[:, :, :rw], exp[np.arange(n) % 7])


# ---- 6. write containment --------------------------------------------------------------------------

CONTAINED = [("general", "right_edge"), ("general", "bottom_edge"), ("general", "w65"), ("oversize", (3, 2, 48, 5)),
             ("flat8", "bottom_edge"), ("off_grid", "right_edge")]


@pytest.mark.parametrize("geom", ["tight", "loose"])
@pytest.mark.parametrize("case", CONTAINED, ids=[f"{c[0]}-{c[1] if isinstance(c[1], str) else 'w48'}"
                                                 for c in CONTAINED])
def test_write_containment(mh, oracle, device, case, geom):
    """Three frames into a guarded buffer with W = RW, H = RH (helpers.containment_plan /
    check_containment, test_gpu_write_containment.py's tight and loose geometries): 8 bw bytes of
    every row y < RH may be written and nothing else -- not the lead guard, the row padding, rows
    >= RH of a bottom-edge region (tight: they would land in the next frame's first rows), the gap
    between frames or the tail guard. Every byte of the buffer is checked."""
    flavour, reg = case
    region = REGIONS[reg] if isinstance(reg, str) else reg
    frames = R.frame_set(mh, oracle, flavour)
    fr, tabs = R.upload(device, _efs(frames))
    R.decode_region_contained(device, geom, fr, tabs, region, _wants(frames))


@pytest.mark.parametrize("geom", ["tight", "loose"])
def test_write_containment_table_set(mh, oracle, device, geom):
    """The same check with a table per frame (three flavours in one launch, a non-zero table stride)."""
    frames = _three_tables(mh, oracle)
    fr, ts = R.upload(device, _efs(frames), "set")
    R.decode_region_contained(device, geom, fr, ts, REGIONS["w65"], _wants(frames))
