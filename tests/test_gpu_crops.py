"""mh_decode_crops: a list of crops of one size in pixels, each with its own frame and PIXEL origin,
in one launch; crop p is written from byte 0 of raster slot p. Every slot is prefilled with 0xA5;
expected pixels are always the numpy slice [y0: y0 + h, x0: x0 + w] of the oracle's
decode_frame_shader of the FULL frame (region_helpers.frame_set, which also checks it against the
image each frame was made from) -- never another GPU decode alone. Bit-exact.

The base frame is region_helpers': a 600 x 72 grid declared 597 x 67 (75 x 9 blocks, partial right
and bottom blocks), three distinct frames per flavour. A crop is (frame, x0, y0); its size (w, h) is
the launch's. round_up(w, 8) bytes of every row are written; columns >= w are not compared. The whole
slot of a rejected or skipped crop must keep the fill."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import region_helpers as R
from helpers import check_containment, containment_plan
from region_helpers import FILL, H, W

pytestmark = pytest.mark.gpu

MH_ERR_DIMS = -2


def _efs(frames):
    return [f[0] for f in frames]


def _wants(frames):
    return [f[1] for f in frames]


def _up8(v):
    return (v + 7) // 8 * 8


def decode_crops_host(device, fr, tabs, crops, size, **kw):
    """decode_crops into slots prefilled with FILL -> u8[n, h, round_up(w, 8)] on the host (and the
    per-crop status list when status=True is passed)."""
    import torch
    from metalhuffman_amd import decoder as D
    n = len(crops)
    out = torch.full((n, size[1], _up8(size[0])), FILL, dtype=torch.uint8, device=device)
    got = D.decode_crops(fr, tabs, crops, size, out=out, **kw)
    torch.cuda.synchronize(device)
    if kw.get("status") is True:
        assert got[0] is out
        return out.cpu().numpy(), got[1].cpu().tolist()
    assert got is out
    return out.cpu().numpy()


def expected(wants, crop, size):
    f, x0, y0 = (int(v) for v in crop[:3])
    assert 0 <= x0 and x0 + size[0] <= W and 0 <= y0 and y0 + size[1] <= H, (crop, size)
    return wants[f][y0: y0 + size[1], x0: x0 + size[0]]


def check_crops(got, crops, size, wants):
    """Slot p holds the numpy slice of its frame's expected raster in its first w columns."""
    w, h = size
    assert got.shape == (len(crops), h, _up8(w)), got.shape
    for p, c in enumerate(crops):
        exp = expected(wants, c, size)
        if not np.array_equal(got[p, :, :w], exp):
            ys, xs = np.nonzero(got[p, :, :w] != exp)
            raise AssertionError(f"crop {p} = {tuple(int(v) for v in c)} of {size}: {ys.size} wrong pixel(s), first "
                                 f"at row {int(ys[0])}, column {int(xs[0])}: {int(got[p, ys[0], xs[0]]):#04x}, "
                                 f"expected {int(exp[ys[0], xs[0]]):#04x}")


# ---- 1. every sub-block origin -------------------------------------------------------------------------

def _all_origins():
    """64 crops of 19 x 13, (x0 & 7, y0 & 7) every pair, over the three frames and over the frame: the
    block columns walk to the right edge (x0 + 19 <= 597) and the block rows to the bottom (y0 + 13 <= 67)."""
    crops = []
    for dy in range(8):
        for dx in range(8):
            i = 8 * dy + dx
            bx = (i * 7) % 72                      # at most 8 * 71 + 7 + 19 = 594 <= 597
            by = min((i * 5) % 7, (H - 13 - dy) // 8)
            crops.append((i % 3, 8 * bx + dx, 8 * by + dy))
    return crops


@pytest.mark.parametrize("tables", ["shared", "set"])
def test_all_sub_block_origins(mh, oracle, device, tables):
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames), tables)
    crops = _all_origins()
    assert {(c[1] & 7, c[2] & 7) for c in crops} == {(dx, dy) for dx in range(8) for dy in range(8)}
    assert {c[0] for c in crops} == {0, 1, 2} and max(c[2] for c in crops) == H - 13
    got, st = decode_crops_host(device, fr, tabs, crops, (19, 13), status=True)
    check_crops(got, crops, (19, 13), _wants(frames))
    assert st == [0] * 64


# ---- 2. sizes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", [1, 8, 9])
@pytest.mark.parametrize("w", [1, 7, 8, 9, 17])
def test_sizes(mh, oracle, device, w, h):
    """The frame's first pixel, its last crop (W - w, H - h), the other two corners, and origins at
    every kind of offset, over the three frames."""
    frames = R.frame_set(mh, oracle, "general")
    fr, ts = R.upload(device, _efs(frames), "set")
    crops = [(0, 0, 0), (1, W - w, H - h), (2, W - w, 0), (0, 0, H - h), (1, 8, 8), (2, 7, 7), (0, 301, 33),
             (1, 4, 58), (2, 252, 3), (0, 63, 1)]
    got = decode_crops_host(device, fr, ts, crops, (w, h))
    check_crops(got, crops, (w, h), _wants(frames))


# ---- 3. edges of the grid and of a tile ------------------------------------------------------------------

RECTS = {
    # (x0, y0, w, h)
    "right_edge": (85, 0, 512, 9),         # ends at column 597: the last block's right neighbour is block column 75
    "bottom_dy6": (85, 54, 512, 13),       # the bottom partial block row, dy = 6
    "no_row_9": (85, 56, 512, 11),         # CBH = 3, but block row 9 does not exist
    "row_unneeded": (85, 48, 512, 13),     # the third block row exists and is not needed
    "one_tile": (7, 5, 504, 10),           # 63 words, 64 live blocks, one tile
    "second_tile": (7, 5, 505, 10),        # a second tile with one word and one live block
    "two_tiles": (3, 2, 520, 21),
    "whole_frame": (0, 0, W, H),
}


@pytest.mark.parametrize("name", list(RECTS))
def test_edges_and_segments(mh, oracle, device, name):
    import torch
    from metalhuffman_amd import decoder as D
    x0, y0, w, h = RECTS[name]
    assert x0 + w <= W and y0 + h <= H
    if name in ("right_edge", "bottom_dy6", "no_row_9", "row_unneeded"):
        # the row's last block is the grid's last column: its right neighbour, block column 75, does not exist
        assert x0 + w == W and (x0 >> 3) + ((x0 & 7) + w + 7) // 8 == R.GBW
    if name == "bottom_dy6":
        assert y0 & 7 == 6 and y0 + h == H
    if name == "no_row_9":
        assert (h + 14) // 8 == 3 and (y0 >> 3) + 2 == R.GBH
    if name == "row_unneeded":
        assert (h + 14) // 8 == 3 and (y0 + h - 1) >> 3 == (y0 >> 3) + 1 and (y0 >> 3) + 2 < R.GBH
    if name == "one_tile":
        assert (w + 7) // 8 == 63 and ((x0 & 7) + w + 7) // 8 == 64
    if name == "second_tile":
        assert (w + 7) // 8 == 64 and ((x0 & 7) + w + 7) // 8 == 64
    frames = R.frame_set(mh, oracle, "general")
    fr, ts = R.upload(device, _efs(frames), "set")
    crops = [(f, x0, y0) for f in (2, 0, 1)]
    got = decode_crops_host(device, fr, ts, crops, (w, h))
    check_crops(got, crops, (w, h), _wants(frames))
    if name == "whole_frame":   # equals decode_frames' first 597 columns
        ref = torch.full((fr.n_frames, H, _up8(W)), FILL, dtype=torch.uint8, device=device)
        D.decode_frames(fr, ts, out=ref)
        torch.cuda.synchronize(device)
        ref = ref.cpu().numpy()
        for p, c in enumerate(crops):
            assert np.array_equal(got[p, :, :W], ref[c[0], :, :W]), p


# ---- 4. step flavours ------------------------------------------------------------------------------------

FLAVOUR_WIDE = ((300, 20), [(0, 3, 5), (1, 3, 47), (2, 3, 0), (1, 297, 30), (2, 3, 12)])
FLAVOUR_SMALL = ((13, 11), [(0, 0, 0), (1, 584, 56), (2, 251, 29), (0, 5, 50), (1, 123, 7), (2, 582, 1)])


@pytest.mark.parametrize("flavour", R.FLAVOURS)
def test_flavours(mh, oracle, device, flavour):
    """Under each step flavour (region_helpers.build_set asserts its precondition): crops of 300 x 20
    at x0 = 3 -- 38 blocks per row, so the words of lanes 31 and 32 are both live; under `oversize`
    38 blocks of 128 bytes exceed the stage window and the tile decodes in decode_halves' two
    passes, lane 31 taking its right half from the block lane 32 decodes beside it -- and small odd
    crops. flat8 is the byte loop, off_grid its slow loop."""
    frames = R.frame_set(mh, oracle, flavour)
    assert bool(frames[0][0].flags & 1) == (flavour == "no_delta")
    assert (frames[0][0].block_init is not None) == (flavour == "block_init")
    if flavour == "oversize":
        o = frames[0][0].block_offsets.astype(np.int64)
        assert (o[38] - o[0]) // 8 > R.STAGE_BYTES
    fr, tabs = R.upload(device, _efs(frames))
    assert fr.n_frames == 3 and fr.frame_code_offsets is not None
    for size, crops in (FLAVOUR_WIDE, FLAVOUR_SMALL):
        got = decode_crops_host(device, fr, tabs, crops, size)
        check_crops(got, crops, size, _wants(frames))


# ---- 5. equivalence with mh_decode_windows -----------------------------------------------------------------

def test_equals_decode_windows(mh, oracle, device):
    """dx = dy = 0, w = 8 bw, h = 8 bh: the bytes of decode_windows, all 8 bw columns."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames))
    bw, bh = 10, 3
    wins = [(0, 0, 0), (2, 64, 5), (1, 30, 2), (0, 64, 0), (1, 5, 5), (2, 0, 0)]
    crops = [(f, 8 * bx, 8 * by) for f, bx, by in wins]
    got = decode_crops_host(device, fr, tabs, crops, (8 * bw, 8 * bh))
    check_crops(got, crops, (8 * bw, 8 * bh), _wants(frames))
    ref = torch.full((len(wins), 8 * bh, 8 * bw), FILL, dtype=torch.uint8, device=device)
    D.decode_windows(fr, tabs, wins, (bw, bh), out=ref)
    torch.cuda.synchronize(device)
    assert np.array_equal(got, ref.cpu().numpy())


# ---- 6. crops the kernel rejects, and a skipped frame ------------------------------------------------------

@pytest.mark.parametrize("tables", ["shared", "set"])
def test_rejected_crops(mh, oracle, device, tables):
    """One launch of valid crops and one of each rejected kind -- a frame that does not exist, x0 = W - w
    + 1, y0 = H - h + 1, x0 = 0xFFFFFFFF (a sum that would wrap), a non-zero reserved word. The
    descriptors are a device tensor, so only the kernel sees them. Rejected slots keep the fill and
    report MH_ERR_DIMS; the valid ones -- the last origins that fit among them -- are right, status 0."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames), tables)
    w, h = 77, 21
    desc = [(0, 3, 5, 0), (3, 0, 0, 0), (0, W - w + 1, 0, 0), (0, 0, H - h + 1, 0), (0, 0xFFFFFFFF, 0, 0),
            (1, 5, 2, 1), (2, W - w, H - h, 0), (1, 0, 0xFFFFFFFF, 0), (1, W - w, 0, 0), (2, 0, H - h, 0)]
    valid = [0, 6, 8, 9]
    crops = torch.from_numpy(np.array(desc, np.uint32).view(np.int32)).to(device)
    n = len(desc)
    out = torch.full((n, h, _up8(w)), FILL, dtype=torch.uint8, device=device)
    status = torch.full((n,), 77, dtype=torch.int32, device=device)
    assert D.decode_crops(fr, tabs, crops, (w, h), out=out, status=status) is out
    torch.cuda.synchronize(device)
    got, st = out.cpu().numpy(), status.cpu().tolist()
    assert st == [0 if p in valid else MH_ERR_DIMS for p in range(n)], st
    for p in range(n):
        if p not in valid:
            assert (got[p] == FILL).all(), f"rejected crop {p} = {desc[p]}: its slot was written"
    check_crops(got[valid], [desc[p][:3] for p in valid], (w, h), _wants(frames))
    # without a status array the same launch leaves the same picture
    out2 = torch.full_like(out, FILL)
    D.decode_crops(fr, tabs, crops, (w, h), out=out2)
    torch.cuda.synchronize(device)
    assert np.array_equal(out2.cpu().numpy()[:, :, :w], got[:, :, :w])


def test_skipped_frame(mh, oracle, device):
    """A table set whose middle header is rejected (a 17-bit length: MH_ERR_CODE_TOO_LONG): crops of
    that frame are untouched and carry the frame's status word, the others are right."""
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    efs = _efs(frames)
    fr = D.DeviceFrames.pack(efs, device, shared_table=False)
    too_long = np.zeros(256, np.uint8)
    too_long[7] = 17
    ts = D.DeviceTableSet.from_canonical_headers(np.stack([efs[0].canon, too_long, efs[2].canon]), device)
    assert ts.status.cpu().tolist() == [0, -3, 0]
    size = (77, 21)
    crops = [(1, 0, 0), (0, 163, 27), (1, 520, 46), (2, 520, 46), (1, 243, 19), (0, 1, 1)]
    ok = [p for p, c in enumerate(crops) if c[0] != 1]
    got, st = decode_crops_host(device, fr, ts, crops, size, status=True)
    assert st == [-3 if c[0] == 1 else 0 for c in crops], st
    for p, c in enumerate(crops):
        if c[0] == 1:
            assert (got[p] == FILL).all(), p
    check_crops(got[ok], [crops[p] for p in ok], size, _wants(frames))


# ---- 7. the forms of `crops` -------------------------------------------------------------------------------

def test_device_crops_tensor(mh, oracle, device):
    """`crops` as an int32 device tensor, [n, 4] (used as it is) and [n, 3], and as a host list: the
    same picture."""
    import torch
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames))
    size = (77, 21)
    crops = [(0, 0, 0), (2, 520, 0), (1, 243, 46), (0, 517, 41), (2, 1, 1), (0, 0, 0), (1, 515, 27)]
    ref = decode_crops_host(device, fr, tabs, crops, size)
    check_crops(ref, crops, size, _wants(frames))
    c4 = torch.tensor([list(c) + [0] for c in crops], dtype=torch.int32, device=device)
    assert c4.shape == (len(crops), 4) and c4.is_contiguous() and c4.data_ptr() % 16 == 0
    w = size[0]
    assert np.array_equal(decode_crops_host(device, fr, tabs, c4, size)[:, :, :w], ref[:, :, :w])
    c3 = torch.tensor([list(c) for c in crops], dtype=torch.int32, device=device)
    assert np.array_equal(decode_crops_host(device, fr, tabs, c3, size)[:, :, :w], ref[:, :, :w])
    assert np.array_equal(decode_crops_host(device, fr, tabs, np.asarray(crops), size)[:, :, :w], ref[:, :, :w])


# ---- 8. the launch shape and the pipelined loop ---------------------------------------------------------------

def _tiles(size):
    ow = (size[0] + 7) // 8
    return ((size[1] + 14) // 8) * ((ow + 62) // 63)


@pytest.mark.parametrize("size,tiles", [((19, 13), 3), ((W, H), 20), ((505, 10), 6), ((504, 10), 3), ((520, 60), 18)])
def test_shape_rule(mh, oracle, device, size, tiles):
    """G = clamp(ceil(R / n_crops), 1, ceil(CBH S / 8)), CBH = (h + 14) / 8, S = ceil(ceil(w / 8) / 63),
    R = CUs x the kernel's occupancy -- 1, 2 or 3 workgroups per CU: 53,280 B of LDS admit no more."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    fr, _ = R.upload(device, _efs(frames))
    assert _tiles(size) == tiles
    most = -(-tiles // 8)
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    occs = set()
    for n in (1, 2, 100, cus, 2 * cus, 3 * cus, 3 * cus + 1, 65536):
        G, waves = D.decode_crops_shape(fr, n, size)
        assert waves == 8
        fit = [o for o in (1, 2, 3) if G == min(max(-(-cus * o // n), 1), most)]
        assert fit, (n, G, cus, most)
        occs.add(tuple(fit))
    assert D.decode_crops_shape(fr, 1, size)[0] == most and D.decode_crops_shape(fr, 65536, size)[0] == 1
    assert set.intersection(*(set(f) for f in occs)), occs    # one occupancy explains every answer


def test_pipelined_loop_many_crops(mh, oracle, device):
    """So many crops of 520 x 60 -- S = 2, CBH = 9, 18 tiles -- that a crop gets ONE workgroup: every
    wave then owns >= 2 tiles, so header, span prefetch and decode of different tiles overlap in
    batch_loop's steady state, and consecutive tiles of a wave change block row (the first row's
    descriptor differs from the others') and segment. y0 & 7 = 0 needs 8 of the 9 block rows: the
    last two tiles are skipped. Origins from a seeded generator."""
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    fr, ts = R.upload(device, _efs(frames), "set")
    size = (520, 60)
    tiles = _tiles(size)
    n = 768
    G, waves = D.decode_crops_shape(fr, n, size)
    while G > 1 and n < 8192:          # (a device with more resident workgroups)
        n *= 2
        G, waves = D.decode_crops_shape(fr, n, size)
    assert G == 1 and waves == 8 and tiles // (G * waves) >= 2, (n, G, waves, tiles)
    rng = np.random.default_rng(2026)
    crops = np.stack([rng.integers(0, 3, n), rng.integers(0, W - size[0] + 1, n),
                      rng.integers(0, H - size[1] + 1, n)], axis=1)
    assert {int(v) for v in crops[:, 2]} == set(range(8)) and len({int(v) & 7 for v in crops[:, 1]}) == 8
    got = decode_crops_host(device, fr, ts, crops, size)
    check_crops(got, crops.tolist(), size, _wants(frames))


# ---- 9. write containment ----------------------------------------------------------------------------------

CONTAINED = {
    # w % 8 != 0, dx != 0 and dy != 0 in every crop, slot 0 and the last slot included
    "small": ((19, 13), [(0, 5, 1), (1, 251, 54), (2, 578, 3), (1, 13, 9), (2, 1, 47), (0, 339, 30)]),
    "two_tiles": ((509, 21), [(0, 3, 2), (1, 87, 46), (2, 85, 41), (0, 1, 7)]),
    "bottom": ((77, 11), [(0, 517, 54), (1, 3, 49), (2, 519, 55)]),
}


@pytest.mark.parametrize("geom", ["tight", "loose"])
@pytest.mark.parametrize("case", list(CONTAINED))
@pytest.mark.parametrize("flavour", ["general", "flat8"])
def test_write_containment(mh, oracle, device, flavour, case, geom):
    """One mh_decode_crops launch through the C-ABI into slots laid out inside a pattern-filled buffer
    (helpers.containment_plan with W = w, H = h, one "frame" per crop): round_up(w, 8) bytes of every
    row of every slot may be written and nothing else -- not the lead guard (the rows of the first
    block row above the crop, dy of them, would land there), the row padding, the gap between slots
    (the rows of the last block row below the crop) or the tail guard. EVERY byte of the buffer is
    checked. Pitch, slot stride and lead are region_helpers.geometry's tight and loose ones."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    (w, h), crops = CONTAINED[case]
    assert w % 8 and all(c[1] & 7 and c[2] & 7 for c in crops)
    frames = R.frame_set(mh, oracle, flavour)
    fr, tabs = R.upload(device, _efs(frames))
    n = len(crops)
    pitch, stride, lead = R.geometry(geom, w, h)
    plan = containment_plan(n, w, h, pitch, stride, lead, 8 * pitch + 4096, written_cols=_up8(w))
    buf = torch.from_numpy(plan.pattern.copy()).to(device)
    d_out = buf.data_ptr() + plan.d_out
    assert d_out % 256 == 0 if geom == "tight" else (d_out % 16 == 8 and stride - h * pitch == 40)
    desc = torch.tensor([list(c) + [0] for c in crops], dtype=torch.int32, device=device)
    status = torch.full((n,), 77, dtype=torch.int32, device=device)
    st, _ = D._frames_entry(fr)
    N.check(N.lib().mh_decode_crops(ctypes.byref(st), desc.data_ptr(), n, w, h, tabs.lut.data_ptr(), 0, None,
                                    status.data_ptr(), d_out, pitch, stride,
                                    torch.cuda.current_stream(device).cuda_stream), "mh_decode_crops")
    torch.cuda.synchronize(device)
    assert status.cpu().tolist() == [0] * n
    check_containment(buf.cpu().numpy(), plan, [expected(_wants(frames), c, (w, h)) for c in crops])
