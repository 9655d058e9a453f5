"""mh_decode_windows: a list of windows of one size, each with its own frame and origin, in one
launch; window p is written to raster slot p. Every raster is prefilled with 0xA5; expected pixels
are the window's rectangle of the oracle's decode_frame_shader of the FULL frame
(region_helpers.frame_set, which also checks it against the image each frame was made from) --
never another GPU decode alone. Bit-exact.

The base frame is region_helpers': a 600 x 72 grid declared 597 x 67 (75 x 9 blocks, partial right
and bottom blocks), three distinct frames per flavour. A window is (frame, bx0, by0); its size
(bw, bh) is the launch's. Rows >= RH_p of a slot (a window at the frame's bottom edge) and the whole
slot of a rejected or skipped window must keep the fill."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import region_helpers as R
from helpers import check_containment, containment_plan
from region_helpers import FILL, REGIONS

pytestmark = pytest.mark.gpu

MH_ERR_DIMS = -2


def _efs(frames):
    return [f[0] for f in frames]


def _wants(frames):
    return [f[1] for f in frames]


def _region(win, size):
    return (win[1], win[2], size[0], size[1])


def decode_windows_host(device, fr, tabs, windows, size, **kw):
    """decode_windows into slots prefilled with FILL -> u8[n, 8 bh, 8 bw] on the host (and the
    per-window status list when status=True is passed)."""
    import torch
    from metalhuffman_amd import decoder as D
    n = len(windows)
    out = torch.full((n, 8 * size[1], 8 * size[0]), FILL, dtype=torch.uint8, device=device)
    got = D.decode_windows(fr, tabs, windows, size, out=out, **kw)
    torch.cuda.synchronize(device)
    if kw.get("status") is True:
        assert got[0] is out
        return out.cpu().numpy(), got[1].cpu().tolist()
    assert got is out
    return out.cpu().numpy()


def check_windows(got, windows, size, wants, width=R.W, height=R.H):
    """Slot p holds window p's rectangle of its frame's expected raster in rows < RH_p, columns
    < RW_p (columns RW_p .. 8 bw - 1 of those rows are written with unspecified bytes), and the fill
    in every row >= RH_p."""
    assert got.shape == (len(windows), 8 * size[1], 8 * size[0]), got.shape
    for p, win in enumerate(windows):
        region = _region(win, size)
        _, _, rw, rh = R.region_pixels(region, width, height)
        exp = R.crop(wants[win[0]], region, width, height)
        if not np.array_equal(got[p, :rh, :rw], exp):
            ys, xs = np.nonzero(got[p, :rh, :rw] != exp)
            raise AssertionError(f"window {p} = {tuple(win)} of {size}: {ys.size} wrong pixel(s), first at row "
                                 f"{int(ys[0])}, column {int(xs[0])}: {int(got[p, ys[0], xs[0]]):#04x}, expected "
                                 f"{int(exp[ys[0], xs[0]]):#04x}")
        assert (got[p, rh:] == FILL).all(), f"window {p} = {tuple(win)}: rows >= RH = {rh} of its slot were written"


# ---- 1. placement ------------------------------------------------------------------------------------

PLACED_SIZE = (10, 3)
PLACED = [(0, 0, 0), (2, 65, 0), (1, 30, 6), (0, 65, 6), (2, 0, 0), (0, 0, 0), (1, 64, 3)]


@pytest.mark.parametrize("tables", ["shared", "set"])
def test_placement(mh, oracle, device, tables):
    """The frame's first block, the right edge (RW = 77), the bottom edge (RH = 19), the corner,
    frames out of order and a duplicate, with one shared table (stride 0) and a table per frame."""
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames), tables)
    px = [R.region_pixels(_region(w, PLACED_SIZE)) for w in PLACED]
    assert px[1][2:] == (77, 24) and px[2][2:] == (80, 19) and px[3][2:] == (77, 19) and PLACED[5] == PLACED[0]
    got, st = decode_windows_host(device, fr, tabs, PLACED, PLACED_SIZE, status=True)
    check_windows(got, PLACED, PLACED_SIZE, _wants(frames))
    assert st == [0] * len(PLACED)
    assert np.array_equal(got[5], got[0])


def test_device_windows_tensor(mh, oracle, device):
    """The placement case with `windows` an int32 device tensor, [n, 4] (used as it is) and [n, 3]:
    the same bytes as the host-list call."""
    import torch
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames))
    ref = decode_windows_host(device, fr, tabs, PLACED, PLACED_SIZE)
    check_windows(ref, PLACED, PLACED_SIZE, _wants(frames))
    w4 = torch.tensor([list(w) + [0] for w in PLACED], dtype=torch.int32, device=device)
    assert w4.shape == (len(PLACED), 4) and w4.is_contiguous() and w4.data_ptr() % 16 == 0
    assert np.array_equal(decode_windows_host(device, fr, tabs, w4, PLACED_SIZE), ref)
    w3 = torch.tensor([list(w) for w in PLACED], dtype=torch.int32, device=device)
    assert np.array_equal(decode_windows_host(device, fr, tabs, w3, PLACED_SIZE), ref)


# ---- 2. sizes ----------------------------------------------------------------------------------------

SIZES = {
    (1, 1): [(0, 0, 0), (1, 74, 8), (2, 37, 4), (0, 74, 0), (1, 0, 8), (2, 74, 8)],   # the frame's last block
    (64, 9): [(0, 0, 0), (1, 11, 0), (2, 5, 0), (1, 0, 0), (0, 11, 0)],
    (65, 5): [(0, 0, 0), (1, 10, 4), (2, 3, 2), (0, 10, 0), (1, 0, 4)],               # S = 2: 1 live lane
    (70, 7): [(0, 0, 0), (1, 5, 2), (2, 2, 1), (0, 5, 0), (2, 0, 2)],                 # S = 2: 6 live lanes
    (75, 9): [(0, 0, 0), (1, 0, 0), (2, 0, 0), (1, 0, 0), (0, 0, 0)],                 # the whole frame
}


@pytest.mark.parametrize("size", list(SIZES), ids=[f"{s[0]}x{s[1]}" for s in SIZES])
def test_sizes(mh, oracle, device, size):
    import torch
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    fr, ts = R.upload(device, _efs(frames), "set")
    wins = SIZES[size]
    assert len(wins) >= 5 and {w[0] for w in wins} == {0, 1, 2}
    assert all(w[1] + size[0] <= R.GBW and w[2] + size[1] <= R.GBH for w in wins)
    assert -(-size[0] // 64) == (2 if size[0] > 64 else 1)
    got = decode_windows_host(device, fr, ts, wins, size)
    check_windows(got, wins, size, _wants(frames))
    if size == (75, 9):   # byte-identical to decode_frames' raster of that frame, the padding columns included
        ref = torch.full((fr.n_frames, R.H, 8 * R.GBW), FILL, dtype=torch.uint8, device=device)
        D.decode_frames(fr, ts, out=ref)
        torch.cuda.synchronize(device)
        ref = ref.cpu().numpy()
        for p, w in enumerate(wins):
            assert np.array_equal(got[p, :R.H], ref[w[0]]), p


# ---- 3. equivalence with mh_decode_region --------------------------------------------------------------

@pytest.mark.parametrize("name", ["w65", "right_edge", "bottom_edge", "last_block"])
def test_equals_decode_region(mh, oracle, device, name):
    """The same rectangle of every frame as three windows: byte-identical to decode_region's output
    over the written bytes (8 bw bytes of every row < RH), padding columns included."""
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames))
    region = REGIONS[name]
    size = region[2:]
    wins = [(f, region[0], region[1]) for f in range(3)]
    got = decode_windows_host(device, fr, tabs, wins, size)
    check_windows(got, wins, size, _wants(frames))
    ref = R.decode_region_host(device, fr, tabs, region)
    rh = ref.shape[1]
    assert ref.shape == (3, rh, 8 * size[0]) and np.array_equal(got[:, :rh], ref)


# ---- 4. step flavours ----------------------------------------------------------------------------------

FLAVOUR_SIZE = (35, 4)
FLAVOUR_WINDOWS = [(0, 0, 0), (1, 40, 5), (2, 20, 2), (0, 40, 0), (1, 0, 5), (2, 13, 3)]


@pytest.mark.parametrize("flavour", R.FLAVOURS)
def test_flavours(mh, oracle, device, flavour):
    """Six windows over the three frames under each step flavour (region_helpers.build_set asserts
    each flavour's precondition on the canonical lengths): general, general14, noesc, flat4, the
    flat8 byte loop, off_grid (its slow loop), no_delta, block_init, and oversize, where a run of 35
    blocks of 128 bytes exceeds the stage window and decodes as two halves."""
    frames = R.frame_set(mh, oracle, flavour)
    assert bool(frames[0][0].flags & 1) == (flavour == "no_delta")
    assert (frames[0][0].block_init is not None) == (flavour == "block_init")
    if flavour == "oversize":
        o = frames[0][0].block_offsets.astype(np.int64)
        assert (o[FLAVOUR_SIZE[0]] - o[0]) // 8 > R.STAGE_BYTES
    fr, tabs = R.upload(device, _efs(frames))
    assert fr.n_frames == 3 and fr.frame_code_offsets is not None
    got = decode_windows_host(device, fr, tabs, FLAVOUR_WINDOWS, FLAVOUR_SIZE)
    check_windows(got, FLAVOUR_WINDOWS, FLAVOUR_SIZE, _wants(frames))


# ---- 5. the pipelined loop -----------------------------------------------------------------------------

def test_pipelined_loop_many_windows(mh, oracle, device):
    """So many windows of (65, 9) -- S = 2, 18 tiles -- that a window gets ONE workgroup
    (decode_windows_shape reports G = 1: n_windows >= CUs x occupancy): every wave then owns >= 2
    tiles, so header, span prefetch and decode of different tiles overlap in batch_loop's steady
    state, and consecutive tiles of a wave change row and segment. Positions from a seeded generator."""
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    fr, ts = R.upload(device, _efs(frames), "set")
    size = (65, 9)
    tiles = size[1] * 2
    n = 768
    G, waves = D.decode_windows_shape(fr, n, size)
    while G > 1 and n < 8192:          # (a device with more resident workgroups)
        n *= 2
        G, waves = D.decode_windows_shape(fr, n, size)
    assert G == 1 and waves == 8 and tiles // (G * waves) >= 2, (n, G, waves, tiles)
    g1, _ = D.decode_windows_shape(fr, 1, size)
    assert g1 == -(-tiles // 8)        # one window: as many workgroups as its tiles fill
    rng = np.random.default_rng(2026)
    wins = np.stack([rng.integers(0, 3, n), rng.integers(0, R.GBW - size[0] + 1, n), np.zeros(n, np.int64)], axis=1)
    assert len({tuple(w) for w in wins.tolist()}) == 3 * (R.GBW - size[0] + 1)   # every position of every frame
    got = decode_windows_host(device, fr, ts, wins, size)
    check_windows(got, wins.tolist(), size, _wants(frames))


# ---- 6. windows the kernel rejects -----------------------------------------------------------------------

@pytest.mark.parametrize("tables", ["shared", "set"])
def test_rejected_windows(mh, oracle, device, tables):
    """One launch of two valid windows and one of each rejected kind -- a frame that does not exist,
    bx0 + bw and by0 + bh past the grid, bx0 = 0xFFFFFFFF (a sum that would wrap), a non-zero
    reserved word. The descriptors are a device tensor, so only the kernel sees them: it decides
    from the descriptor alone, before any load through it, so no address is formed from a rejected
    value. Rejected slots keep the fill and report MH_ERR_DIMS; the valid ones are right, status 0;
    the launch completes."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames), tables)
    size = (10, 3)
    desc = [(0, 0, 0, 0), (3, 0, 0, 0), (0, 66, 0, 0), (0, 0, 7, 0), (0, 0xFFFFFFFF, 0, 0), (1, 5, 2, 1),
            (2, 65, 6, 0)]
    valid = [0, 6]
    wins = torch.from_numpy(np.array(desc, np.uint32).view(np.int32)).to(device)
    n = len(desc)
    out = torch.full((n, 8 * size[1], 8 * size[0]), FILL, dtype=torch.uint8, device=device)
    status = torch.full((n,), 77, dtype=torch.int32, device=device)
    assert D.decode_windows(fr, tabs, wins, size, out=out, status=status) is out
    torch.cuda.synchronize(device)
    got, st = out.cpu().numpy(), status.cpu().tolist()
    assert st == [0 if p in valid else MH_ERR_DIMS for p in range(n)], st
    for p in range(n):
        if p not in valid:
            assert (got[p] == FILL).all(), f"rejected window {p} = {desc[p]}: its slot was written"
    check_windows(got[valid], [desc[p][:3] for p in valid], size, _wants(frames))
    # without a status array the same launch leaves the same bytes
    out2 = torch.full_like(out, FILL)
    D.decode_windows(fr, tabs, wins, size, out=out2)
    torch.cuda.synchronize(device)
    assert np.array_equal(out2.cpu().numpy(), got)


# ---- 7. a frame skipped by its status word -----------------------------------------------------------------

def test_skipped_frame(mh, oracle, device):
    """A table set whose middle header is rejected (a 17-bit length: MH_ERR_CODE_TOO_LONG): windows of
    that frame are untouched and carry the frame's status word, the others are right. With
    skip_rejected=False the status array is not passed: the frame decodes with its all-zero table
    (every window of the stream the zero-width entry: pixels 0, tests/test_gpu_multitable.py), status 0."""
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    efs = _efs(frames)
    fr = D.DeviceFrames.pack(efs, device, shared_table=False)
    too_long = np.zeros(256, np.uint8)
    too_long[7] = 17
    ts = D.DeviceTableSet.from_canonical_headers(np.stack([efs[0].canon, too_long, efs[2].canon]), device)
    assert ts.status.cpu().tolist() == [0, -3, 0]
    size = (10, 3)
    wins = [(1, 0, 0), (0, 20, 3), (1, 65, 6), (2, 65, 6), (1, 30, 2), (0, 0, 0)]
    ok = [p for p, w in enumerate(wins) if w[0] != 1]
    got, st = decode_windows_host(device, fr, ts, wins, size, status=True)
    assert st == [-3 if w[0] == 1 else 0 for w in wins], st
    for p, w in enumerate(wins):
        if w[0] == 1:
            assert (got[p] == FILL).all(), p
    check_windows(got[ok], [wins[p] for p in ok], size, _wants(frames))
    got, st = decode_windows_host(device, fr, ts, wins, size, status=True, skip_rejected=False)
    assert st == [0] * len(wins), st
    check_windows(got[ok], [wins[p] for p in ok], size, _wants(frames))
    for p, w in enumerate(wins):
        if w[0] == 1:
            _, _, rw, rh = R.region_pixels(_region(w, size))
            assert not got[p, :rh].any() and (got[p, rh:] == FILL).all(), p


# ---- 8. write containment ----------------------------------------------------------------------------------

CONTAINED = {
    # six interior windows, all RW = 80, RH = 24
    "interior": ((10, 3), [(0, 5, 1), (1, 30, 3), (2, 64, 5), (1, 5, 1), (2, 0, 0), (0, 40, 4)], (80, 24)),
    # three bottom-right windows, one per frame, all RW = 77, RH = 19: rows 19 .. 23 of every slot stay
    "corner": ((10, 3), [(0, 65, 6), (1, 65, 6), (2, 65, 6)], (77, 19)),
}


@pytest.mark.parametrize("geom", ["tight", "loose"])
@pytest.mark.parametrize("case", list(CONTAINED))
@pytest.mark.parametrize("flavour", ["general", "flat8"])
def test_write_containment(mh, oracle, device, flavour, case, geom):
    """One mh_decode_windows launch through the C-ABI into slots laid out inside a pattern-filled
    buffer (helpers.containment_plan with W = RW, H = RH, one "frame" per window): 8 bw bytes of every
    row y < RH of every slot may be written and nothing else -- not the lead guard, the row padding,
    the rows >= RH of a slot, the gap between slots or the tail guard. EVERY byte of the buffer is
    checked. Pitch, slot stride and lead are region_helpers.geometry's tight and loose ones for a
    slot of its full 8 bh rows (the stride the host check demands), so in the tight geometry the rows
    >= RH of a bottom-edge window are all that separates it from the next slot."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    size, wins, (rw, rh) = CONTAINED[case]
    frames = R.frame_set(mh, oracle, flavour)
    fr, tabs = R.upload(device, _efs(frames))
    for w in wins:
        assert R.region_pixels(_region(w, size))[2:] == (rw, rh)
    n, rows = len(wins), 8 * size[1]
    pitch, stride, lead = R.geometry(geom, rw, rows)
    assert pitch >= 8 * size[0] and stride >= rows * pitch
    plan = containment_plan(n, rw, rh, pitch, stride, lead, 8 * pitch + 4096, written_cols=8 * size[0])
    buf = torch.from_numpy(plan.pattern.copy()).to(device)
    d_out = buf.data_ptr() + plan.d_out
    assert d_out % 256 == 0 if geom == "tight" else (d_out % 16 == 8 and stride - rows * pitch == 40)
    desc = torch.tensor([list(w) + [0] for w in wins], dtype=torch.int32, device=device)
    status = torch.full((n,), 77, dtype=torch.int32, device=device)
    st, _ = D._frames_entry(fr)
    N.check(N.lib().mh_decode_windows(ctypes.byref(st), desc.data_ptr(), n, size[0], size[1], tabs.lut.data_ptr(), 0,
                                      None, status.data_ptr(), d_out, pitch, stride,
                                      torch.cuda.current_stream(device).cuda_stream), "mh_decode_windows")
    torch.cuda.synchronize(device)
    assert status.cpu().tolist() == [0] * n
    check_containment(buf.cpu().numpy(), plan, [R.crop(frames[w[0]][1], _region(w, size)) for w in wins])
