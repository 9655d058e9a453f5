"""mh_decode_windows_scaled: a list of windows of one size, each with its own frame and origin, at
1/2, 1/4 or 1/8 scale in one launch; window p is written to raster slot p. Every raster is prefilled
with 0xA5; expected pixels are scaled_helpers.box_reduce_np (the numpy statement of the box filter)
of the window's crop of the oracle's decode_frame_shader of the FULL frame (region_helpers.frame_set)
-- never another GPU decode alone. Bit-exact.

The frame is region_helpers' 597 x 67 one (75 x 9 blocks, the last block column 5 pixels wide, the
last block row 3 rows high): a lone column, a lone row, a corner cell and cells wholly outside the
frame all occur. The windows, sizes and descriptor lists are those of test_gpu_windows.py. Rows
>= SH_p of a slot and the whole slot of a rejected or skipped window must keep the fill; columns
SW_p .. bw c - 1 of the written rows are 0."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import region_helpers as R
import scaled_helpers as S
import test_gpu_windows as TW
import windows_scaled_helpers as WS
from helpers import check_containment, containment_plan
from region_helpers import FILL, REGIONS

pytestmark = pytest.mark.gpu

KS = (1, 2, 3)
MH_ERR_DIMS = -2


def _efs(frames):
    return [f[0] for f in frames]


def _wants(frames):
    return [f[1] for f in frames]


# ---- 1. placement ------------------------------------------------------------------------------------

@pytest.mark.parametrize("tables", ["shared", "set"])
@pytest.mark.parametrize("k", KS)
def test_placement(mh, oracle, device, k, tables):
    """The frame's first block, the right edge (RW = 77), the bottom edge (RH = 19), the corner,
    frames out of order and a duplicate, with one shared table (stride 0) and a table per frame."""
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames), tables)
    wins, size = TW.PLACED, TW.PLACED_SIZE
    assert size == (10, 3)
    px = [R.region_pixels(WS.window_region(w, size)) for w in wins]
    assert px[1][2:] == (77, 24) and px[2][2:] == (80, 19) and px[3][2:] == (77, 19) and wins[5] == wins[0]
    got, st = WS.decode_windows_scaled_host(device, fr, tabs, wins, size, k, status=True)
    WS.check_windows_scaled(got, wins, size, k, _wants(frames))
    assert st == [0] * len(wins)
    assert np.array_equal(got[5], got[0])


# ---- 2. sizes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(1, 1), (64, 9), (65, 5), (75, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("k", KS)
def test_sizes(mh, oracle, device, k, size):
    """One block (the frame's last, (74, 8), included: its cells lie partly or wholly outside the
    frame), one full tile per row, S = 2 with one live lane in the second tile, and the whole frame,
    which is byte-identical to decode_region_scaled of the full grid."""
    frames = R.frame_set(mh, oracle, "general")
    fr, ts = R.upload(device, _efs(frames), "set")
    wins = TW.SIZES[size]
    assert {w[0] for w in wins} == {0, 1, 2}
    assert all(w[1] + size[0] <= R.GBW and w[2] + size[1] <= R.GBH for w in wins)
    if size == (1, 1):
        assert (1, 74, 8) in wins or (2, 74, 8) in wins
    got = WS.decode_windows_scaled_host(device, fr, ts, wins, size, k)
    WS.check_windows_scaled(got, wins, size, k, _wants(frames))
    if size == (75, 9):
        ref = S.decode_scaled_host(device, fr, ts, REGIONS["full"], k)
        sh = ref.shape[1]
        assert ref.shape[2] == got.shape[2] and sh == -(-R.H // (1 << k))
        for p, w in enumerate(wins):
            assert np.array_equal(got[p, :sh], ref[w[0]]), p


# ---- 3. equivalence with mh_decode_region_scaled -----------------------------------------------------

@pytest.mark.parametrize("name", ["w65", "right_edge", "bottom_edge", "last_block"])
@pytest.mark.parametrize("k", KS)
def test_equals_decode_region_scaled(mh, oracle, device, k, name):
    """The same rectangle of every frame as three windows: byte-identical to decode_region_scaled's
    output over all bw c written columns of every row < SH."""
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames))
    region = REGIONS[name]
    size = region[2:]
    wins = [(f, region[0], region[1]) for f in range(3)]
    got = WS.decode_windows_scaled_host(device, fr, tabs, wins, size, k)
    WS.check_windows_scaled(got, wins, size, k, _wants(frames))
    ref = S.decode_scaled_host(device, fr, tabs, region, k)
    sh = ref.shape[1]
    assert ref.shape == (3, sh, size[0] * (8 >> k)) and np.array_equal(got[:, :sh], ref)


# ---- 4. step flavours ----------------------------------------------------------------------------------

_ONE_K = {"general14": 1, "noesc": 2, "flat4": 3, "off_grid": 1, "block_init": 2, "oversize": 3}
FLAVOUR_CASES = [(fl, k) for fl in R.FLAVOURS for k in (KS if fl not in _ONE_K else (_ONE_K[fl],))]


def test_flavour_cases_cover():
    assert {fl for fl, _ in FLAVOUR_CASES} == set(R.FLAVOURS)
    for fl in ("general", "flat8", "no_delta"):
        assert {k for f, k in FLAVOUR_CASES if f == fl} == set(KS)
    assert {k for f, k in FLAVOUR_CASES if f in _ONE_K} == set(KS)


@pytest.mark.parametrize("flavour,k", FLAVOUR_CASES)
def test_flavours(mh, oracle, device, flavour, k):
    """The windows test's six windows of (35, 4) under each step flavour: both loops, both slow paths
    (off_grid, oversize), no_delta and block_init all end in the reducing stage."""
    frames = R.frame_set(mh, oracle, flavour)
    assert bool(frames[0][0].flags & 1) == (flavour == "no_delta")
    fr, tabs = R.upload(device, _efs(frames))
    assert fr.n_frames == 3
    got = WS.decode_windows_scaled_host(device, fr, tabs, TW.FLAVOUR_WINDOWS, TW.FLAVOUR_SIZE, k)
    WS.check_windows_scaled(got, TW.FLAVOUR_WINDOWS, TW.FLAVOUR_SIZE, k, _wants(frames))


# ---- 5. the pipelined loop -----------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3])
def test_pipelined_loop_many_windows(mh, oracle, device, k):
    """So many windows of (65, 9) -- S = 2, 18 tiles -- that a window gets ONE workgroup
    (decode_windows_scaled_shape reports G = 1): every wave then owns >= 2 tiles, so header, span
    prefetch and the reducing decode of different tiles overlap. Positions from a seeded generator."""
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    fr, ts = R.upload(device, _efs(frames), "set")
    size = (65, 9)
    tiles = size[1] * 2
    n = 768
    G, waves = D.decode_windows_scaled_shape(fr, n, size, k)
    while G > 1 and n < 8192:          # (a device with more resident workgroups)
        n *= 2
        G, waves = D.decode_windows_scaled_shape(fr, n, size, k)
    assert G == 1 and waves == 8 and tiles // (G * waves) >= 2, (n, G, waves, tiles)
    g1, _ = D.decode_windows_scaled_shape(fr, 1, size, k)
    assert g1 == -(-tiles // 8)
    rng = np.random.default_rng(2026 + k)
    wins = np.stack([rng.integers(0, 3, n), rng.integers(0, R.GBW - size[0] + 1, n), np.zeros(n, np.int64)], axis=1)
    got = WS.decode_windows_scaled_host(device, fr, ts, wins, size, k)
    # (one expectation per distinct position; every slot is compared)
    distinct = sorted({tuple(w) for w in wins.tolist()})
    assert len(distinct) == 3 * (R.GBW - size[0] + 1)
    exp = {}
    for w in distinct:
        region = WS.window_region(w, size)
        sw, sh, cols = S.scaled_size(region, k, R.W, R.H)
        e = np.zeros((sh, cols), np.uint8)
        e[:, :sw] = S.expected_scaled(frames[w[0]][1], region, k, R.W, R.H)
        exp[w] = e
    sh = -(-R.H // (1 << k))
    for p, w in enumerate(wins.tolist()):
        assert np.array_equal(got[p, :sh], exp[tuple(w)]), (p, w)
    assert (got[:, sh:] == FILL).all()


# ---- 6. rejected windows and a skipped frame --------------------------------------------------------------

@pytest.mark.parametrize("tables", ["shared", "set"])
def test_rejected_windows(mh, oracle, device, tables):
    """The windows test's descriptor list at k = 2: a frame that does not exist, bx0 + bw and by0 + bh
    past the grid, bx0 = 0xFFFFFFFF, a non-zero reserved word. Rejected slots keep the fill and report
    MH_ERR_DIMS; the valid ones are right, status 0; without a status array the same bytes."""
    import torch
    from metalhuffman_amd import decoder as D
    k, c = 2, 2
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames), tables)
    size = (10, 3)
    desc = [(0, 0, 0, 0), (3, 0, 0, 0), (0, 66, 0, 0), (0, 0, 7, 0), (0, 0xFFFFFFFF, 0, 0), (1, 5, 2, 1),
            (2, 65, 6, 0)]
    valid = [0, 6]
    wins = torch.from_numpy(np.array(desc, np.uint32).view(np.int32)).to(device)
    n = len(desc)
    out = torch.full((n, c * size[1], c * size[0]), FILL, dtype=torch.uint8, device=device)
    status = torch.full((n,), 77, dtype=torch.int32, device=device)
    assert D.decode_windows_scaled(fr, tabs, wins, size, k, out=out, status=status) is out
    torch.cuda.synchronize(device)
    got, st = out.cpu().numpy(), status.cpu().tolist()
    assert st == [0 if p in valid else MH_ERR_DIMS for p in range(n)], st
    for p in range(n):
        if p not in valid:
            assert (got[p] == FILL).all(), f"rejected window {p} = {desc[p]}: its slot was written"
    WS.check_windows_scaled(got[valid], [desc[p][:3] for p in valid], size, k, _wants(frames))
    out2 = torch.full_like(out, FILL)
    D.decode_windows_scaled(fr, tabs, wins, size, k, out=out2)
    torch.cuda.synchronize(device)
    assert np.array_equal(out2.cpu().numpy(), got)


def test_skipped_frame(mh, oracle, device):
    """The windows test's table set (the middle header rejected, MH_ERR_CODE_TOO_LONG) at k = 2:
    windows of that frame keep the fill and carry the frame's status word, the others are right;
    without a status array the same bytes."""
    from metalhuffman_amd import decoder as D
    k = 2
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
    got, st = WS.decode_windows_scaled_host(device, fr, ts, wins, size, k, status=True)
    assert st == [-3 if w[0] == 1 else 0 for w in wins], st
    for p, w in enumerate(wins):
        if w[0] == 1:
            assert (got[p] == FILL).all(), p
    WS.check_windows_scaled(got[ok], [wins[p] for p in ok], size, k, _wants(frames))
    assert np.array_equal(WS.decode_windows_scaled_host(device, fr, ts, wins, size, k), got)


# ---- 7. write containment ----------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", ["tight", "loose"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", list(TW.CONTAINED))
@pytest.mark.parametrize("flavour", ["general", "flat8"])
def test_write_containment(mh, oracle, device, flavour, case, k, geom):
    """One mh_decode_windows_scaled launch through the C ABI into slots laid out inside a
    pattern-filled buffer (helpers.containment_plan with W = SW, H = SH, one "frame" per window):
    bw c bytes of every row Y < SH of every slot may be written and nothing else -- not the lead
    guard, the row padding, the rows >= SH of a slot, the gap between slots or the tail guard. EVERY
    byte of the buffer is checked. Pitch, slot stride and lead are scaled_helpers.scaled_geometry's
    for a slot of its full bh c rows: loose, d_out, the pitch and the stride are multiples of c and
    not of 2 c."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    size, wins, (rw, rh) = TW.CONTAINED[case]
    c, s = 8 >> k, 1 << k
    frames = R.frame_set(mh, oracle, flavour)
    fr, tabs = R.upload(device, _efs(frames))
    for w in wins:
        assert R.region_pixels(WS.window_region(w, size))[2:] == (rw, rh)
    sw, sh = -(-rw // s), -(-rh // s)
    n, rows, cols = len(wins), c * size[1], c * size[0]
    pitch, stride, lead = S.scaled_geometry(geom, cols, rows, c)
    assert pitch >= cols and stride >= rows * pitch
    plan = containment_plan(n, sw, sh, pitch, stride, lead, 8 * pitch + 4096, written_cols=cols)
    buf = torch.from_numpy(plan.pattern.copy()).to(device)
    d_out = buf.data_ptr() + plan.d_out
    assert d_out % 256 == 0 if geom == "tight" else (d_out % (2 * c) == c and pitch % (2 * c) == c
                                                     and stride % (2 * c) == c)
    desc = torch.tensor([list(w) + [0] for w in wins], dtype=torch.int32, device=device)
    status = torch.full((n,), 77, dtype=torch.int32, device=device)
    st, _ = D._frames_entry(fr)
    N.check(N.lib().mh_decode_windows_scaled(ctypes.byref(st), desc.data_ptr(), n, size[0], size[1], k,
                                             tabs.lut.data_ptr(), 0, None, status.data_ptr(), d_out, pitch, stride,
                                             torch.cuda.current_stream(device).cuda_stream),
            "mh_decode_windows_scaled")
    torch.cuda.synchronize(device)
    assert status.cpu().tolist() == [0] * n
    after = buf.cpu().numpy()
    check_containment(after, plan, [S.expected_scaled(frames[w[0]][1], WS.window_region(w, size), k, R.W, R.H)
                                    for w in wins])
    assert (plan.frame_view(after, cols)[:, :, sw:] == 0).all(), "written columns >= SW are not 0"


# ---- 8. scale 1 ------------------------------------------------------------------------------------------

def test_scale_one_is_decode_windows(mh, oracle, device):
    """log2_scale = 0 forwards to mh_decode_windows: the same bytes, statuses and launch shape."""
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames))
    got, st = WS.decode_windows_scaled_host(device, fr, tabs, TW.PLACED, TW.PLACED_SIZE, 0, status=True)
    ref, st_ref = TW.decode_windows_host(device, fr, tabs, TW.PLACED, TW.PLACED_SIZE, status=True)
    assert got.shape == ref.shape and np.array_equal(got, ref) and st == st_ref == [0] * len(TW.PLACED)
    TW.check_windows(got, TW.PLACED, TW.PLACED_SIZE, _wants(frames))
    assert (D.decode_windows_scaled_shape(fr, 7, TW.PLACED_SIZE, 0) == D.decode_windows_shape(fr, 7, TW.PLACED_SIZE))
