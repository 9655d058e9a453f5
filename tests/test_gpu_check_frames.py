"""mh_check_frames / mh_check_headers on the GPU against the oracle, frame by frame: the report equals
oracle.check_frame's under the frame's own table for every frame of ANY input, the verdict is MH_OK exactly
for a clean report, and the verdict array fed to the decode entries as d_frame_status keeps every rejected
frame's raster untouched. Every call goes through the C ABI into report, verdict and header-status buffers
that were 0xA5 before it and lie between guard words (check_frames_helpers)."""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import pytest

import check_frames_helpers as CH
import defect_helpers as DH
import scaled_helpers as S
import slice_helpers as SH

pytestmark = pytest.mark.gpu

CLEAN = CH.CLEAN
STREAM = CH.MH_ERR_STREAM


def _table_set(device, dfs):
    from metalhuffman_amd import decoder as D
    return D.DeviceTableSet.from_canonical_headers(CH.canons_of(dfs), device)


def _single_table(device, df):
    from metalhuffman_amd import decoder as D
    t1, t2 = df.ef.tables()
    return D.DeviceTables.upload(t1, t2, device)


# ---- the sweep ----------------------------------------------------------------------------------------

def test_frames_sweep_and_isolation(mh, oracle, device):
    """The 40 "frames" cases under a table set, then again with the frames in reversed order: no frame's
    report depends on its neighbours or its place."""
    cases = CH.cases(mh, oracle, "frames")
    assert len(cases) == 40
    for case in cases:
        _, _, W, H = case.grid
        for dfs in (list(case.frames), list(case.frames)[::-1]):
            fr = DH.pack(device, dfs, W, H)
            CH.assert_checked(CH.check_frames(device, fr, _table_set(device, dfs)), dfs, case.describe())


def test_headers_sweep(mh, oracle, device):
    cases = CH.cases(mh, oracle, "headers")
    assert len(cases) == 40
    for case in cases:
        _, _, W, H = case.grid
        dfs = list(case.frames)
        rep, ver, hdr = CH.check_headers(device, DH.pack(device, dfs, W, H), CH.canons_of(dfs))
        CH.assert_checked((rep, ver), dfs, case.describe())
        assert hdr.tolist() == [0] * len(dfs)


def test_check_cases_through_both_entries_equal_mh_check(mh, oracle, device):
    """The 30 check cases with a whole T2 (swapped offsets, offsets past the slot): stride 0 with the one
    prepared table, the header replicated per frame, and mh_check's own report."""
    cases = CH.cases(mh, oracle, DH.CHECK)
    assert len(cases) == 30
    for case in cases:
        up, tabs, dfs = DH.upload(device, case)          # tabs: T1/T2 for mh_check
        fr = up.frames
        want = DH.gpu_check(device, fr, tabs)
        DH.assert_reports(want, dfs, case.describe())
        shared = CH.check_frames(device, fr, _single_table(device, dfs[0]), status=None)
        CH.assert_checked(shared, dfs, case.describe())
        assert np.array_equal(shared[0], want)
        rep, ver, hdr = CH.check_headers(device, fr, up.canons)
        CH.assert_checked((rep, ver), dfs, case.describe())
        assert np.array_equal(rep, want) and not hdr.any()
        assert not rep[:, 1].any()


# ---- tile and workgroup edges ---------------------------------------------------------------------------

GRIDS = {1: (1, 1), 63: (63, 1), 64: (8, 8), 65: (65, 1), 72: (9, 8)}


@pytest.mark.parametrize("nb", sorted(GRIDS))
def test_one_defect_at_tile_and_frame_edges(mh, oracle, device, nb):
    """One stalled block at a time -- block 0, 63, 64, the frame's last and the next frame's first -- in
    batches of 2 to 5 frames: the report names that frame and that block, the others are clean; the dead
    lanes of a last tile add nothing."""
    gbw, gbh = GRIDS[nb]
    assert gbw * gbh == nb
    spots = sorted({b for b in (0, 63, 64, nb - 1) if b < nb})
    for j, b in enumerate(spots):
        n = 2 + (j + nb) % 4
        for f, blk in ((n // 2, b), (n // 2 + 1 if n // 2 + 1 < n else 0, 0)):
            dfs = CH.single_frames(oracle, gbw, gbh, n, {f: [blk]})
            want = [64, 0, int(blk < nb - 1), blk]
            assert [df.report.tolist() for df in dfs] == [want if i == f else CLEAN for i in range(n)]
            fr = DH.pack(device, dfs, 8 * gbw, 8 * gbh)
            CH.assert_checked(CH.check_frames(device, fr, _table_set(device, dfs)), dfs, (nb, n, f, blk))
            rep, ver, _ = CH.check_headers(device, fr, CH.canons_of(dfs))
            CH.assert_checked((rep, ver), dfs, (nb, n, f, blk, "headers"))


@pytest.mark.parametrize("pair", [(3, 600), (511, 512), (70, 639)])
def test_two_defects_served_by_different_workgroups(mh, oracle, device, pair):
    """640 blocks are 10 tiles: with more than one workgroup per frame, tiles 0..7 and 8..9 belong to
    different ones. The counts add and [3] is the smaller block."""
    lo, hi = pair
    dfs = CH.single_frames(oracle, 40, 16, 2, {1: [lo, hi]})
    assert dfs[1].report.tolist() == [128, 0, 1 + int(hi < 639), lo] and dfs[0].report.tolist() == CLEAN
    fr = DH.pack(device, dfs, 320, 128)
    for headers in (False, True):
        g, w = CH.shape(mh, fr, headers)
        assert (g, w) == (2, 8), "two frames of 10 tiles: two workgroups of 8 waves per frame"
        assert lo // 64 < 8 * (g - 1) <= hi // 64
    CH.assert_checked(CH.check_frames(device, fr, _table_set(device, dfs)), dfs, pair)
    rep, ver, _ = CH.check_headers(device, fr, CH.canons_of(dfs))
    CH.assert_checked((rep, ver), dfs, pair)


# ---- the slot's end ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("rest", [1, 2, 3])
def test_a_slot_of_any_length_reads_zero_behind_it(mh, oracle, device, rest):
    """One frame without an offset array whose codes_bytes is 1, 2, 3 mod 4, with 0xFF bytes behind it in the
    allocation. Under the single-symbol code a one bit stalls. Block 30 starts at byte 240 and holds one
    set bit, in byte 241: a slot of 241 bytes ends in front of it (the block sees zeros, all codes, where
    the memory holds 0xFF), one of 242 or 243 bytes holds it (the block stalls at its 10th step, 55
    zero-width steps) -- the slot's last, partial dword is read byte by byte, neither dropped nor read whole."""
    def one_bit(slot, offs, payload):
        slot[: payload] = 0
        slot[241] = 0x40
    full = DH.made_frame(oracle, "single", 16, 2, 3, one_bit)
    assert full.ef.codes.size == 272 and int(full.ef.block_offsets[30]) == 8 * 240
    assert full.report.tolist() == [55, 0, 1, 30]
    for cut in (240 + rest, 244 + rest, 236 + rest, 4 + rest):
        df = CH.cut_slot(oracle, full, cut)
        assert cut % 4 == rest
        if cut == 240 + rest:
            assert df.report.tolist() == ([0, 0, 1, 31] if rest == 1 else [55, 0, 2, 30])
        fr = CH.pack_one(device, df)
        assert fr.frame_code_offsets is None and fr.codes.numel() == cut
        CH.assert_checked(CH.check_frames(device, fr, _single_table(device, df), status=None), [df], cut)
        rep, ver, _ = CH.check_headers(device, fr, CH.canons_of([df]))
        CH.assert_checked((rep, ver), [df], (cut, "headers"))


def test_a_short_slot_reads_zero_not_its_neighbour(mh, oracle, device):
    """test_gpu_check_sweep's case for mh_check: a slot cut in front of its last two blocks is followed at
    once by its neighbour's first byte, in both orders."""
    def ones(slot, offs, payload):
        slot[payload - 8: payload] = 0xFF
    full = DH.made_frame(oracle, "single", 16, 2, 3, ones)
    assert full.report.tolist() == [64, 0, 0, 31]
    cut = dataclasses.replace(full, ef=dataclasses.replace(full.ef, codes=full.ef.codes[:240].copy()),
                              tail=full.ef.codes[240:].copy())
    DH._reference(oracle, cut, 128, 16, False, 0)
    assert cut.report.tolist() == [0, 0, 1, 31]
    def leading_ones(slot, offs, payload):
        slot[:8] = 0xFF
    loud = DH.made_frame(oracle, "single", 16, 2, 4, leading_ones)               # a neighbour that starts with ones
    assert loud.report.tolist() == [64, 0, 1, 0]
    for dfs in ([cut, full], [full, cut], [cut, loud], [loud, cut, loud], [cut]):
        fr = DH.pack(device, dfs, 128, 16)
        CH.assert_checked(CH.check_frames(device, fr, _table_set(device, dfs)), dfs, [d.ef.codes.size for d in dfs])
        rep, ver, _ = CH.check_headers(device, fr, CH.canons_of(dfs))
        CH.assert_checked((rep, ver), dfs, "headers")


# ---- offsets ----------------------------------------------------------------------------------------------

def test_offsets_past_the_slot_and_at_the_32_bit_edge(mh, oracle, device):
    """0xFFFFFFFF and just past 8 x slot under the single-symbol code: the zero bits there are codes, the
    walk goes on past the slot -- and past bit 2^32 -- without a stall."""
    dfs = CH.far_offset_frames(oracle)
    fr = DH.pack(device, dfs, 72, 16)
    CH.assert_checked(CH.check_frames(device, fr, _table_set(device, dfs)), dfs, "far offsets")
    rep, ver, _ = CH.check_headers(device, fr, CH.canons_of(dfs))
    CH.assert_checked((rep, ver), dfs, "far offsets, headers")
    for df in dfs:
        one = DH.pack(device, [df], 72, 16)
        CH.assert_checked(CH.check_frames(device, one, _single_table(device, df), status=None), [df], "one frame")


# ---- skips ------------------------------------------------------------------------------------------------

def test_a_nonzero_status_word_passes_through(mh, oracle, device):
    import torch
    dfs = CH.single_frames(oracle, 9, 8, 4, {0: [5], 1: [7], 3: [71]})
    fr = DH.pack(device, dfs, 72, 64)
    status = torch.tensor([0, -4, 77, 0], dtype=torch.int32, device=device)
    want_rep = np.stack([df.report if s == 0 else np.array(CLEAN, np.uint32) for df, s in zip(dfs, status.tolist())])
    want_ver = [STREAM, -4, 77, STREAM]
    for verdict in (True, False):
        rep, ver = CH.check_frames(device, fr, _table_set(device, dfs), status=status, verdict=verdict)
        assert np.array_equal(rep, want_rep)
        assert ver is None or ver.tolist() == want_ver
        rep, ver, hdr = CH.check_headers(device, fr, CH.canons_of(dfs), status=status, verdict=verdict)
        assert np.array_equal(rep, want_rep)
        assert ver is None or ver.tolist() == want_ver
        assert hdr[[0, 3]].tolist() == [0, 0] and (hdr[[1, 2]] == CH.DIRTY).all(), "a skipped frame's header is not judged"
    assert status.tolist() == [0, -4, 77, 0]


@pytest.mark.parametrize("name,code", [("too_long", -3), ("kraft", -5)])
def test_a_rejected_header_among_good_ones(mh, oracle, device, name, code):
    dfs = CH.single_frames(oracle, 9, 8, 3, {0: [5], 1: [3], 2: [70]})
    fr = DH.pack(device, dfs, 72, 64)
    canons = CH.canons_of(dfs)
    canons[1] = CH.bad_header(canons[1], name)
    want_rep = np.stack([dfs[0].report, np.array(CLEAN, np.uint32), dfs[2].report])
    for verdict, header_status in ((True, True), (False, True), (True, False), (False, False)):
        rep, ver, hdr = CH.check_headers(device, fr, canons, verdict=verdict, header_status=header_status)
        assert np.array_equal(rep, want_rep)
        assert ver is None or ver.tolist() == [STREAM, code, STREAM]
        assert hdr is None or hdr.tolist() == [0, code, 0]


# ---- the chain: check -> decode on one stream -------------------------------------------------------------

def _chain(device, case, entry):
    """mh_check_* then mh_decode_* with the verdict as d_frame_status, no sync between, into a guarded
    raster: a rejected frame's slot keeps every byte, an accepted frame is byte-exact."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    up, tabs, dfs = DH.upload(device, case)
    fr, n = up.frames, len(dfs)
    _, _, W, H = case.grid
    cols = (W + 7) // 8 * 8
    pitch, stride, lead = S.scaled_geometry("tight", cols, H, 8)
    want = CH.want_verdict(dfs)
    pics = [(df.want if v == 0 else np.zeros((0, 0), np.uint8), False) for df, v in zip(dfs, want)]
    g = CH.guarded(device, n)
    st, _ = D._frames_entry(fr)
    stream = torch.cuda.current_stream(device).cuda_stream
    hdr = torch.from_numpy(up.canons.copy()).to(device)
    L = N.lib()

    def launch(d_out):
        if entry == "frames":
            N.check(L.mh_check_frames(ctypes.byref(st), tabs.luts.data_ptr(), tabs.stride, tabs.status.data_ptr(),
                                      g.ptr("report"), g.ptr("verdict"), stream), "mh_check_frames")
            N.check(L.mh_decode_frames(ctypes.byref(st), tabs.luts.data_ptr(), tabs.stride, g.ptr("verdict"), d_out,
                                       pitch, stride, stream), "mh_decode_frames")
        else:
            N.check(L.mh_check_headers(ctypes.byref(st), hdr.data_ptr(), None, None, g.ptr("report"), g.ptr("verdict"),
                                       stream), "mh_check_headers")
            N.check(L.mh_decode_headers(ctypes.byref(st), hdr.data_ptr(), g.ptr("verdict"), g.ptr("header"), d_out,
                                        pitch, stride, stream), "mh_decode_headers")
        return None
    SH.run_slots(device, cols, H, pics, (pitch, stride, lead, 8 * pitch + 4096), launch,
                 label=lambda p: f"{case.describe()}, frame {p}")
    rep, ver, hs = g.read()
    CH.assert_checked((rep, ver), dfs, case.describe())
    if entry == "headers":      # the decode judged the headers of the frames it did not skip
        assert [int(h) for h, v in zip(hs, want) if v == 0] == [0] * want.count(0)
        assert all(h == CH.DIRTY for h, v in zip(hs, want) if v != 0)
    return want


@pytest.mark.parametrize("entry", ["frames", "headers"])
def test_check_then_decode_on_one_stream(mh, oracle, device, entry):
    seen = []
    for case in CH.cases(mh, oracle, entry)[:10]:
        seen += _chain(device, case, entry)
    assert seen.count(0) >= 5 and seen.count(STREAM) >= 5


def test_encoded_batch_check(mh, device, bigbridge):
    """A freshly encoded batch: every verdict MH_OK, every report clean, on the encoder's stream; the
    verdict goes into decode_headers' frame_status as it is."""
    import torch
    from metalhuffman_amd import decoder as D, encoder as E
    n, H, W = 5, 43, 150
    imgs = np.stack([np.ascontiguousarray(bigbridge[20 * i: 20 * i + H, 30 * i: 30 * i + W]) for i in range(n)])
    batch = E.BatchEncoder(W, H, n, device).encode_async(torch.from_numpy(imgs).to(device))
    rep, ver = batch.check()
    out = D.decode_headers(batch.frames(check=False), batch.canon, frame_status=ver)
    assert rep.dtype is torch.int64 and ver.dtype is torch.int32
    assert rep.cpu().tolist() == [CLEAN] * n and ver.cpu().tolist() == [0] * n
    assert np.array_equal(out[:, :, :W].cpu().numpy(), imgs)
    rep2, ver2, hs = D.check_headers(batch.frames(check=False), batch.canon)
    assert torch.equal(rep2, rep) and torch.equal(ver2, ver) and hs.cpu().tolist() == [0] * n
