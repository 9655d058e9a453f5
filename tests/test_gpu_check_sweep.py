"""mh_check against the oracle, frame by frame (contract point 4: the report equals orc_check_frame's for
every frame of ANY input): over defect_helpers' seeded batches -- the decode entries' defect kinds plus
swapped offsets, an offset past the slot's end and a T2 truncated to 512 entries, which no decode entry
is given -- and over fixed edges of the one-thread-per-block grid. Every call writes into a report whose
bytes were 0xA5 before it and which lies between guard words (defect_helpers.gpu_check).

The sweep's range is test_gpu_defect_isolation.py's: MH_DEFECT_SWEEP_CASES cases from
MH_DEFECT_SWEEP_FIRST on, 40 from 0."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

import defect_helpers as DH

pytestmark = pytest.mark.gpu

CLEAN = [0, 0, 0, 0xFFFFFFFF]


def test_check_sweep(mh, oracle, device):
    first, count = DH.sweep_range()
    assert count >= 1
    for i in range(first, first + count):
        case = DH.defect_case(mh, oracle, DH.CHECK, i)
        up, tabs, dfs = DH.upload(device, case)
        DH.assert_reports(DH.gpu_check(device, up.frames, tabs), dfs, case.describe())


def _stall(b):
    """Under the single-symbol code ('0') a set bit at block b's start is a window no code matches: the
    block's 64 steps are zero width and it ends where it began."""
    def edit(slot, offs, payload):
        bit = int(offs[b])
        slot[bit >> 3] |= 0x80 >> (bit & 7)
    return edit


def _frames(oracle, gbw, gbh, n, hurt):
    """n single-symbol frames; hurt = {frame: [blocks]} get a stall each."""
    def edit(blocks):
        def go(slot, offs, payload):
            for b in blocks:
                _stall(b)(slot, offs, payload)
        return go
    return [DH.made_frame(oracle, "single", gbw, gbh, f, edit(hurt[f]) if f in hurt else None) for f in range(n)]


# nb x n_frames = 255, 256, 257, 513 blocks under 256-thread workgroups
GRIDS = {255: (17, 5, 3), 256: (8, 8, 4), 257: (257, 1, 1), 513: (19, 9, 3)}


@pytest.mark.parametrize("total", sorted(GRIDS))
def test_workgroup_and_frame_boundaries(mh, oracle, device, total):
    """One defective block at a time, on each side of every workgroup boundary and of every frame boundary
    of the batch (and in its first and last block): the report names that frame and that block, and every
    other frame stays clean."""
    gbw, gbh, n = GRIDS[total]
    nb = gbw * gbh
    assert nb * n == total
    edges = {0, total - 1}
    for g in list(range(256, total, 256)) + list(range(nb, total, nb)):
        edges |= {g - 1, g}
    tabs = None
    for g in sorted(edges):
        f, b = divmod(g, nb)
        dfs = _frames(oracle, gbw, gbh, n, {f: [b]})
        want = [64, 0, int(b < nb - 1), b]
        assert [df.report.tolist() for df in dfs] == [want if j == f else CLEAN for j in range(n)], (g, f, b)
        tabs = tabs or DH.check_tables(device, dfs[0])
        fr = DH.pack(device, dfs, 8 * gbw, 8 * gbh)
        DH.assert_reports(DH.gpu_check(device, fr, tabs), dfs, f"{total} blocks, defect in global block {g}")


@pytest.mark.parametrize("offsets", [False, True], ids=["no_offset_array", "offset_array"])
def test_one_frame_with_and_without_an_offset_array(mh, oracle, device, offsets):
    def edit(slot, offs, payload):
        offs[7] += 3                                   # block 6 ends 3 bits early
        slot[int(offs[20]) >> 3] ^= 0x10               # a flipped bit inside block 20
        slot[payload - 1:] = 0                         # ... and a slot whose last code byte reads 0
    df = DH.made_frame(oracle, "escapes", 9, 5, 1, edit)
    assert int(df.report[2]) >= 1 and int(df.report[3]) == 6
    fr = DH.pack(device, [df], 72, 40, force_offsets=offsets)
    assert (fr.frame_code_offsets is not None) == offsets
    DH.assert_reports(DH.gpu_check(device, fr, DH.check_tables(device, df)), [df], "one frame")


def test_a_short_slot_reads_zero_not_its_neighbour(mh, oracle, device):
    """A slot cut in front of its last two blocks: the bytes behind it are the next frame's (or lie
    outside every slot) and must read as zero. Under the single-symbol code block 30 is then all '0'
    codes and ends on block 31's offset, and block 31 -- whose real bytes, all ones, would stall it --
    walks on without a stall; it counts in [2] only because it ends outside the slot."""
    def ones(slot, offs, payload):
        slot[payload - 8: payload] = 0xFF              # the last block: 64 one bits
    full = DH.made_frame(oracle, "single", 16, 2, 3, ones)
    assert full.ef.codes.size == 272 and full.report.tolist() == [64, 0, 0, 31]
    cut = dataclasses.replace(full, ef=dataclasses.replace(full.ef, codes=full.ef.codes[:240].copy()),
                              tail=full.ef.codes[240:].copy())
    DH._reference(oracle, cut, 128, 16, False, 0)
    assert cut.report.tolist() == [0, 0, 1, 31], "zeros from the slot's end on: no stall, one block outside the slot"
    tabs = DH.check_tables(device, full)
    for dfs in ([cut, full], [full, cut], [cut]):
        fr = DH.pack(device, dfs, 128, 16)
        DH.assert_reports(DH.gpu_check(device, fr, tabs), dfs, [d.ef.codes.size for d in dfs])


def test_the_byte_at_the_slots_end_reads_zero(mh, oracle, device):
    """The window's third byte at index i + 2 == slot bytes is outside the slot. up to 60 frames of long codes
    in one batch, each cut at a 16-byte boundary inside block b, with the offsets behind b re-chained
    to where the reference walk (zeros from the cut on) ends: by the oracle every block ends on the next
    one's offset and only the last counts in [2], for ending outside the slot. That stays so only if
    block b's codes across the cut see zeros -- the byte that follows a slot in memory is the next
    frame's first code byte, and 0xFF behind the last."""
    dfs = []
    for seed in range(12):
        for b in range(2, 7):
            df = DH.made_frame(oracle, "escapes", 9, 1, seed)
            offs = df.ef.block_offsets.copy()
            cut = -(-int(offs[b]) // 128) * 16
            if 8 * cut >= int(offs[b + 1]):
                continue
            slot = df.ef.codes[:cut].copy()
            t1, t2 = df.ef.tables()
            for j in range(b, offs.size - 1):
                offs[j + 1] = oracle.walk_frame(offs, slot, t1, t2)[0][j]
            df = dataclasses.replace(df, ef=dataclasses.replace(df.ef, codes=slot, block_offsets=offs),
                                     tail=np.full(16, 0xFF, np.uint8))
            DH._reference(oracle, df, 72, 8, False, 0)
            assert df.report.tolist() == [0, 0, 1, 8] and int(offs[b]) < 8 * cut < int(df.ends[b])
            dfs.append(df)
    assert len(dfs) >= 40
    fr = DH.pack(device, dfs, 72, 8)
    DH.assert_reports(DH.gpu_check(device, fr, DH.check_tables(device, dfs[0])), dfs, "cut slots")


@pytest.mark.parametrize("pair", [(3, 5), (62, 64), (200, 260), (255, 256), (10, 300)])
def test_two_defects_report_the_smaller_block(mh, oracle, device, pair):
    """[3] is a minimum, whichever thread comes last: two blocks of one lane group, of two waves, and of
    two workgroups with the larger block in the EARLIER slot of its workgroup (260 is thread 4 of the
    second, 200 thread 200 of the first)."""
    lo, hi = pair
    dfs = _frames(oracle, 40, 8, 2, {0: [lo, hi]})
    assert dfs[0].report.tolist() == [128, 0, 2, lo] and dfs[1].report.tolist() == CLEAN
    fr = DH.pack(device, dfs, 320, 64)
    DH.assert_reports(DH.gpu_check(device, fr, DH.check_tables(device, dfs[0])), dfs, pair)


def test_side_stream_after_an_upload_on_it(mh, oracle, device):
    """The call is ordered on the stream it is given: the codes arrive through a copy queued on a side
    stream just before it; the buffer held 0xFF bytes (every block a stall) until then."""
    import torch
    dfs = _frames(oracle, 33, 4, 3, {1: [40], 2: [0, 131]})
    fr = DH.pack(device, dfs, 264, 32)
    tabs = DH.check_tables(device, dfs[0])
    host = fr.codes.cpu().pin_memory()
    late = torch.full_like(fr.codes, 0xFF)
    torch.cuda.synchronize(device)
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        late.copy_(host, non_blocking=True)
    got = DH.gpu_check(device, dataclasses.replace(fr, codes=late), tabs, stream=side)
    DH.assert_reports(got, dfs, "side stream")
