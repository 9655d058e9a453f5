"""mh_encode_set_device_async at its limits, through the raw ABI into guard-filled outputs against the
host codec frame by frame (set_encode_helpers.py): a loader batch of 768 frames, the dimension limits,
the tile and pack-unit thresholds in mixed sets, the largest row pitch of one record, totals that are
smaller than the plan's (the header's "a stale plan cannot store outside the caller's arrays"), and
two sets in flight on two streams."""
from __future__ import annotations

import numpy as np
import pytest

import encode_helpers as EH
import set_encode_helpers as SH
from encode_helpers import CAPACITY, FILL_BYTES, OK

pytestmark = pytest.mark.gpu

SPAN_MAX = 0x7FFFFFF0           # MH_IMAGE_TILE_SPAN_MAX
BIG = (264, 256)                # 33 x 32 blocks: 5 tiles, 2 pack units


# ---- many frames ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def loader_batch(mh, bigbridge):
    """256 three-channel images of seeded sizes in 1..40 x 1..40, images 0, 128 and 255 of 264 x 256:
    768 plane frames, and what the host codec makes of each (computed once, left unchanged)."""
    r = np.random.default_rng(768)
    sizes = [BIG if i in (0, 128, 255) else (int(r.integers(1, 41)), int(r.integers(1, 41))) for i in range(256)]
    planes_of = [SH.images(bigbridge, [s] * 3, seed=100 + 3 * i) for i, s in enumerate(sizes)]
    imgs = [p for planes in planes_of for p in planes]
    free = SH.expect(mh, imgs, [1 << 62] * len(imgs), 0, True)
    assert len(imgs) == 768 and all(s == OK for s, _ in free)
    return sizes, planes_of, imgs, free


@pytest.mark.parametrize("pitch_extra", [0, 1], ids=["dwords", "bytes"])
def test_many_frames(mh, device, loader_batch, pitch_extra):
    """Every one of the 768 frames against the host codec: the tile offsets at first_tile + f + t, the
    tree grid of one workgroup per frame and both plan maps at a loader batch's frame count."""
    from metalhuffman_amd import _native as N
    sizes, planes_of, imgs, free = loader_batch
    srcs = SH.interleaved_sources(device, planes_of, 3, pitch_extra)
    r, _ = SH.run(mh, device, imgs, srcs, init_zero=True)
    assert r.plan.totals.fetch_mode == (3 if pitch_extra == 0 else N.MH_SET_FETCH_BYTES)
    assert r.plan.totals.n_frames == 768 and r.plan.totals.total_tiles == 759 + 9 * 5
    SH.check(r, free)


@pytest.mark.parametrize("pitch_extra", [0, 1], ids=["dwords", "bytes"])
def test_many_frames_stripped(mh, device, loader_batch, pitch_extra):
    """The same set with a 16-byte slot for every one-tile frame: each is rejected with -4 (but the few
    whose codes fit 16 bytes), and the nine planes of the three large images, at frames 0..2, 384..386
    and 765..767, are exact all the same -- tile_off, tile_tail and the meta words behind hundreds of
    rejected frames."""
    sizes, planes_of, imgs, free = loader_batch
    caps = [SH.roomy_cap(*BIG) if sizes[f // 3] == BIG else 16 for f in range(768)]
    exp = [(s, ef) if EH.r4(ef.codes.size) <= c else (CAPACITY, None) for (s, ef), c in zip(free, caps)]
    large = [f for f in range(768) if sizes[f // 3] == BIG]
    assert large == [0, 1, 2, 384, 385, 386, 765, 766, 767] and all(exp[f][0] == OK for f in large)
    assert sum(s == CAPACITY for s, _ in exp) >= 700, sum(s == CAPACITY for s, _ in exp)
    srcs = SH.interleaved_sources(device, planes_of, 3, pitch_extra)
    r, _ = SH.run(mh, device, imgs, srcs, init_zero=True, caps=caps)
    SH.check(r, exp)


# ---- the dimension limits -------------------------------------------------------------------------------------

@pytest.mark.parametrize("aligned", [True, False], ids=["dwords", "bytes"])
def test_dimension_limits(mh, device, bigbridge, aligned):
    """65535 in either dimension beside tiny frames: 8192 blocks, 32 tiles and 8 pack units a frame. The
    height-1 frame's row_pitch is garbage in its source record (the contract ignores it there)."""
    from metalhuffman_amd import _native as N
    sizes = [(65535, 8), (3, 5), (8, 65535), (65535, 1), (1, 65535), (9, 7)]
    imgs = SH.images(bigbridge, sizes, seed=61)
    srcs = SH.planar_sources(device, imgs, aligned)
    srcs[3].pitch = 0xFFFF_FFFF_FFFF_FFF3
    r, _ = SH.run(mh, device, imgs, srcs, init_zero=True)
    assert r.plan.totals.fetch_mode == (1 if aligned else N.MH_SET_FETCH_BYTES)
    assert [int(q.n_tiles) for q in r.plan.records] == [32, 1, 32, 32, 32, 1] and r.plan.records[3].row_pitch == 0
    exp = SH.expect(mh, imgs, r.caps, 0, True)
    assert all(s == OK for s, _ in exp)
    SH.check(r, exp)


# ---- the thresholds in mixed sets -----------------------------------------------------------------------------

@pytest.mark.parametrize("first", range(0, len(EH.THRESHOLD_WIDTHS), 3))
def test_thresholds_in_mixed_sets(mh, device, bigbridge, first):
    """All of encode_helpers.threshold_shapes("batch", bw) for three widths at a time in one set, in a
    seeded order: block counts on, below and above one packer step, one tile and one pack unit
    (test_encode_sweep_cases.py asserts the counts), each beside frames of other tile counts."""
    from metalhuffman_amd import _native as N
    sizes = [s for bw in EH.THRESHOLD_WIDTHS[first: first + 3] for s in EH.threshold_shapes("batch", bw)]
    sizes = [sizes[k] for k in np.random.default_rng(first).permutation(len(sizes))]
    imgs = SH.images(bigbridge, sizes, seed=7 + first)
    exp = None
    for aligned in (True, False):
        srcs = SH.planar_sources(device, imgs, aligned)
        r, _ = SH.run(mh, device, imgs, srcs, flags=EH.LIMIT, init_zero=aligned)
        assert r.plan.totals.fetch_mode == (1 if aligned else N.MH_SET_FETCH_BYTES)
        exp = SH.expect(mh, imgs, r.caps, EH.LIMIT, aligned)
        assert all(s == OK for s, _ in exp)
        SH.check(r, exp)


# ---- the pitch limit of one record ----------------------------------------------------------------------------

@pytest.mark.parametrize("aligned", [True, False], ids=["dwords", "bytes"])
def test_the_pitch_limit_of_one_record(mh, device, bigbridge, aligned):
    """A 13 x 3 frame whose rows are the largest admitted pitch apart, (3 - 1) * pitch + 13 =
    MH_IMAGE_TILE_SPAN_MAX - 1 (rounded down to a multiple of 4 for the dword mode), between two ordinary
    frames. The ~2 GiB span is built on the device with only its rows written. One byte more is refused
    by the planner (also asserted on the CPU in test_encode_set_plan.py)."""
    import torch
    from metalhuffman_amd import _native as N
    w, h = 13, 3
    pitch = (SPAN_MAX - w) // (h - 1)
    if aligned:
        pitch -= pitch % 4
    imgs = SH.images(bigbridge, [(264, 120), (w, h), (37, 50)], seed=29)
    srcs = SH.planar_sources(device, imgs, aligned)
    t = torch.empty((h - 1) * pitch + w + 512, dtype=torch.uint8, device=device)
    o = (t.data_ptr() + 255) // 256 * 256 - t.data_ptr() + (64 if aligned else 61)
    t[o:].as_strided((h, w), (pitch, 1)).copy_(torch.from_numpy(imgs[1]).to(device))
    srcs[1] = SH.Source(t, t.data_ptr() + o, pitch, 1)
    r, _ = SH.run(mh, device, imgs, srcs, init_zero=True)
    assert r.plan.totals.fetch_mode == (1 if aligned else N.MH_SET_FETCH_BYTES)
    exp = SH.expect(mh, imgs, r.caps, 0, True)
    assert all(s == OK for s, _ in exp)
    SH.check(r, exp)
    over = [(s.pixels, s.pitch, s.ps, im.shape[1], im.shape[0], c) for s, im, c in zip(srcs, imgs, r.caps)]
    over[1] = (over[1][0], (SPAN_MAX - w) // (h - 1) + 1) + over[1][2:]
    with pytest.raises(mh.MHError) as e:
        mh.encode_set_plan(over)
    assert e.value.status == CAPACITY


# ---- stale totals ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("init_zero", [True, False], ids=["init", "no_init"])
def test_totals_smaller_than_the_plan(mh, device, bigbridge, init_zero):
    """The header: the kernels' stores are bounded by the totals, so a stale plan cannot store outside the
    caller's arrays. Five frames are planned; the entry gets a copy of the totals whose total_blocks ends
    in the middle of frame 3's blocks and whose codes_bytes ends in the middle of frame 3's code bytes
    (n_frames, the tile counts, the grids and the workspace size as planned). Every output tensor keeps
    its full planned size inside its guards, so a bound that failed would still write inside this test's
    own memory. Frames 0..2 are the host codec's; nothing at or behind either cut is written;
    d_frame_code_offsets[n] is the cut codes_bytes. What frames 3 and 4 leave in front of the cuts, and
    their headers, lengths and status words, is unspecified and not compared."""
    sizes = [(40, 30), BIG, (9, 7), (520, 200), (128, 64)]
    imgs = SH.images(bigbridge, sizes, seed=83)
    srcs = SH.planar_sources(device, imgs, True)
    caps = [SH.roomy_cap(w, h) for w, h in sizes]
    exp = SH.expect(mh, imgs, caps, EH.LIMIT, init_zero)
    assert all(s == OK for s, _ in exp)
    plan = mh.encode_set_plan([(s.pixels, s.pitch, s.ps, w, h, c) for s, (w, h), c in zip(srcs, sizes, caps)], EH.LIMIT)
    rec = plan.records[3]
    assert rec.n_tiles == 7 and rec.n_blocks == 65 * 25
    cut = type(plan.totals).from_buffer_copy(plan.totals)
    cut.total_blocks = rec.first_block + rec.n_blocks // 2
    cut.codes_bytes = rec.slot_offset + EH.r16(exp[3][1].codes.size // 2)
    assert rec.slot_offset < cut.codes_bytes < rec.slot_offset + exp[3][1].codes.size
    r, _ = SH.run(mh, device, imgs, srcs, flags=EH.LIMIT, init_zero=init_zero, caps=caps, totals=cut)
    assert bytes(r.plan.plan) == bytes(plan.plan)
    SH.check(r, exp, frames=range(3), fco_end=int(cut.codes_bytes))
    behind = r.host["codes"][int(cut.codes_bytes):]
    assert (behind == FILL_BYTES).all(), f"{int((behind != FILL_BYTES).sum())} code byte(s) written behind codes_bytes"
    offs = r.host["offs"].view(np.uint32)[int(cut.total_blocks):]
    assert (offs == 0x3C3C3C3C).all(), f"{int((offs != 0x3C3C3C3C).sum())} block offset(s) written behind total_blocks"
    if init_zero:
        init = r.host["init"][int(cut.total_blocks):]
        assert (init == FILL_BYTES).all(), f"{int((init != FILL_BYTES).sum())} init byte(s) written behind total_blocks"


# ---- two sets in flight ---------------------------------------------------------------------------------------

def test_two_sets_in_flight(mh, device, bigbridge):
    """Two different sets on two streams with separate workspaces, one synchronisation: both exact."""
    import torch
    sets = [(SH.EDGE_SET, True, EH.LIMIT, True), (SH.EDGE_SET[::-1][:5] + [(300, 300)], False, EH.NO_DELTA | EH.LIMIT, False)]
    made = []
    for k, (sizes, aligned, flags, init_zero) in enumerate(sets):
        imgs = SH.images(bigbridge, sizes, seed=40 + k)
        made.append((imgs, SH.planar_sources(device, imgs, aligned), flags, init_zero))
    torch.cuda.synchronize(device)          # the sources are written; the streams below do not wait for the default one
    streams = [torch.cuda.Stream(device), torch.cuda.Stream(device)]
    runs = [SH.run(mh, device, imgs, srcs, flags=flags, init_zero=init_zero, stream=s, sync=False)[0]
            for (imgs, srcs, flags, init_zero), s in zip(made, streams)]
    torch.cuda.synchronize(device)
    for r, (imgs, _, flags, init_zero) in zip(runs, made):
        r.collect()
        exp = SH.expect(mh, imgs, r.caps, flags, init_zero)
        assert all(s == OK for s, _ in exp)
        SH.check(r, exp)
