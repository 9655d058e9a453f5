"""mh_decode_set_frames on the GPU: every frame of a set whole, each at its own size, in ONE launch
(include/metalhuffman.h). The sets are built from the smallest frames at which
each path of the entry can still go wrong (decode_set_helpers.SIZES): one lane, one block, a partial
block, exactly one full tile, a second tile of one lane, one block per row (a tile spanning 64 block
rows), a tile that straddles block rows, and a 1024 x 512 frame under a group budget that gives it two
workgroups, so that each of its waves grid-strides eight times. Every case is one launch into a buffer
with guard bytes on both sides, between the rasters and in the pitch padding; every byte is compared
with codec.decode_frame_cpu of the same frame, and every guard byte with its fill."""
from __future__ import annotations

import numpy as np
import pytest

import decode_set_helpers as H

pytestmark = pytest.mark.gpu

BUDGET = 2      # 139 tiles in all: round(2 * 128 / 139) = 2 groups for the 1024 x 512 frame, 1 for the others


def _decode(mh, oracle, device, sizes, headers, fmt="delta", shared=False, budget=BUDGET, pitch_align=0,
            guarded=True, block_order=None, alias=None, extra_flags=0):
    fr = H.frames(mh, oracle, sizes, headers, fmt)
    efs, wants = [f[0] for f in fr], [f[1] for f in fr]
    fs = H.pack(device, efs, block_order, alias)
    tabs = H.tables(device, efs, shared)
    rec = H.records(mh, fs, budget, pitch_align, guarded)
    lay = H.run(device, fs, tabs, rec, extra_flags=extra_flags)
    assert lay.rc == 0
    H.check(lay, rec.rasters, fs.sizes, wants)
    assert lay.status == [0] * len(sizes)
    return lay, rec


@pytest.mark.parametrize("shared", [False, True], ids=["table_per_frame", "shared_table"])
def test_every_size_in_one_set(mh, oracle, device, shared):
    """All eight sizes in one launch; a table per frame (the four flavours dealt in turn) or one shared
    table (lut_stride_bytes 0)."""
    lay, rec = _decode(mh, oracle, device, H.SIZES, ("escapes",) if shared else H.HEADERS, shared=shared)
    assert rec.shares[:, 1].tolist() == [1, 1, 1, 1, 1, 1, 1, 2] and rec.group_frame.size == 9


@pytest.mark.parametrize("header", H.HEADERS)
def test_each_table_flavour(mh, oracle, device, header):
    """The four step flavours slice_decode dispatches on, each over all the sizes under one table."""
    _decode(mh, oracle, device, H.SIZES, (header,), shared=True)


@pytest.mark.parametrize("size", [(1, 1), (9, 7), (520, 8), (8, 520), (1024, 512)], ids=str)
def test_a_set_of_one_frame(mh, oracle, device, size):
    """n = 1: no frame offsets array; the large frame under a budget of one resident round."""
    _decode(mh, oracle, device, (size,), ("noesc",), budget=2048 if size[0] == 1024 else 1)


@pytest.mark.parametrize("fmt", ["raw", "init"])
def test_formats(mh, oracle, device, fmt):
    """MH_FLAG_NO_DELTA, and block_init present (based at each frame's own first block)."""
    lay, _ = _decode(mh, oracle, device, H.SIZES, H.HEADERS, fmt)


@pytest.mark.parametrize("dense", [(0,), (9,), (0, 9, 16), (1, 2, 3, 4, 5, 6, 7)], ids=str)
def test_tiles_whose_codes_exceed_the_staging_window(mh, oracle, device, dense):
    """A 512 x 136 frame, 17 tiles on one workgroup: wave w owns tiles w, w + 8 (and wave 0 tile 16).
    The blocks of the `dense` tiles hold 16-bit codes only (8192 bytes a tile, above the 4352-byte
    window), the others the shortest codes: a wave decodes a dense tile unpipelined and goes back to
    the pipelined loop for its next tile -- as its first tile, between two others, or as its last."""
    from helpers import encode_with_header, image_of_symbols
    import slice_helpers as SH
    canon = SH.headers()["escapes"].canon
    longest, shortest = np.flatnonzero(canon == 16), np.flatnonzero(canon == canon[canon > 0].min())
    rng = np.random.default_rng([17, *dense])
    sym = rng.choice(shortest, (17, 64 * 64)).astype(np.uint8)
    for t in dense:
        sym[t] = rng.choice(longest, 64 * 64)
    big = encode_with_header(canon, sym.reshape(-1), 512, 136)
    ends = np.append(big.block_offsets.astype(np.int64), 8 * big.payload_bytes)[::64]
    assert [t for t in range(17) if ends[t + 1] - ends[t] > 8 * 4352] == list(dense)
    want = mh.decode_frame_cpu(big)
    assert np.array_equal(want, image_of_symbols(sym.reshape(-1), 512, 136))
    small = H.frame(mh, oracle, (9, 7), "escapes")
    efs, wants = [small[0], big], [small[1], want]
    fs, tabs = H.pack(device, efs), H.tables(device, efs)
    rec = H.records(mh, fs, 1)
    assert rec.shares[:, 1].tolist() == [1, 1]
    lay = H.run(device, fs, tabs, rec)
    assert lay.rc == 0 and lay.status == [0, 0]
    H.check(lay, rec.rasters, fs.sizes, wants)


def test_first_block_order_differs_from_frame_order(mh, oracle, device):
    """The block arrays hold the frames in another order than the frame numbers: first_block falls and
    rises; with block_init, which is based the same way."""
    order = [5, 0, 7, 2, 6, 1, 4, 3]
    _decode(mh, oracle, device, H.SIZES, H.HEADERS, block_order=order)
    _decode(mh, oracle, device, H.SIZES[:7], H.HEADERS, "init", block_order=[6, 4, 2, 0, 5, 3, 1])


def test_two_frames_share_block_entries(mh, oracle, device):
    """Frames 1 and 3 are the same stream in two code slots and name ONE run of block entries; their
    rasters are disjoint and both hold the picture."""
    sizes = ((264, 40), (520, 8), (9, 7), (520, 8))
    fr = [H.frame(mh, oracle, s, "escapes", "delta", j) for s, j in zip(sizes, (0, 1, 2, 1))]
    efs, wants = [f[0] for f in fr], [f[1] for f in fr]
    fs = H.pack(device, efs, alias={3: 1})
    assert fs.total_blocks == 165 + 65 + 2
    rec = H.records(mh, fs, 4)
    assert rec.geoms[1, 0] == rec.geoms[3, 0]
    lay = H.run(device, fs, H.tables(device, efs), rec)
    H.check(lay, rec.rasters, fs.sizes, wants)
    assert lay.rc == 0 and lay.status == [0] * 4


@pytest.mark.parametrize("guarded", [False, True], ids=["planner_rasters", "caller_pitch"])
def test_pitch_align_64(mh, oracle, device, guarded):
    """The planner's own rasters at pitch_align 64 (the alignment's padding is guarded), and a caller
    pitch larger than the planner's on the same grid."""
    lay, rec = _decode(mh, oracle, device, H.SIZES, H.HEADERS, pitch_align=64, guarded=guarded)
    assert all(int(r[0]) % 64 == 0 and int(r[2]) % 64 == 0 for r in rec.rasters)


def test_frame_status_skips_one_frame(mh, oracle, device):
    """A non-zero d_frame_status word: the frame's raster stays untouched, its word is carried into
    d_set_status, and its neighbours are decoded."""
    import torch
    fr = H.frames(mh, oracle)
    efs, wants = [f[0] for f in fr], [f[1] for f in fr]
    fs, tabs = H.pack(device, efs), H.tables(device, efs)
    rec = H.records(mh, fs, BUDGET)
    for victim, word in ((4, -3), (7, 12345), (0, -9)):
        st = torch.zeros(len(efs), dtype=torch.int32, device=device)
        st[victim] = word
        lay = H.run(device, fs, tabs, rec, frame_status=st)
        assert lay.rc == 0
        H.check(lay, rec.rasters, fs.sizes, [None if f == victim else w for f, w in enumerate(wants)])
        assert lay.status == [word if f == victim else 0 for f in range(len(efs))]
    # without d_set_status, and without d_frame_status (a shared table has none of its own)
    lay = H.run(device, fs, tabs, rec, frame_status=st, set_status=None)
    H.check(lay, rec.rasters, fs.sizes, [None if f == 0 else w for f, w in enumerate(wants)])
    lay = H.run(device, fs, tabs, rec, frame_status=None)
    H.check(lay, rec.rasters, fs.sizes, wants)


def test_any_order_flag_and_python_surface(mh, oracle, device):
    """decoder.decode_set_frames: the default plan (the kernel's resident workgroups as the budget,
    cached on the set), views of each frame's own size, the status tensor; and MH_FLAG_ANY_ORDER."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    fr = H.frames(mh, oracle)
    efs, wants = [f[0] for f in fr], [f[1] for f in fr]
    fs, tabs = D.DeviceFrameSet.pack(efs, device), H.tables(device, efs)
    resident, waves = D.decode_set_frames_shape(fs)
    assert waves == N.MH_DECODE_GROUP_WAVES and resident >= torch.cuda.get_device_properties(device).multi_processor_count
    views, status = D.decode_set_frames(fs, tabs, status=True)
    plan = fs.__dict__["_set_plan"][1]
    assert plan.plan.n_groups == mh.decode_set_plan([(0, w, h, 0) for w, h in fs.sizes], resident).n_groups
    torch.cuda.synchronize(device)
    assert status.cpu().tolist() == [0] * len(efs)
    for f, (v, want) in enumerate(zip(views, wants)):
        assert tuple(v.shape) == want.shape and np.array_equal(v.cpu().numpy(), want), f
    views2 = D.decode_set_frames(fs, tabs, extra_flags=N.MH_FLAG_ANY_ORDER)
    assert fs.__dict__["_set_plan"][1] is plan                      # planned and uploaded once
    torch.cuda.synchronize(device)
    assert all(np.array_equal(v.cpu().numpy(), w) for v, w in zip(views2, wants))
    # a caller's plan and output: guard bytes around a buffer of exactly out_bytes
    p = mh.decode_set_plan(fs.geoms.cpu().numpy().view(np.uint32), BUDGET, 64)
    buf = torch.full((p.out_bytes + 512,), H.FILL, dtype=torch.uint8, device=device)
    views3 = D.decode_set_frames(fs, tabs, plan=p, out=buf[256: 256 + p.out_bytes])
    torch.cuda.synchronize(device)
    assert all(np.array_equal(v.cpu().numpy(), w) for v, w in zip(views3, wants))
    host = buf.cpu().numpy()
    assert (host[:256] == H.FILL).all() and (host[256 + p.out_bytes:] == H.FILL).all()
    with pytest.raises(ValueError):
        D.decode_set_frames(fs, tabs, plan=p, out=buf[: p.out_bytes - 8])
    with pytest.raises(TypeError):
        D.decode_set_frames(D.DeviceFrames.pack(efs[:1], device), tabs)


def test_defect_isolation_through_the_set_entry(mh, oracle, device):
    """Five seeded cases of defect_helpers (2 to 5 frames, at least one clean, the others with damaged
    code bits, offsets or slots), repacked as a set: every pixel of a specified block equals the
    reference walk's, clean frames in full, and every guard byte keeps its fill."""
    import torch
    import defect_helpers as DH
    from metalhuffman_amd import decoder as D
    for i in range(5):
        case = DH.defect_case(mh, oracle, "frames", i)
        try:
            up, tabs, dfs = DH.upload(device, case)
            b, (_, _, W, Hh) = up.frames, case.grid
            n, nb = b.n_frames, b.n_blocks
            assert 2 <= n <= 5
            geoms = np.array([(f * nb, W, Hh, 0) for f in range(n)], np.uint32)
            fs = D.DeviceFrameSet(W, Hh, n, ((W, Hh),) * n, n * nb, b.block_offsets, b.codes, b.frame_code_offsets,
                                  torch.from_numpy(geoms.view(np.int32)).to(device), b.block_init, b.flags, 0)
            rec = H.records(mh, fs, 3 * n)
            lay = H.run(device, fs, tabs, rec, frame_status=None)
            assert lay.rc == 0 and lay.status == [0] * n
            H.check(lay, rec.rasters, fs.sizes, [df.want for df in dfs], care=[df.care for df in dfs])
        except Exception as e:
            raise AssertionError(f"{case.describe()}\n{type(e).__name__}: {e}") from e
