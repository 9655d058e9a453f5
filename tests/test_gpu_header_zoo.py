"""Table builds and decodes on the GPU over canonical headers that no Huffman construction emits
(helpers.header_zoo; its classes are asserted in test_header_zoo.py).

Tables: the four builders of the 13-bit table -- mh_prepare_lut over T1/T2, mh_build_tables_device,
mh_build_luts_device, and header_build inside the decode kernel (copied out by
mh_header_luts_device) -- are each compared byte for byte with helpers.prepared_table_reference,
a plain numpy statement of what the prepared table holds, made from the oracle's 65,536-entry
table (not from another builder). Statuses are compared with the zoo's.

Decodes: frames of 96x56 (84 blocks: tile 0 has 64 blocks, which at >= 14 bits a symbol span more
than the 4,352-byte stage -- decode_halves -- and tile 1 has 20 and stays under it), packed under a
chosen header by helpers.encode_with_header from uniformly drawn used symbols, three distinct
frames per header, through every decode entry. The expected raster is the oracle's
decode_frame_shader with oracle.split_tables(canon), which must also be the image the symbols
integrate to. Every decode goes into a 0xA5-filled raster and every pixel is exact."""
from __future__ import annotations

import numpy as np
import pytest

from helpers import (PREPARED_BYTES, PREPARED_L13_BYTES, PREPARED_WORD_OFF, frame_under_header, header_zoo,
                     prepared_table_reference)

pytestmark = pytest.mark.gpu

W, H = 96, 56
STAGE_BYTES = 4352   # kStageBytes (mh_decode.hip)
T2_CAP = 257 * 256   # MH_TABLE2_MAX_ENTRIES


@pytest.fixture(scope="module")
def cus(device):
    import torch
    return torch.cuda.get_device_properties(device).multi_processor_count


_REFS: dict = {}


def _ref(oracle, z) -> np.ndarray:
    """The reference prepared table of a zoo header, computed once."""
    if z.name not in _REFS:
        r = prepared_table_reference(oracle, z.canon, z.status)
        r.setflags(write=False)
        _REFS[z.name] = r
    return _REFS[z.name]


def _first_diff(got, want):
    i = int(np.flatnonzero(got != want)[0])
    return f"first difference at byte {i}: {int(got[i]):#04x}, expected {int(want[i]):#04x}"


# ---- 1. tables ---------------------------------------------------------------------------------

def _batch_luts(fn, heads, device):
    """One launch of mh_build_luts_device / mh_header_luts_device over `heads` into 0xA5-filled
    slots of mh_lut_bytes() + 48 bytes -> (u8[n, stride], status list)."""
    import torch
    from metalhuffman_amd import _native as N
    lb = int(N.lib().mh_lut_bytes())
    assert lb == PREPARED_BYTES
    stride, n = lb + 48, len(heads)
    hdr = torch.from_numpy(np.stack([z.canon for z in heads])).to(device)
    luts = torch.full((n, stride), 0xA5, dtype=torch.uint8, device=device)
    status = torch.full((n,), 77, dtype=torch.int32, device=device)
    N.check(fn(hdr.data_ptr(), n, luts.data_ptr(), stride, status.data_ptr(),
               torch.cuda.current_stream(device).cuda_stream), "luts")
    torch.cuda.synchronize(device)
    return luts.cpu().numpy(), status.cpu().tolist()


def _check_batch(oracle, heads, got, st, whole_table):
    assert st == [z.status for z in heads], [(z.name, s) for z, s in zip(heads, st) if s != z.status][:8]
    for k, z in enumerate(heads):
        want = _ref(oracle, z)
        if whole_table:  # mh_build_luts_device: 13-bit table, 14-bit table, lengths word
            assert np.array_equal(got[k, :PREPARED_BYTES], want), (z.name, k, _first_diff(got[k, :PREPARED_BYTES], want))
        else:            # mh_header_luts_device: the 13-bit table and the word; the 14-bit table's bytes stay
            a, b = got[k, :PREPARED_L13_BYTES], want[:PREPARED_L13_BYTES]
            assert np.array_equal(a, b), (z.name, k, _first_diff(a, b))
            assert np.array_equal(got[k, PREPARED_WORD_OFF:PREPARED_BYTES], want[PREPARED_WORD_OFF:]), \
                (z.name, k, got[k, PREPARED_WORD_OFF:PREPARED_BYTES].view(np.uint32), want[PREPARED_WORD_OFF:].view(np.uint32))
            assert (got[k, PREPARED_L13_BYTES:PREPARED_WORD_OFF] == 0xA5).all(), (z.name, k)
    assert (got[:, PREPARED_BYTES:] == 0xA5).all()


@pytest.mark.parametrize("builder", ["mh_build_luts_device", "mh_header_luts_device"])
def test_batch_builders_match_the_reference_table(mh, oracle, device, builder):
    """The whole zoo (400 random complete codes, 50 incomplete, 32 hand-written, 7 rejected) in one
    launch, then again 70 headers per launch (another number of slices per table for
    mh_build_luts_device), cycling through the zoo until every header has been in such a launch.
    Every byte of every slot: the reference's where the builder writes, 0xA5 elsewhere."""
    from metalhuffman_amd import _native as N
    fn = getattr(N.lib(), builder)
    zoo = header_zoo()
    whole = builder == "mh_build_luts_device"
    got, st = _batch_luts(fn, zoo, device)
    _check_batch(oracle, zoo, got, st, whole)
    for lo in range(0, len(zoo), 70):
        heads = [zoo[i % len(zoo)] for i in range(lo, lo + 70)]
        got, st = _batch_luts(fn, heads, device)
        _check_batch(oracle, heads, got, st, whole)


def _table_subset():
    zoo = header_zoo()
    rnd = [z for z in zoo if z.kind == "random"]
    return [z for z in zoo if z.kind in ("hand", "rejected")] + rnd[::4]


def test_build_tables_device_matches_reference_and_host(mh, oracle, device):
    """mh_build_tables_device, one launch per header, for every hand-written and rejected header
    and every 4th random one: the prepared table against the reference, T1 / T2 / the used-entry
    count against the host builder (T2 over its whole capacity: zero past the used subtables), the
    status against the zoo's. A rejected header: all-zero T1 and T2, 256 entries, all-zero tables."""
    import torch
    from metalhuffman_amd import _native as N
    stream = torch.cuda.current_stream(device).cuda_stream
    heads = _table_subset()
    assert len(heads) == 32 + 7 + 100
    for z in heads:
        hdr = torch.from_numpy(z.canon.copy()).to(device)
        t1 = torch.full((512,), 0xA5, dtype=torch.uint8, device=device)
        t2 = torch.full((2 * T2_CAP,), 0xA5, dtype=torch.uint8, device=device)
        meta = torch.full((2,), 77, dtype=torch.int32, device=device)
        lut = torch.full((PREPARED_BYTES + 48,), 0xA5, dtype=torch.uint8, device=device)
        N.check(N.lib().mh_build_tables_device(hdr.data_ptr(), t1.data_ptr(), t2.data_ptr(), meta.data_ptr(),
                                               lut.data_ptr(), meta.data_ptr() + 4, stream), "mh_build_tables_device")
        torch.cuda.synchronize(device)
        entries, status = meta.cpu().tolist()
        assert status == z.status, (z.name, status)
        got = lut.cpu().numpy()
        want = _ref(oracle, z)
        assert np.array_equal(got[:PREPARED_BYTES], want), (z.name, _first_diff(got[:PREPARED_BYTES], want))
        assert (got[PREPARED_BYTES:] == 0xA5).all(), z.name
        g1, g2 = t1.cpu().numpy(), t2.cpu().numpy()
        if z.status == 0:
            h1, h2 = mh.Huffman.generateSplitLookupTables(z.canon)
            assert entries == h2.size // 2, (z.name, entries)
            assert np.array_equal(g1, h1), z.name
            assert np.array_equal(g2[: h2.size], h2) and not g2[h2.size:].any(), z.name
        else:
            assert entries == 256 and not g1.any() and not g2.any(), (z.name, entries)


def test_prepare_lut_over_host_tables_matches_the_reference(mh, oracle, device):
    """mh_prepare_lut over the host builder's T1 / T2 (T2 cut to its used entries), the accepted
    headers of the same subset."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    heads = [z for z in _table_subset() if z.status == 0]
    assert len(heads) == 132
    for z in heads:
        t1, t2 = mh.Huffman.generateSplitLookupTables(z.canon)
        tabs = D.DeviceTables.upload(t1, t2, device, prepare_lut=False)
        tabs.lut = torch.full((PREPARED_BYTES,), 0xA5, dtype=torch.uint8, device=device)
        N.check(N.lib().mh_prepare_lut(tabs.table1.data_ptr(), tabs.table2.data_ptr(), tabs.table2_entries,
                                       tabs.lut.data_ptr(), torch.cuda.current_stream(device).cuda_stream),
                "mh_prepare_lut")
        torch.cuda.synchronize(device)
        got = tabs.lut.cpu().numpy()
        want = _ref(oracle, z)
        assert np.array_equal(got, want), (z.name, _first_diff(got, want))


# ---- 2. decodes --------------------------------------------------------------------------------

def _decode_cases():
    """(id, header, format): every accepted hand-written header, 12 random ones (three of each
    longest length 13..16: the first, the middle and the last of that class), and a no-delta and
    an init-byte variant of {14: 2} and {16: 256}."""
    zoo = header_zoo()
    cases = [(z.name, z, "delta") for z in zoo if z.kind == "hand"]
    rnd = [z for z in zoo if z.kind == "random"]
    for longest in (13, 14, 15, 16):
        cls = [z for z in rnd if z.longest == longest]
        assert len(cls) >= 20
        cases += [(f"{z.name}-longest{longest}", z, "delta") for z in (cls[0], cls[len(cls) // 2], cls[-1])]
    by_name = {z.name: z for z in zoo}
    for name in ("14x2/a", "16x256/a"):
        cases += [(f"{name}-no_delta", by_name[name], "no_delta"), (f"{name}-init", by_name[name], "init_zero_delta")]
    return cases


CASES = _decode_cases()
DECODE = pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
_FRAMES: dict = {}


def _frames(oracle, case):
    """Three frames under the case's header, built once: [(EncodedFrame, expected raster)]. The
    expected raster is the oracle's shader decode, which must be the image."""
    name, z, fmt = case
    if name not in _FRAMES:
        out = []
        t1, t2 = oracle.split_tables(z.canon)
        for k in range(3):
            ef, img = frame_under_header(z.canon, W, H, seed=1000 * CASES.index(case) + k, no_delta=fmt == "no_delta",
                                         init_zero_delta=fmt == "init_zero_delta")
            want = oracle.decode_frame_shader(ef.block_offsets, ef.codes, t1, t2, W, H, block_init=ef.block_init,
                                              delta=fmt != "no_delta")
            assert np.array_equal(want, img), name
            want.setflags(write=False)
            out.append((ef, want))
        used = int((z.canon > 0).sum())
        if used > 1:
            assert len({ef.codes.tobytes() for ef, _ in out}) == 3, name
        o = out[0][0].block_offsets.astype(np.int64)
        if z.canon[z.canon > 0].min() >= 14:   # all-long: tile 0 oversize, tile 1 staged
            assert (o[64] - o[0]) // 8 > STAGE_BYTES > (8 * out[0][0].payload_bytes - o[64]) // 8, name
        _FRAMES[name] = out
    return _FRAMES[name]


def _expect(out, frames, n, what):
    got = out[..., :W].cpu().numpy()
    assert got.shape == (n, H, W)
    want = np.stack([f[1] for f in frames])[np.arange(n) % len(frames)]
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).reshape(n, -1).any(axis=1))
        f = int(bad[0])
        ys, xs = np.nonzero(got[f] != want[f])
        raise AssertionError(f"{what}: {bad.size} of {n} frame(s) wrong, first frame {f}: {ys.size} wrong pixel(s), "
                             f"first at row {int(ys[0])}, column {int(xs[0])}: {int(got[f, ys[0], xs[0]]):#04x}, "
                             f"expected {int(want[f, ys[0], xs[0]]):#04x}")


def _mh_decode(device, cus, frames, n, prepared, kernel):
    """n frames (cycling `frames`) through mh_decode with the host builder's T1 / T2 and, when
    `prepared`, mh_prepare_lut's table; asserts the tile count that routes the launch (launch()
    in mh_decode.hip)."""
    import torch
    from metalhuffman_amd import decoder as D
    efs = [frames[i % len(frames)][0] for i in range(n)]
    t1, t2 = efs[0].tables()
    tabs = D.DeviceTables.upload(t1, t2, device, prepare_lut=prepared)
    fr = D.DeviceFrames.pack(efs, device)
    tiles = -(-fr.n_blocks // 64) * n
    if kernel == "frame":
        assert prepared and n == 1 and fr.frame_code_offsets is None and tiles <= 4 * cus
    elif kernel == "small":
        assert prepared and fr.frame_code_offsets is not None and tiles <= 4 * cus
    elif kernel == "batch":   # 5-wave workgroups: the whole table copied, the flavour from its lengths word
        assert prepared and tiles > 4 * cus and -(-tiles // cus) >= 5
    elif kernel == "batch_inkernel_table":
        assert not prepared and tabs.lut is None
    else:
        raise KeyError(kernel)
    out = torch.full((n, H, W), 0xA5, dtype=torch.uint8, device=device)
    assert D.decode(fr, tabs, out=out) is out
    torch.cuda.synchronize(device)
    _expect(out, frames, n, kernel)


@DECODE
def test_mh_decode_one_frame(mh, oracle, device, cus, case):
    """mh_decode, one frame, prepared table: mh_decode_frame_kernel. Each of the three frames."""
    frames = _frames(oracle, case)
    for k in range(3):
        _mh_decode(device, cus, frames[k: k + 1], 1, True, "frame")


@DECODE
def test_mh_decode_three_frames(mh, oracle, device, cus, case):
    """mh_decode, three frames, prepared table: mh_decode_small_kernel."""
    _mh_decode(device, cus, _frames(oracle, case), 3, True, "small")


@DECODE
def test_mh_decode_large_batch(mh, oracle, device, cus, case):
    """mh_decode, 4 x CUs // 2 + 1 frames cycling the three (more than 4 x CUs tiles), prepared
    table: mh_decode_kernel, which takes its step flavour from the table's lengths word."""
    _mh_decode(device, cus, _frames(oracle, case), 4 * cus // 2 + 1, True, "batch")


@DECODE
def test_mh_decode_three_frames_without_prepared_table(mh, oracle, device, cus, case):
    """mh_decode, three frames, no prepared table: mh_decode_kernel builds its table itself."""
    _mh_decode(device, cus, _frames(oracle, case), 3, False, "batch_inkernel_table")


@DECODE
def test_mh_decode_frames(mh, oracle, device, case):
    """mh_decode_frames: a table per frame from mh_build_luts_device, statuses all zero."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = _frames(oracle, case)
    efs = [f[0] for f in frames]
    fr = D.DeviceFrames.pack(efs, device, shared_table=False)
    ts = D.DeviceTableSet.from_canonical_headers(np.stack([ef.canon for ef in efs]), device)
    out = torch.full((3, H, W), 0xA5, dtype=torch.uint8, device=device)
    assert D.decode_frames(fr, ts, out=out) is out
    torch.cuda.synchronize(device)
    assert ts.status.cpu().tolist() == [0, 0, 0]
    _expect(out, frames, 3, "mh_decode_frames")


@DECODE
def test_mh_decode_headers(mh, oracle, device, case):
    """mh_decode_headers: the table built in the decode kernel, header statuses all zero."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = _frames(oracle, case)
    efs = [f[0] for f in frames]
    fr = D.DeviceFrames.pack(efs, device, shared_table=False)
    out = torch.full((3, H, W), 0xA5, dtype=torch.uint8, device=device)
    hst = torch.full((3,), 77, dtype=torch.int32, device=device)
    assert D.decode_headers(fr, np.stack([ef.canon for ef in efs]), out=out, header_status=hst) is out
    torch.cuda.synchronize(device)
    assert hst.cpu().tolist() == [0, 0, 0]
    _expect(out, frames, 3, "mh_decode_headers")


def test_one_launch_of_every_header(mh, oracle, device):
    """All cases of the delta format in ONE mh_decode_frames and ONE mh_decode_headers launch, a
    frame per header: neighbouring workgroups take different step flavours."""
    import torch
    from metalhuffman_amd import decoder as D
    picked = [_frames(oracle, c)[1] for c in CASES if c[2] == "delta"]
    n = len(picked)
    efs = [f[0] for f in picked]
    canons = np.stack([ef.canon for ef in efs])
    fr = D.DeviceFrames.pack(efs, device, shared_table=False)
    ts = D.DeviceTableSet.from_canonical_headers(canons, device)
    out = torch.full((n, H, W), 0xA5, dtype=torch.uint8, device=device)
    D.decode_frames(fr, ts, out=out)
    torch.cuda.synchronize(device)
    assert not ts.status.any().item()
    _expect(out, picked, n, "mh_decode_frames, every header")
    out = torch.full((n, H, W), 0xA5, dtype=torch.uint8, device=device)
    hst = torch.full((n,), 77, dtype=torch.int32, device=device)
    D.decode_headers(fr, canons, out=out, header_status=hst)
    torch.cuda.synchronize(device)
    assert not hst.any().item()
    _expect(out, picked, n, "mh_decode_headers, every header")


STREAM = [c for c in CASES if c[0] == "14x2/a" or c[0].endswith("longest16")][:2]


@pytest.mark.parametrize("case", STREAM, ids=[c[0] for c in STREAM])
def test_header_mode_stream(mh, oracle, device, case):
    """The header-mode stream, {14: 2} and one random header with 16-bit codes: three frames
    through two slots into 0xA5-filled rasters, each checked before its slot is reused."""
    import torch
    from metalhuffman_amd.stream import HeaderFrameStream, pinned_frame_with_header
    frames = _frames(oracle, case)
    outs = [torch.full((H, W), 0xA5, dtype=torch.uint8, device=device) for _ in range(2)]
    fs = HeaderFrameStream(W, H, max(f[0].codes.size for f in frames), slots=2, device=device, outputs=outs)
    try:
        for k, (ef, want) in enumerate(frames):
            slot = fs.submit(*pinned_frame_with_header(ef))
            assert slot == k % 2
            fs.wait(slot)
            assert fs.slot_status(slot) == 0, k
            _expect(fs.output(slot)[None], [(ef, want)], 1, f"stream frame {k}")
            fs.output(slot).fill_(0xA5)
            torch.cuda.synchronize(device)
        fs.synchronize()
    finally:
        fs.close()
