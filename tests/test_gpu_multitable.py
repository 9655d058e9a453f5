"""Batches with one Huffman table per frame: mh_build_luts_device (n prepared tables in one
launch) and mh_decode_frames (frame f decoded with table f), against the oracle's
shader-semantics decode and the encoder inputs -- never against mh_decode's output alone.
Every case is bit-exact."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from helpers import (check_containment, containment_plan, fibonacci_deltas, image_from_block_deltas,
                     long_span_deltas)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cus(device):
    import torch
    return torch.cuda.get_device_properties(device).multi_processor_count


def _oracle_decode(O, ef, tables=None):
    t1, t2 = tables if tables is not None else ef.tables()
    return O.decode_frame_shader(ef.block_offsets, ef.codes, t1, t2, ef.width, ef.height,
                                 block_init=ef.block_init, delta=not (ef.flags & 1))


def _shape(device, w, h, n, flags=0):
    """(workgroups per frame, waves per workgroup) of an n-frame w x h launch."""
    import torch
    from metalhuffman_amd import _native as N
    fr = N.mh_frame()
    fr.dims = N.mh_dims(w, h, (w + 7) // 8, (h + 7) // 8)
    fr.n_frames, fr.flags = n, flags
    g, wv = ctypes.c_uint32(), ctypes.c_uint32()
    N.check(N.lib().mh_decode_frames_shape(ctypes.byref(fr), torch.cuda.current_stream(device).cuda_stream,
                                           ctypes.byref(g), ctypes.byref(wv)), "mh_decode_frames_shape")
    assert wv.value == 8
    return int(g.value), int(wv.value)


def _tiles(w, h):
    return -(-(((w + 7) // 8) * ((h + 7) // 8)) // 64)


def _decode_mixed(device, efs, fill=0xA5, skip_rejected=True, extra_flags=0, canons=None):
    """efs through DeviceFrames.pack(shared_table=False) + DeviceTableSet + decode_frames into a
    raster prefilled with `fill` -> (u8[n, H, W] on the host, status list)."""
    import torch
    from metalhuffman_amd import decoder as D
    fr = D.DeviceFrames.pack(efs, device, shared_table=False)
    ts = D.DeviceTableSet.from_canonical_headers(np.stack([ef.canon for ef in efs] if canons is None else canons),
                                                 device)
    out = torch.full((len(efs), fr.height, (fr.width + 7) // 8 * 8), fill, dtype=torch.uint8, device=device)
    got = D.decode_frames(fr, ts, out=out, skip_rejected=skip_rejected, extra_flags=extra_flags)
    assert got is out
    torch.cuda.synchronize(device)
    return out[..., : fr.width].cpu().numpy(), ts.status.cpu().tolist()


def _crops(mh, bigbridge, w, h, n, **kw):
    """n crops of a tiled BigBridge at n different origins, n different histograms, encoded with
    the host codec -> (images, frames). Origins whose tree is deeper than 16 bits are passed over."""
    src = np.tile(bigbridge, (3, 3))
    sh, sw = src.shape
    imgs, efs = [], []
    for k in range(4 * n + 16):
        im = np.ascontiguousarray(src[37 * k % (sh - h):, 101 * k % (sw - w):][:h, :w])
        try:
            efs.append(mh.encode_frame(im, **kw))
        except mh.MHError as e:
            assert e.status == -3
            continue
        imgs.append(im)
        if len(imgs) == n:
            return imgs, efs
    raise AssertionError("too few encodable crops")


# ---- 1. tables ----------------------------------------------------------------------------

def _six_headers(mh, bigbridge):
    from metalhuffman_amd import _native as N
    from metalhuffman_amd import frames as F
    h = w = 256
    too_long = np.zeros(256, np.uint8)  # the 19-symbol Fibonacci histogram: deeper than 16 bits
    freq = np.bincount(fibonacci_deltas(19, h * w, seed=2), minlength=256).astype(np.uint64)
    assert N.lib().mh_code_lengths(freq.ctypes.data_as(N._u64p),
                                   too_long.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))) == -3
    assert too_long.max() > 16 and int((too_long > 0).sum()) == 19
    kraft = np.zeros(256, np.uint8)
    kraft[[1, 2, 3]] = 1  # three 1-bit codes: not a prefix code
    heads = [mh.encode_frame(np.ascontiguousarray(bigbridge[:h, 500:500 + w])).canon,
             mh.encode_frame(F.uniform_random(w, h, 5)).canon,
             mh.encode_frame(image_from_block_deltas(fibonacci_deltas(15, h * w, seed=4), w, h)).canon,
             mh.encode_frame(np.where(np.arange(h * w).reshape(h, w) % 3 == 0, 7, 0).astype(np.uint8),
                             flags=mh.MH_FLAG_NO_DELTA).canon,
             too_long, kraft]
    assert (heads[1] == 8).all() and heads[2].max() == 14 and int((heads[3] > 0).sum()) == 2
    return heads, [0, 0, 0, 0, -3, -5]


def test_luts_match_single_header_build(mh, device, bigbridge):
    """mh_build_luts_device for 6 headers (natural, flat8, 14-bit Fibonacci, two-symbol, one
    deeper than 16 bits, one breaking Kraft) is byte-identical over mh_lut_bytes() to six
    mh_build_tables_device calls, at a stride larger than the table whose padding stays
    untouched; a bad header shows in its own status word only. n = 1, 6 and 70 headers
    (launch shapes of 32, 32 and 3 slices per table on 256 CUs)."""
    import torch
    from metalhuffman_amd import _native as N
    from metalhuffman_amd import decoder as D
    heads, want_status = _six_headers(mh, bigbridge)
    lb = int(N.lib().mh_lut_bytes())
    ref = []
    for hd, st in zip(heads, want_status):
        t = D.DeviceTables.from_canonical_header(hd, device)
        torch.cuda.synchronize(device)
        assert int(t._meta[1].item()) == st
        ref.append(t.lut.cpu().numpy().copy())
        assert ref[-1].size == lb
    assert not ref[4][:-16].any() and not ref[5][:-16].any()  # rejected: all-zero tables
    stride = lb + 48
    stream = torch.cuda.current_stream(device).cuda_stream
    for idx in ([0], [1], [2], [3], [4], [5], list(range(6)), [i % 6 for i in range(70)]):
        n = len(idx)
        hdr = torch.from_numpy(np.stack([heads[i] for i in idx])).to(device)
        luts = torch.full((n, stride), 0xA5, dtype=torch.uint8, device=device)
        status = torch.full((n,), 77, dtype=torch.int32, device=device)
        N.check(N.lib().mh_build_luts_device(hdr.data_ptr(), n, luts.data_ptr(), stride, status.data_ptr(), stream),
                "mh_build_luts_device")
        torch.cuda.synchronize(device)
        got = luts.cpu().numpy()
        assert status.cpu().tolist() == [want_status[i] for i in idx], idx
        for k, i in enumerate(idx):
            assert np.array_equal(got[k, :lb], ref[i]), (n, k, i)
        assert (got[:, lb:] == 0xA5).all(), n
    # the Python wrapper: same tables, and check_status names the rejected frames
    ts = D.DeviceTableSet.from_canonical_headers(np.stack(heads), device)
    with pytest.raises(mh.MHError) as ei:
        ts.check_status()
    assert ei.value.status == -3 and "[4, 5]" in str(ei.value)
    assert np.array_equal(ts.luts.cpu().numpy()[:, :lb], np.stack(ref))


# ---- 2. mixed batch through the asynchronous chain -------------------------------------------

def _mixed_five(mh, bigbridge, raw):
    """The frames of test_batch_mixed_histograms_and_rejected_frame (256 x 256, 16 tiles); raw:
    the delta streams themselves as pixels, for MH_FLAG_NO_DELTA."""
    from metalhuffman_amd import frames as F
    h = w = 256
    fib = lambda n, seed: fibonacci_deltas(n, h * w, seed=seed)
    as_img = (lambda d: d.reshape(h, w)) if raw else (lambda d: image_from_block_deltas(d, w, h))
    return [np.ascontiguousarray(bigbridge[:h, 500:500 + w]), F.uniform_random(w, h, 5), as_img(fib(15, 4)),
            as_img(fib(19, 2)), np.where(np.arange(h * w).reshape(h, w) % 3 == 0, 7, 0).astype(np.uint8)]


def _flavour(canon):
    used = canon[canon > 0]
    mx, mn = int(used.max()), int(used.min())
    if mx == mn == 8 and used.size == 256:
        return "flat8"
    return "flat" if mx == mn else "noesc" if mx <= 13 else "general"


@pytest.mark.parametrize("variant", ["delta", "init_zero_delta", "no_delta"])
def test_mixed_batch_encode_tables_decode_chain(mh, oracle, device, bigbridge, variant):
    """encode batch -> n tables -> decode batch with no host synchronisation in between
    (BatchEncoder.encode_async(...).decode()): frames with unrelated histograms, one of them
    rejected by the encoder (delta and no-delta formats). Every valid frame equals its input
    and the oracle's decode with its own tables; the rejected frame's raster keeps its fill."""
    import torch
    from metalhuffman_amd.encoder import BatchEncoder
    flags = mh.MH_FLAG_NO_DELTA if variant == "no_delta" else 0
    init = variant == "init_zero_delta"
    imgs = _mixed_five(mh, bigbridge, raw=bool(flags))
    refs, rejected = [], []
    for f, im in enumerate(imgs):  # what the host codec says about each frame
        try:
            refs.append(mh.encode_frame(im, flags=flags, init_zero_delta=init))
        except mh.MHError as e:
            assert e.status == -3
            refs.append(None)
            rejected.append(f)
    assert rejected == ([] if init else [3]), rejected  # (moving the first deltas out flattens frame 3's tree)
    flavours = {_flavour(r.canon) for r in refs if r is not None}
    # the step flavours one launch mixes (the no-delta set holds all four)
    assert flavours == {"delta": {"flat8", "general", "noesc"}, "init_zero_delta": {"general", "noesc"},
                        "no_delta": {"flat8", "flat", "general", "noesc"}}[variant], flavours
    enc = BatchEncoder(256, 256, len(imgs), device)
    grays = torch.from_numpy(np.stack(imgs)).to(device)
    out = torch.full((len(imgs), 256, 256), 0xA5, dtype=torch.uint8, device=device)
    a = enc.encode_async(grays, flags, init)
    got = a.decode(out=out)  # asynchronous: nothing above or in here waits for the device
    assert got is out
    torch.cuda.synchronize(device)
    host = out.cpu().numpy()
    st = a.tables.status.cpu().tolist()
    assert [f for f, s in enumerate(st) if s] == rejected and all(st[f] == -3 for f in rejected), st
    assert a.status.cpu().tolist() == st
    for f, im in enumerate(imgs):
        if f in rejected:
            assert (host[f] == 0xA5).all(), f
        else:
            assert np.array_equal(host[f], im), f
            assert np.array_equal(host[f], _oracle_decode(oracle, refs[f])), f
    if rejected:
        with pytest.raises(mh.MHError):
            a.tables.check_status()


# ---- 3. shapes -------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [(1, 1), (9, 17), (72, 24), (512, 512), (1001, 777), (2056, 2048)])
def test_shapes_three_distinct_frames(mh, oracle, device, bigbridge, hw):
    """Partial tiles, block counts that are no multiple of 64, one-block frames, and frames whose
    tiles are fewer than, equal to (512 x 512: 64 tiles on 8 workgroups) or -- by the clamp, never
    for 3 frames -- more than 8 G waves' worth; with and without per-block init bytes."""
    h, w = hw
    G, _ = _shape(device, w, h, 3)
    tpf = _tiles(w, h)
    assert G == min(G, -(-tpf // 8)) and tpf <= 8 * G
    if hw == (512, 512):
        assert tpf == 8 * G
    for init in (False, True):
        imgs, efs = _crops(mh, bigbridge, w, h, 3, init_zero_delta=init)
        if h * w >= 4096:
            assert len({ef.canon.tobytes() for ef in efs}) == 3
        out, st = _decode_mixed(device, efs)
        assert st == [0, 0, 0]
        for f, im in enumerate(imgs):
            assert np.array_equal(out[f], im), (hw, init, f)
        if h * w <= 1001 * 777:
            assert np.array_equal(out[1], _oracle_decode(oracle, efs[1])), (hw, init)


# ---- 4. slow loop ----------------------------------------------------------------------------

def test_oversize_tile_takes_the_slow_loop(mh, oracle, device, bigbridge, cus):
    """[natural, long-span frame, natural] at 512 x 512: the first tile of frame 1 spans more than
    the LDS window and decodes in halves. Then the same three frames cycled over enough frames that
    G < 8: waves hold two tiles, and the wave that met the oversize tile finishes its later tile in
    the slow loop too."""
    w = h = 512
    nat, nat_efs = _crops(mh, bigbridge, w, h, 2)
    imgs = [nat[0], image_from_block_deltas(long_span_deltas(w, h), w, h), nat[1]]
    efs = [nat_efs[0], mh.encode_frame(imgs[1]), nat_efs[1]]
    assert (int(efs[1].block_offsets[64]) - int(efs[1].block_offsets[0])) // 8 > 4352
    want = [_oracle_decode(oracle, ef) for ef in efs]
    for f in range(3):
        assert np.array_equal(want[f], imgs[f])
    out, st = _decode_mixed(device, efs)
    assert st == [0, 0, 0]
    for f in range(3):
        assert np.array_equal(out[f], want[f]), f
    n = next(n for n in range(3, 4096) if _shape(device, w, h, n)[0] < 8)
    G, _ = _shape(device, w, h, n)
    assert _tiles(w, h) == 64 > 8 * G and n <= 8 * cus
    out, st = _decode_mixed(device, [efs[i % 3] for i in range(n)])
    assert not any(st)
    bad = [i for i in range(n) if not np.array_equal(out[i], want[i % 3])]
    assert not bad, bad[:8]


# ---- 5. multi-tile waves ---------------------------------------------------------------------

def test_multi_tile_waves_distinct_tables(mh, device, bigbridge, cus):
    """n frames of 1024 x 512 (128 tiles each) with distinct tables, n chosen from the device's
    launch shape so that 8 G < 128 < 16 G: some waves decode two tiles and some one (64 frames and
    G = 12 on 256 CUs). Compared on the device with the encoder inputs."""
    import torch
    from metalhuffman_amd import decoder as D
    w, h = 1024, 512
    tpf = _tiles(w, h)
    assert tpf == 128
    n = next(n for n in range(2, 1024) if 8 * _shape(device, w, h, n)[0] < tpf < 16 * _shape(device, w, h, n)[0])
    G, waves = _shape(device, w, h, n)
    assert tpf > waves * G and tpf % (waves * G) != 0 and n <= cus  # two tiles for some waves, one for others
    imgs, efs = _crops(mh, bigbridge, w, h, n)
    assert len({ef.canon.tobytes() for ef in efs}) > n // 2
    fr = D.DeviceFrames.pack(efs, device, shared_table=False)
    ts = D.DeviceTableSet.from_canonical_headers(np.stack([ef.canon for ef in efs]), device)
    out = D.decode_frames(fr, ts)
    ref = torch.from_numpy(np.stack(imgs)).to(device)
    torch.cuda.synchronize(device)
    assert not ts.status.any().item()
    bad = [i for i in range(n) if not torch.equal(out[i, :, :w], ref[i])]
    assert not bad, (n, G, bad[:8])


# ---- 6. table isolation ----------------------------------------------------------------------

def test_same_codes_different_tables(mh, oracle, device):
    """Two frames with the same code bytes and block offsets but different tables decode
    differently, each per its own table (oracle): the flat 8-bit identity table, and a table with
    64 seven-bit and 128 eight-bit codes (so every block still ends inside its 64 bytes). In both
    orders: a workgroup reading frame 0's table for every frame fails one of them."""
    from metalhuffman_amd import codec as C
    w = h = 256
    nb = (w // 8) * (h // 8)
    rng = np.random.default_rng(6)
    codes = np.concatenate([rng.integers(0, 256, nb * 64, dtype=np.uint8), np.zeros(mh.MH_CODES_PAD, np.uint8)])
    offs = (np.arange(nb, dtype=np.uint32) * 512).astype(np.uint32)
    ident = np.full(256, 8, np.uint8)
    mixed = np.zeros(256, np.uint8)
    mixed[:128] = 8
    mixed[192:] = 7
    fa = C.EncodedFrame(w, h, ident, codes, offs, None, 0)
    fb = C.EncodedFrame(w, h, mixed, codes, offs, None, 0)
    wa, wb = _oracle_decode(oracle, fa), _oracle_decode(oracle, fb)
    assert not np.array_equal(wa, wb)
    for order in ([fa, fb], [fb, fa], [fa, fb, fb, fa, fa]):
        out, st = _decode_mixed(device, order)
        assert not any(st)
        for i, ef in enumerate(order):
            assert np.array_equal(out[i], wa if ef is fa else wb), (len(order), i)


# ---- 7. a rejected header's zero table without a status array ---------------------------------

@pytest.mark.parametrize("flags", [0, 1])
def test_zero_table_without_status_is_zero_width(mh, oracle, device, flags):
    """d_frame_status NULL: a rejected header's table is all zero, every window is the reference's
    zero-width entry ({0,0}: nothing consumed, symbol 0), so every pixel is the block's init byte,
    0 -- what test_zero_width_windows_match_reference establishes for mh_decode. Code spans stay
    bounded by the descriptors as in mh_decode. The valid frame beside it is exact."""
    img = (np.arange(24 * 40, dtype=np.uint32) * 7 % 251).astype(np.uint8).reshape(24, 40)
    ef = mh.encode_frame(img, flags=flags)
    too_long = np.zeros(256, np.uint8)
    too_long[7] = 17
    zero_tables = (np.zeros(512, np.uint8), np.zeros(512, np.uint8))
    want = _oracle_decode(oracle, ef, zero_tables)
    assert not want.any()
    out, st = _decode_mixed(device, [ef, ef], skip_rejected=False, canons=[ef.canon, too_long])
    assert st == [0, -3]
    assert np.array_equal(out[0], img) and np.array_equal(out[0], _oracle_decode(oracle, ef))
    assert np.array_equal(out[1], want)
    out, _ = _decode_mixed(device, [ef, ef], skip_rejected=True, canons=[ef.canon, too_long])
    assert np.array_equal(out[0], img) and (out[1] == 0xA5).all()


# ---- 8. write containment --------------------------------------------------------------------

@pytest.mark.parametrize("skip", [None, 1])
def test_write_containment(mh, oracle, device, bigbridge, skip):
    """3 distinct-table frames of 93 x 37 into a caller's pitch (136), frame stride (rows + 40 bytes)
    and an 8-byte-aligned d_out between guards: only rows y < H and round_up(W, 8) bytes of each
    are written, and a skipped frame's region is wholly untouched."""
    import torch
    from metalhuffman_amd import _native as N
    from metalhuffman_amd import decoder as D
    W, H, n = 93, 37, 3
    imgs, efs = _crops(mh, bigbridge, W, H, n)
    assert len({ef.canon.tobytes() for ef in efs}) == n
    want = [_oracle_decode(oracle, ef) for ef in efs]
    pitch, w8 = 136, 96
    stride, lead = H * pitch + 40, 4096 + 8
    plan = containment_plan(n, W, H, pitch, stride, lead, 8 * pitch + 4096, written_cols=w8)
    buf = torch.from_numpy(plan.pattern.copy()).to(device)
    d_out = buf.data_ptr() + plan.d_out
    assert d_out % 16 == 8
    fr = D.DeviceFrames.pack(efs, device, shared_table=False)
    ts = D.DeviceTableSet.from_canonical_headers(np.stack([ef.canon for ef in efs]), device)
    if skip is not None:
        ts.status[skip] = -3
    st, _ = D._frames_entry(fr)
    N.check(N.lib().mh_decode_frames(ctypes.byref(st), ts.luts.data_ptr(), ts.stride, ts.status.data_ptr(), d_out,
                                     pitch, stride, torch.cuda.current_stream(device).cuda_stream), "mh_decode_frames")
    torch.cuda.synchronize(device)
    after = buf.cpu().numpy()
    if skip is not None:
        lo = plan.d_out + skip * stride
        assert np.array_equal(after[lo: lo + stride], plan.pattern[lo: lo + stride])
        want[skip] = plan.frame_view(plan.pattern, W)[skip]
    check_containment(after, plan, want)


# ---- 9. MH_FLAG_ANY_ORDER --------------------------------------------------------------------

def test_any_order_second_launch(mh, oracle, device, bigbridge):
    """Two decode_frames calls into distinct rasters on one stream, the second without the
    dispatch barrier: both exact."""
    import torch
    from metalhuffman_amd import _native as N
    from metalhuffman_amd import decoder as D
    w, h = 520, 264
    imgs, efs = _crops(mh, bigbridge, w, h, 6)
    sets = []
    for part in (efs[:3], efs[3:]):
        fr = D.DeviceFrames.pack(part, device, shared_table=False)
        sets.append((fr, D.DeviceTableSet.from_canonical_headers(np.stack([e.canon for e in part]), device)))
    outs = [torch.full((3, h, w), 0xA5, dtype=torch.uint8, device=device) for _ in sets]
    torch.cuda.synchronize(device)  # the tables are built: nothing in flight writes the second call's inputs
    D.decode_frames(sets[0][0], sets[0][1], out=outs[0])
    D.decode_frames(sets[1][0], sets[1][1], out=outs[1], extra_flags=N.MH_FLAG_ANY_ORDER)
    torch.cuda.synchronize(device)
    got = torch.cat(outs).cpu().numpy()
    for i, im in enumerate(imgs):
        assert np.array_equal(got[i], im), i
    assert np.array_equal(got[4], _oracle_decode(oracle, efs[4]))


def test_host_helpers(mh, device, bigbridge):
    """decode_frames_mixed (lists with different headers) and decode_frames' host form (the
    shared-table helper, unchanged)."""
    from metalhuffman_amd import decoder as D
    from metalhuffman_amd import frames as F
    imgs, efs = _crops(mh, bigbridge, 200, 120, 3)
    out = D.decode_frames_mixed(efs, device)
    assert out.shape == (3, 120, 200) and all(np.array_equal(out[i], imgs[i]) for i in range(3))
    base = np.ascontiguousarray(bigbridge[:128, :256])
    same = [base, F.block_shuffle(base, 3)]
    out = D.decode_frames([mh.encode_frame(im) for im in same], device)
    assert all(np.array_equal(out[i], same[i]) for i in range(2))
    with pytest.raises(ValueError, match="a batch shares one canonical table"):
        D.decode_frames(efs, device)
