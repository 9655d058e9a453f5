"""mh_decode_headers: a batch decoded straight from its canonical headers, every workgroup
building its frame's 13-bit table in LDS. The table is pinned byte for byte against
mh_build_luts_device (mh_header_luts_device copies it out); the decodes are compared with the
encoder inputs and the oracle's shader-semantics decode with each frame's own tables -- with
mh_decode_frames' raster only where the docstring says so. Every case is bit-exact.

The headers here are Huffman-optimal ones (and ten of them with a quarter of their lengths zeroed).
Valid headers that no Huffman construction emits -- all-long codes, random complete and incomplete
codes, the extremes of the escape range -- and the comparison of each builder's table with a plain
reference live in test_gpu_header_zoo.py; new header shapes go there, not here."""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import pytest

from helpers import (check_containment, containment_plan, fibonacci_deltas, image_from_block_deltas,
                     long_span_deltas)

pytestmark = pytest.mark.gpu

TABLE_BYTES = 18464          # the 13-bit table: the first bytes of a prepared table
LENGTHS_OFF = 18464 + 32768  # [longest, shortest, flat8, 0]


@pytest.fixture(scope="module")
def cus(device):
    import torch
    return torch.cuda.get_device_properties(device).multi_processor_count


def _oracle_decode(O, ef, tables=None):
    t1, t2 = tables if tables is not None else ef.tables()
    return O.decode_frame_shader(ef.block_offsets, ef.codes, t1, t2, ef.width, ef.height,
                                 block_init=ef.block_init, delta=not (ef.flags & 1))


def _shape(device, w, h, n, flags=0):
    """(workgroups per frame, waves per workgroup) of an n-frame w x h mh_decode_headers launch."""
    import torch
    from metalhuffman_amd import _native as N
    fr = N.mh_frame()
    fr.dims = N.mh_dims(w, h, (w + 7) // 8, (h + 7) // 8)
    fr.n_frames, fr.flags = n, flags
    g, wv = ctypes.c_uint32(), ctypes.c_uint32()
    N.check(N.lib().mh_decode_headers_shape(ctypes.byref(fr), torch.cuda.current_stream(device).cuda_stream,
                                            ctypes.byref(g), ctypes.byref(wv)), "mh_decode_headers_shape")
    assert wv.value == 8
    return int(g.value), int(wv.value)


def _tiles(w, h):
    return -(-(((w + 7) // 8) * ((h + 7) // 8)) // 64)


def _decode(device, efs, fill=0xA5, canons=None, frame_status=None, header_status=True, extra_flags=0):
    """efs through DeviceFrames.pack(shared_table=False) + decode_headers into a raster prefilled
    with `fill` -> (u8[n, H, W] on the host, header status list (77: not written) or None)."""
    import torch
    from metalhuffman_amd import decoder as D
    fr = D.DeviceFrames.pack(efs, device, shared_table=False)
    canons = np.stack([ef.canon for ef in efs] if canons is None else canons)
    out = torch.full((len(efs), fr.height, (fr.width + 7) // 8 * 8), fill, dtype=torch.uint8, device=device)
    hst = torch.full((len(efs),), 77, dtype=torch.int32, device=device) if header_status else None
    fst = torch.tensor(frame_status, dtype=torch.int32, device=device) if frame_status is not None else None
    got = D.decode_headers(fr, canons, out=out, frame_status=fst, header_status=hst, extra_flags=extra_flags)
    assert got is out
    torch.cuda.synchronize(device)
    return out[..., : fr.width].cpu().numpy(), (hst.cpu().tolist() if header_status else None)


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


def _code_lengths(freq):
    """(status, u8[256]) of mh_code_lengths."""
    from metalhuffman_amd import _native as N
    out = np.zeros(256, np.uint8)
    rc = N.lib().mh_code_lengths(np.ascontiguousarray(freq, np.uint64).ctypes.data_as(N._u64p),
                                 out.ctypes.data_as(N._u8p))
    return rc, out


def _too_long_header(n):
    """The 19-symbol Fibonacci histogram's lengths: deeper than 16 bits."""
    rc, h = _code_lengths(np.bincount(fibonacci_deltas(19, n, seed=2), minlength=256))
    assert rc == -3 and h.max() > 16 and int((h > 0).sum()) == 19
    return h


# ---- 1. the table, byte for byte -------------------------------------------------------------

def _six_headers(mh, bigbridge):
    from metalhuffman_amd import frames as F
    h = w = 256
    kraft = np.zeros(256, np.uint8)
    kraft[[1, 2, 3]] = 1  # three 1-bit codes: not a prefix code
    heads = [mh.encode_frame(np.ascontiguousarray(bigbridge[:h, 500:500 + w])).canon,
             mh.encode_frame(F.uniform_random(w, h, 5)).canon,
             mh.encode_frame(image_from_block_deltas(fibonacci_deltas(15, h * w, seed=4), w, h)).canon,
             mh.encode_frame(np.where(np.arange(h * w).reshape(h, w) % 3 == 0, 7, 0).astype(np.uint8),
                             flags=mh.MH_FLAG_NO_DELTA).canon,
             _too_long_header(h * w), kraft]
    assert (heads[1] == 8).all() and heads[2].max() == 14 and int((heads[3] > 0).sum()) == 2
    return heads, [0, 0, 0, 0, -3, -5]


def _random_complete_headers(seed=2024, trials=40):
    """Huffman code lengths of random heavy-tailed histograms over random alphabets; those
    mh_code_lengths rejects as deeper than 16 bits are passed over (seed 2024: 31 of 40 stay,
    longest codes from 1 to 16 bits, 14 of them with 16-bit codes)."""
    r = np.random.default_rng(seed)
    heads = []
    for k in range(trials):
        nsym = int(r.integers(2, 257))
        freq = np.zeros(256, np.uint64)
        syms = r.choice(256, nsym, replace=False)
        freq[syms] = (r.pareto(0.6 + 0.05 * (k % 8), nsym) * 50 + 1).astype(np.uint64)
        rc, h = _code_lengths(freq)
        if rc == 0:
            heads.append(h)
        else:
            assert rc == -3
    return heads


def test_table_bytes_match_build_luts(mh, device, bigbridge):
    """mh_header_luts_device (the decode kernel's builder, copied out) against mh_build_luts_device
    over the 18,464 table bytes and the lengths word, for: the six headers of the multitable test
    (statuses 0, 0, 0, 0, -3, -5), the single-symbol header, the 17-symbol Fibonacci header (15-
    and 16-bit codes: the lengths word's sampling rule), the accepted ones of 40 random complete
    codes (at least 30) and 10 incomplete codes made by zeroing random lengths of those. All in
    one launch, each alone (n = 1) and cycled over n = 70. Every other byte of a 0xA5-filled
    slot stays 0xA5."""
    import torch
    from metalhuffman_amd import _native as N
    six, six_status = _six_headers(mh, bigbridge)
    single = np.zeros(256, np.uint8)
    single[42] = 1
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    freq = np.zeros(256, np.uint64)
    freq[:17] = fib
    rc, fib17 = _code_lengths(freq)
    assert rc == 0 and fib17.max() == 16 and (fib17 == 15).any()
    rnd = _random_complete_headers()
    assert len(rnd) >= 30
    r = np.random.default_rng(7)
    incomplete = []
    for h in rnd[:10]:
        g = h.copy()
        used = np.flatnonzero(g)
        g[r.choice(used, max(1, used.size // 4), replace=False)] = 0
        incomplete.append(g)
    heads = six + [single, fib17] + rnd + incomplete
    want_status = six_status + [0] * (len(heads) - 6)
    lb = int(N.lib().mh_lut_bytes())
    assert lb == LENGTHS_OFF + 16
    stride = lb + 48
    stream = torch.cuda.current_stream(device).cuda_stream

    def both(idx):
        n = len(idx)
        hdr = torch.from_numpy(np.stack([heads[i] for i in idx])).to(device)
        out = []
        for fn in (N.lib().mh_build_luts_device, N.lib().mh_header_luts_device):
            luts = torch.full((n, stride), 0xA5, dtype=torch.uint8, device=device)
            status = torch.full((n,), 77, dtype=torch.int32, device=device)
            N.check(fn(hdr.data_ptr(), n, luts.data_ptr(), stride, status.data_ptr(), stream), "luts")
            torch.cuda.synchronize(device)
            out.append((luts.cpu().numpy(), status.cpu().tolist()))
        (ref, ref_st), (got, got_st) = out
        assert ref_st == [want_status[i] for i in idx] == got_st, idx
        for k, i in enumerate(idx):
            assert np.array_equal(got[k, :TABLE_BYTES], ref[k, :TABLE_BYTES]), (n, k, i)
            assert np.array_equal(got[k, LENGTHS_OFF:lb], ref[k, LENGTHS_OFF:lb]), \
                (n, k, i, got[k, LENGTHS_OFF:lb].view(np.uint32), ref[k, LENGTHS_OFF:lb].view(np.uint32))
        assert (got[:, TABLE_BYTES:LENGTHS_OFF] == 0xA5).all() and (got[:, lb:] == 0xA5).all(), n
        return got

    got = both(list(range(len(heads))))
    assert not got[4, :TABLE_BYTES].any() and not got[5, :TABLE_BYTES].any()  # rejected: zero tables
    for i in range(len(heads)):
        both([i])
    both([i % len(heads) for i in range(70)])


# ---- 2. mixed batch --------------------------------------------------------------------------

def _mixed_five(mh, bigbridge, raw):
    """The frames of the multitable test's mixed batch (256 x 256, 16 tiles); raw: the delta
    streams themselves as pixels, for MH_FLAG_NO_DELTA."""
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
def test_mixed_batch_headers_from_host_codec(mh, oracle, device, bigbridge, variant):
    """Five frames with unrelated histograms in one launch, headers straight from the host codec.
    The frame whose tree is deeper than 16 bits (delta and no-delta formats) has no codes: it
    goes in with its too-long lengths and another frame's codes, keeps its 0xA5 fill and reports
    -3; every other frame reports 0 and equals its input and the oracle's decode with its own
    tables. The launch mixes the step flavours listed below."""
    flags = mh.MH_FLAG_NO_DELTA if variant == "no_delta" else 0
    init = variant == "init_zero_delta"
    imgs = _mixed_five(mh, bigbridge, raw=bool(flags))
    efs, rejected = [], []
    for f, im in enumerate(imgs):
        try:
            efs.append(mh.encode_frame(im, flags=flags, init_zero_delta=init))
        except mh.MHError as e:
            assert e.status == -3
            efs.append(None)
            rejected.append(f)
    assert rejected == ([] if init else [3]), rejected
    flavours = {_flavour(e.canon) for e in efs if e is not None}
    assert flavours == {"delta": {"flat8", "general", "noesc"}, "init_zero_delta": {"general", "noesc"},
                        "no_delta": {"flat8", "flat", "general", "noesc"}}[variant], flavours
    for f in rejected:
        efs[f] = dataclasses.replace(efs[0], canon=_too_long_header(256 * 256))
    out, st = _decode(device, efs)
    assert st == [-3 if f in rejected else 0 for f in range(5)], st
    for f, im in enumerate(imgs):
        if f in rejected:
            assert (out[f] == 0xA5).all(), f
        else:
            assert np.array_equal(out[f], im), f
            assert np.array_equal(out[f], _oracle_decode(oracle, efs[f])), f


# ---- 3. shapes -------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [(1, 1), (9, 17), (72, 24), (512, 512), (1001, 777)])
def test_shapes_three_distinct_frames(mh, oracle, device, bigbridge, hw):
    """Partial tiles, block counts that are no multiple of 64, one-block frames, and frames whose
    tiles are fewer than or equal to (512 x 512: 64 tiles on 8 workgroups) 8 G waves' worth; with
    and without per-block init bytes."""
    h, w = hw
    G, _ = _shape(device, w, h, 3)
    tpf = _tiles(w, h)
    assert G == min(G, -(-tpf // 8)) and tpf <= 8 * G
    for init in (False, True):
        imgs, efs = _crops(mh, bigbridge, w, h, 3, init_zero_delta=init)
        if h * w >= 4096:
            assert len({ef.canon.tobytes() for ef in efs}) == 3
        out, st = _decode(device, efs)
        assert st == [0, 0, 0]
        for f, im in enumerate(imgs):
            assert np.array_equal(out[f], im), (hw, init, f)
        assert np.array_equal(out[1], _oracle_decode(oracle, efs[1])), (hw, init)


# ---- 4. oversize tile, multi-tile waves --------------------------------------------------------

def test_oversize_tile_takes_the_slow_loop(mh, oracle, device, bigbridge):
    """[natural, long-span frame, natural] at 512 x 512: the first tile of frame 1 spans more than
    the LDS window and decodes in halves, through the staging windows the builder used as scratch."""
    w = h = 512
    nat, nat_efs = _crops(mh, bigbridge, w, h, 2)
    imgs = [nat[0], image_from_block_deltas(long_span_deltas(w, h), w, h), nat[1]]
    efs = [nat_efs[0], mh.encode_frame(imgs[1]), nat_efs[1]]
    assert (int(efs[1].block_offsets[64]) - int(efs[1].block_offsets[0])) // 8 > 4352
    out, st = _decode(device, efs)
    assert st == [0, 0, 0]
    for f in range(3):
        assert np.array_equal(out[f], imgs[f]), f
        assert np.array_equal(out[f], _oracle_decode(oracle, efs[f])), f


def test_multi_tile_waves_distinct_headers(mh, device, bigbridge, cus):
    """n frames of 1024 x 512 (128 tiles each), n chosen from the device's launch shape so that
    8 G < 128 < 16 G: some waves decode two tiles and some one. Eight distinct headers, cycled;
    compared on the device with the encoder inputs."""
    import torch
    from metalhuffman_amd import decoder as D
    w, h = 1024, 512
    tpf = _tiles(w, h)
    assert tpf == 128
    n = next(n for n in range(2, 1024) if 8 * _shape(device, w, h, n)[0] < tpf < 16 * _shape(device, w, h, n)[0])
    G, waves = _shape(device, w, h, n)
    assert tpf > waves * G and tpf % (waves * G) != 0 and n <= cus
    imgs, efs = _crops(mh, bigbridge, w, h, 8)
    assert len({ef.canon.tobytes() for ef in efs}) == 8
    pick = [(5 * i) % 8 for i in range(n)]
    fr = D.DeviceFrames.pack([efs[i] for i in pick], device, shared_table=False)
    hst = torch.full((n,), 77, dtype=torch.int32, device=device)
    out = D.decode_headers(fr, np.stack([efs[i].canon for i in pick]), header_status=hst)
    ref = torch.from_numpy(np.stack(imgs)).to(device)
    torch.cuda.synchronize(device)
    assert not hst.any().item()
    bad = [i for i in range(n) if not torch.equal(out[i, :, :w], ref[pick[i]])]
    assert not bad, (n, G, bad[:8])


# ---- 5. header isolation ---------------------------------------------------------------------

def test_same_codes_different_headers(mh, oracle, device):
    """Two frames with the same code bytes and block offsets but different headers decode
    differently, each per its own header (oracle): the flat 8-bit identity code, and 64 seven-bit
    + 128 eight-bit codes (every block still ends inside its 64 bytes). In both orders: a
    workgroup that builds from frame 0's header for every frame fails one of them."""
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
        out, st = _decode(device, order)
        assert not any(st)
        for i, ef in enumerate(order):
            assert np.array_equal(out[i], wa if ef is fa else wb), (len(order), i)


# ---- 6. garbage code bytes ---------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, 1])
def test_garbage_codes_match_decode_frames(mh, device, bigbridge, flags):
    """Random code bytes under a natural header, the 14-bit Fibonacci header and an incomplete
    header (a quarter of the natural one's lengths zeroed: windows no code matches), 256 x 256,
    blocks 48 bytes apart: no fault, and the raster equals mh_decode_frames' raster for the same
    inputs byte for byte. The one deliberate GPU-to-GPU comparison: it walks escapes and
    zero-width windows that the table-bytes test pins statically."""
    import torch
    from metalhuffman_amd import codec as C
    from metalhuffman_amd import decoder as D
    w = h = 256
    nb = (w // 8) * (h // 8)
    rng = np.random.default_rng(11)
    codes = np.concatenate([rng.integers(0, 256, nb * 48 + 160, dtype=np.uint8), np.zeros(mh.MH_CODES_PAD, np.uint8)])
    offs = (np.arange(nb, dtype=np.uint32) * 384).astype(np.uint32)
    natural = mh.encode_frame(np.ascontiguousarray(bigbridge[:h, 500:500 + w])).canon
    fib14 = mh.encode_frame(image_from_block_deltas(fibonacci_deltas(15, h * w, seed=4), w, h)).canon
    assert fib14.max() == 14
    incomplete = natural.copy()
    used = np.flatnonzero(incomplete)
    incomplete[rng.choice(used, used.size // 4, replace=False)] = 0
    canons = [natural, fib14, incomplete]
    efs = [C.EncodedFrame(w, h, c, codes, offs, None, flags) for c in canons]
    out, st = _decode(device, efs)
    assert st == [0, 0, 0]
    fr = D.DeviceFrames.pack(efs, device, shared_table=False)
    ts = D.DeviceTableSet.from_canonical_headers(np.stack(canons), device)
    ref = torch.full((3, h, w), 0xA5, dtype=torch.uint8, device=device)
    D.decode_frames(fr, ts, out=ref)
    torch.cuda.synchronize(device)
    assert not ts.status.any().item()
    ref = ref.cpu().numpy()
    for f in range(3):
        assert np.array_equal(out[f], ref[f]), f
    assert len({out[f].tobytes() for f in range(3)}) == 3


# ---- 7. status arrays --------------------------------------------------------------------------

def test_frame_status_skip_and_rejected_header_without_status(mh, oracle, device, bigbridge):
    """d_frame_status: the skipped frame's raster and its header-status word are untouched (its
    header is not even looked at: it is a too-long one). Without either status array a rejected
    header's raster is still untouched, and the frames beside it are exact."""
    w, h = 200, 120
    imgs, efs = _crops(mh, bigbridge, w, h, 3)
    bad = _too_long_header(256 * 256)
    canons = [efs[0].canon, bad, efs[2].canon]
    out, st = _decode(device, efs, canons=canons, frame_status=[0, -3, 0])
    assert st == [0, 77, 0]
    assert np.array_equal(out[0], imgs[0]) and np.array_equal(out[2], imgs[2]) and (out[1] == 0xA5).all()
    assert np.array_equal(out[2], _oracle_decode(oracle, efs[2]))
    # a skipped frame with a valid header: still not decoded, word still not written
    out, st = _decode(device, efs, frame_status=[7, 0, 0])
    assert st == [77, 0, 0]
    assert (out[0] == 0xA5).all() and np.array_equal(out[1], imgs[1]) and np.array_equal(out[2], imgs[2])
    # no status arrays at all
    out, st = _decode(device, efs, canons=canons, header_status=False)
    assert st is None
    assert np.array_equal(out[0], imgs[0]) and np.array_equal(out[2], imgs[2]) and (out[1] == 0xA5).all()
    # header status only: the verdicts of mh_build_tables_device
    kraft = np.zeros(256, np.uint8)
    kraft[[1, 2, 3]] = 1
    out, st = _decode(device, efs, canons=[kraft, bad, efs[2].canon])
    assert st == [-5, -3, 0]
    assert (out[0] == 0xA5).all() and (out[1] == 0xA5).all() and np.array_equal(out[2], imgs[2])


# ---- 8. write containment ----------------------------------------------------------------------

@pytest.mark.parametrize("skip", [None, 1])
def test_write_containment(mh, oracle, device, bigbridge, skip):
    """3 distinct-header frames of 93 x 37 into a caller's pitch (136), an odd frame stride (rows +
    40 bytes) and an 8-byte-aligned d_out between guards: only rows y < H and round_up(W, 8) bytes
    of each are written, and a skipped frame's region is wholly untouched."""
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
    hdr = torch.from_numpy(np.stack([ef.canon for ef in efs])).to(device)
    fst = torch.zeros(n, dtype=torch.int32, device=device)
    hst = torch.full((n,), 77, dtype=torch.int32, device=device)
    if skip is not None:
        fst[skip] = -3
    st, _ = D._frames_entry(fr)
    N.check(N.lib().mh_decode_headers(ctypes.byref(st), hdr.data_ptr(), fst.data_ptr(), hst.data_ptr(), d_out,
                                      pitch, stride, torch.cuda.current_stream(device).cuda_stream),
            "mh_decode_headers")
    torch.cuda.synchronize(device)
    after = buf.cpu().numpy()
    assert hst.cpu().tolist() == [77 if f == skip else 0 for f in range(n)]
    if skip is not None:
        lo = plan.d_out + skip * stride
        assert np.array_equal(after[lo: lo + stride], plan.pattern[lo: lo + stride])
        want[skip] = plan.frame_view(plan.pattern, W)[skip]
    check_containment(after, plan, want)
