"""Batched GPU encode under ONE Huffman table (mh_encode_frames_shared_device_async): the
header built from the batch's summed histogram or supplied by the caller, every frame byte for
byte the host twin's (mh_encode_frame_with_header) and, where the batch is the reference's own
image, the reference encoder's (golden.json). Every call is made twice over one workspace, into
guard-filled outputs: a rejected frame, and the bytes around every output, stay untouched."""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np
import pytest

from helpers import fibonacci_deltas, golden, image_from_block_deltas

pytestmark = pytest.mark.gpu

OK, TOO_LONG, CAPACITY, TABLE = 0, -3, -4, -5
NO_DELTA, ZEROED, LIMIT = 0x1, 0x100, 0x200
FILL = 0xC3
GUARD = 256          # guard bytes in front of slot 0 and behind slot n - 1; guard words around the offsets
_u64p = ctypes.POINTER(ctypes.c_uint64)


def _run(mh, device, imgs, header=None, flags=0, init_zero=False, zeroed=True, ws_fill=None, alias=False,
         slot=None, copy_out=True):
    """Two calls over one workspace into fresh guard-filled outputs -> the second call's outputs on
    the host (the first call's must be identical). header: None (built mode) or u8[256]."""
    import torch
    L = mh.lib()
    n = len(imgs)
    h, w = imgs[0].shape
    nb = -(-w // 8) * -(-h // 8)
    slot = slot or (nb * 64 * 2 + 4 + 15) // 16 * 16 + 16
    wsb = int(L.mh_encode_frames_shared_workspace_bytes(w, h, n))
    ws = torch.zeros(wsb + 256, dtype=torch.uint8, device=device)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    al = (ws.data_ptr() + 255) // 256 * 256
    grays = torch.from_numpy(np.ascontiguousarray(np.stack(imgs))).to(device)
    results = []
    for _ in range(2):
        codes = torch.full((n * slot + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device=device)
        c0 = (codes.data_ptr() + 15) // 16 * 16 - codes.data_ptr() + GUARD
        offs = torch.full((n * nb + 2 * GUARD,), -0x3C3C3C3D, dtype=torch.int32, device=device)   # 0xC3C3C3C3
        init = torch.full((n * nb + 2 * GUARD,), FILL, dtype=torch.uint8, device=device) if init_zero else None
        canon = torch.full((256 + 2 * GUARD,), FILL, dtype=torch.uint8, device=device)
        lens = torch.full((n + 2,), -1, dtype=torch.int64, device=device)
        fco = torch.full((n + 3,), -1, dtype=torch.int64, device=device)
        st = torch.full((n + 2,), 0x5A5A5A5A, dtype=torch.int32, device=device)
        hst = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device=device)
        cin = None
        if header is not None:
            if alias:
                canon[GUARD:GUARD + 256] = torch.from_numpy(np.ascontiguousarray(header, np.uint8)).to(device)
                cin = canon.data_ptr() + GUARD
            else:
                cin_t = torch.from_numpy(np.ascontiguousarray(header, np.uint8)).to(device)
                cin = cin_t.data_ptr()
        rc = L.mh_encode_frames_shared_device_async(
            grays.data_ptr(), h * w, n, w, h, flags | (ZEROED if zeroed else 0), cin, canon.data_ptr() + GUARD,
            codes.data_ptr() + c0, slot, lens.data_ptr() + 8, fco.data_ptr() + 8, offs.data_ptr() + 4 * GUARD,
            init.data_ptr() + GUARD if init is not None else None, st.data_ptr() + 4, hst.data_ptr() + 4, al, wsb,
            ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
        assert rc == OK, rc
        torch.cuda.synchronize(device)
        r = dict(n=n, nb=nb, slot=slot, c0=c0, codes=codes.cpu().numpy(), offs=offs.cpu().numpy().view(np.uint32),
                 init=init.cpu().numpy() if init is not None else None, canon=canon.cpu().numpy(),
                 lens=lens.cpu().numpy(), fco=fco.cpu().numpy(), st=st.cpu().numpy(), hst=hst.cpu().numpy())
        # containment: the bytes around every output
        assert (r["codes"][:c0] == FILL).all() and (r["codes"][c0 + n * slot:] == FILL).all()
        assert (r["offs"][:GUARD] == 0xC3C3C3C3).all() and (r["offs"][GUARD + n * nb:] == 0xC3C3C3C3).all()
        if init is not None:
            assert (r["init"][:GUARD] == FILL).all() and (r["init"][GUARD + n * nb:] == FILL).all()
        assert (r["canon"][:GUARD] == FILL).all() and (r["canon"][GUARD + 256:] == FILL).all()
        assert r["lens"][0] == -1 and r["lens"][-1] == -1 and r["fco"][0] == -1 and r["fco"][-1] == -1
        assert r["st"][0] == 0x5A5A5A5A and r["st"][-1] == 0x5A5A5A5A
        assert r["hst"][0] == 0x5A5A5A5A and r["hst"][2] == 0x5A5A5A5A
        assert np.array_equal(r["fco"][1:-1], np.arange(n + 1) * slot)
        results.append(r)
    a, b = results
    for k in ("codes", "offs", "canon", "lens", "st", "hst"):
        assert np.array_equal(a[k], b[k]), f"the second call over the workspace differs in {k}"
    b["header"] = b["canon"][GUARD:GUARD + 256]
    b["status"] = b["st"][1:-1]
    b["header_status"] = int(b["hst"][1])
    b["codes_len"] = b["lens"][1:-1]
    return b


def _slot(r, f):
    return r["codes"][r["c0"] + f * r["slot"]: r["c0"] + (f + 1) * r["slot"]]


def _offsets(r, f):
    return r["offs"][GUARD + f * r["nb"]: GUARD + (f + 1) * r["nb"]]


def _check_frames(mh, r, imgs, header, flags=0, init_zero=False, rejected=None):
    """Accepted frames: the host twin's bytes under `header`, nothing behind the code words;
    rejected frames ({f: status}): status, codes_len 0, slot and offsets untouched."""
    rejected = rejected or {}
    for f, img in enumerate(imgs):
        if f in rejected:
            assert r["status"][f] == rejected[f], (f, r["status"][f])
            assert r["codes_len"][f] == 0
            assert (_slot(r, f) == FILL).all(), f
            assert (_offsets(r, f) == 0xC3C3C3C3).all(), f
            continue
        assert r["status"][f] == OK, (f, r["status"][f])
        ref = mh.encode_frame(img, flags=flags, init_zero_delta=init_zero, header=header)
        n = ref.codes.size
        assert r["codes_len"][f] == n, f
        assert np.array_equal(_slot(r, f)[:n], ref.codes), f
        assert (_slot(r, f)[(n + 3) // 4 * 4:] == FILL).all(), f
        assert np.array_equal(_offsets(r, f), ref.block_offsets), f
        if init_zero:
            assert np.array_equal(r["init"][GUARD + f * r["nb"]: GUARD + (f + 1) * r["nb"]], ref.block_init), f


def _mixed(bigbridge):
    from metalhuffman_amd import frames as F
    h = w = 256
    return [np.ascontiguousarray(bigbridge[:h, 500:500 + w]), F.uniform_random(w, h, 5),
            image_from_block_deltas(fibonacci_deltas(15, h * w, seed=4), w, h),
            np.where(np.arange(h * w).reshape(h, w) % 3 == 0, 7, 0).astype(np.uint8)]


def test_pinned_to_reference_encoder(mh, device, bigbridge):
    """BigBridge and its seed-7 block shuffle under the table built from both: doubling every
    count keeps the tree, so the header and each frame's bytes are the reference encoder's
    (golden.json). 6.3 M symbols: the tree takes its 64-bit key branch."""
    from metalhuffman_amd import frames as F
    g = golden()["workloads"]
    imgs = [bigbridge, F.block_shuffle(bigbridge, 7)]
    r = _run(mh, device, imgs)
    sha = lambda b: hashlib.sha256(np.ascontiguousarray(b).tobytes()).hexdigest()
    assert r["header_status"] == OK and (r["status"] == OK).all()
    assert sha(r["header"]) == g["bigbridge"]["canon_sha256"]
    for f, wl in enumerate(["bigbridge", "bigbridge_shuffle_seed7"]):
        n = int(r["codes_len"][f])
        assert sha(_slot(r, f)[:n]) == g[wl]["huffbuff_sha256"]
        assert sha(_offsets(r, f).astype("<u4")) == g[wl]["offsets_sha256"]


def test_mixed_histograms_built_and_supplied(mh, device, bigbridge):
    """Unrelated histograms under one built table: the header is the host's shared_header, every
    frame the host twin's; supplied mode with that header writes identical bytes, also with
    d_canon_header aliasing d_canon_in."""
    from metalhuffman_amd import codec
    imgs = _mixed(bigbridge)
    header = codec.shared_header(imgs)
    r = _run(mh, device, imgs)
    assert r["header_status"] == OK
    assert np.array_equal(r["header"], header)
    _check_frames(mh, r, imgs, header)
    for alias in (False, True):
        s = _run(mh, device, imgs, header=header, alias=alias)
        assert s["header_status"] == OK and np.array_equal(s["header"], header)
        for k in ("codes", "offs", "codes_len", "status"):
            assert np.array_equal(s[k], r[k]), (alias, k)


def test_supplied_header_without_one_frames_symbol(mh, device):
    """A header that lacks a symbol only frame 2 uses: frame 2 is rejected alone."""
    from metalhuffman_amd import codec
    h = w = 256
    d2 = fibonacci_deltas(12, h * w, seed=2)
    d2[np.flatnonzero(d2 == 3)[:5]] = 200
    imgs = [image_from_block_deltas(fibonacci_deltas(12, h * w, seed=1), w, h),
            np.where(np.arange(h * w).reshape(h, w) % 3 == 0, 7, 0).astype(np.uint8),
            image_from_block_deltas(d2, w, h),
            image_from_block_deltas(fibonacci_deltas(10, h * w, seed=3), w, h)]
    assert [int(codec.frame_histogram(im)[200]) for im in imgs] == [0, 0, 5, 0]
    header = codec.shared_header(imgs)
    assert header[200] > 0
    header[200] = 0
    r = _run(mh, device, imgs, header=header)
    assert r["header_status"] == OK
    _check_frames(mh, r, imgs, header, rejected={2: TABLE})


@pytest.mark.parametrize("kind,verdict", [("len17", TOO_LONG), ("kraft", TABLE)])
def test_supplied_header_rejected(mh, device, bigbridge, kind, verdict):
    from metalhuffman_amd import codec
    imgs = _mixed(bigbridge)[:3]
    header = codec.shared_header(imgs)            # complete, all 256 symbols (the random frame)
    if kind == "len17":
        header[5] = 17
    else:
        header[int(np.argmax(header))] -= 1       # a complete code with one code shortened: Kraft > 1
    r = _run(mh, device, imgs, header=header)
    assert r["header_status"] == verdict
    _check_frames(mh, r, imgs, header, rejected={f: verdict for f in range(3)})


def test_length_limiting(mh, device):
    """A summed tree deeper than 16: every frame -3 and nothing written without
    MH_ENCODE_LIMIT_LENGTHS; with it the header is mh_code_lengths_limited(sum, 16)."""
    from metalhuffman_amd import codec
    h = w = 256
    imgs = [image_from_block_deltas(fibonacci_deltas(19, h * w, seed=k), w, h) for k in (2, 3, 4)]
    freq = np.zeros(256, np.uint64)
    for im in imgs:
        freq += codec.frame_histogram(im)
    lens = np.zeros(256, np.uint8)
    assert mh.lib().mh_code_lengths(freq.ctypes.data_as(_u64p),
                                    lens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))) == TOO_LONG
    r = _run(mh, device, imgs)
    assert r["header_status"] == TOO_LONG
    _check_frames(mh, r, imgs, None, rejected={f: TOO_LONG for f in range(3)})
    r = _run(mh, device, imgs, flags=LIMIT)
    header = codec.code_lengths_limited(freq, 16)
    assert r["header_status"] == OK and np.array_equal(r["header"], header) and header.max() == 16
    _check_frames(mh, r, imgs, header)
    # supplied mode ignores the flag
    s = _run(mh, device, imgs, header=header, flags=LIMIT)
    assert np.array_equal(s["codes"], r["codes"]) and np.array_equal(s["offs"], r["offs"])


@pytest.mark.parametrize("hw", [(1, 1), (9, 17), (72, 24), (64, 776), (80, 48), (1040, 1032)])
def test_shapes_and_formats(mh, device, bigbridge, hw):
    """One block; partial edge blocks; every packer row loader (byte loads, one 8-byte load per
    block, one 16-byte load per block pair); tile counts off the packer's four waves; 66 tiles,
    one more than the 64-tile chunk of the offset scan. Also the init-byte and no-delta formats."""
    from metalhuffman_amd import codec
    from metalhuffman_amd import frames as F
    h, w = hw
    src = np.tile(bigbridge, (2, 2))
    imgs = [np.ascontiguousarray(F.block_shuffle(src, 11 + k)[:h, :w]) if h * w >= 64 else
            np.ascontiguousarray(src[k:k + h, :w]) for k in range(3)]
    for init_zero in (False, True):
        header = codec.shared_header(imgs, 0, init_zero)
        r = _run(mh, device, imgs, init_zero=init_zero)
        assert r["header_status"] == OK and np.array_equal(r["header"], header)
        _check_frames(mh, r, imgs, header, init_zero=init_zero)
    if h * w >= 4096:
        raw = [np.ascontiguousarray(fibonacci_deltas(12, h * w, seed=k).reshape(h, w)) for k in range(3)]
        header = codec.shared_header(raw, NO_DELTA)
        r = _run(mh, device, raw, flags=NO_DELTA)
        assert r["header_status"] == OK and np.array_equal(r["header"], header)
        _check_frames(mh, r, raw, header, flags=NO_DELTA)


def test_batch_total_past_2_22_symbols(mh, device, bigbridge):
    """4 x 1040 x 1032 with distinct content: 4,293,120 symbols in the batch (the tree's 64-bit
    keys), 1,073,280 in each frame (what the per-frame encoder sorts with 32-bit keys)."""
    from metalhuffman_amd import codec
    imgs = [np.ascontiguousarray(bigbridge[40 * k:40 * k + 1040, 200 * k:200 * k + 1032]) for k in range(4)]
    assert 4 * 130 * 129 * 64 > (1 << 22) - 1 > 130 * 129 * 64
    header = codec.shared_header(imgs)
    r = _run(mh, device, imgs)
    assert r["header_status"] == OK and np.array_equal(r["header"], header)
    _check_frames(mh, r, imgs, header)


def test_unzeroed_workspace(mh, device, bigbridge):
    """A workspace full of 0xA5 without MH_ENCODE_WORKSPACE_ZEROED, both modes."""
    from metalhuffman_amd import codec
    from metalhuffman_amd import frames as F
    imgs = [np.ascontiguousarray(F.block_shuffle(bigbridge, 50 + k)[:512, 100 * k:100 * k + 768]) for k in range(3)]
    header = codec.shared_header(imgs)
    r = _run(mh, device, imgs, zeroed=False, ws_fill=0xA5)
    assert r["header_status"] == OK and np.array_equal(r["header"], header)
    _check_frames(mh, r, imgs, header)
    s = _run(mh, device, imgs, header=header, zeroed=False, ws_fill=0xA5)
    assert s["header_status"] == OK
    _check_frames(mh, s, imgs, header)


def test_capacity_is_per_frame(mh, device, bigbridge):
    """A slot too small for the random frame alone: that frame is -4, the others exact."""
    from metalhuffman_amd import codec
    imgs = _mixed(bigbridge)
    header = codec.shared_header(imgs)
    sizes = [mh.encode_frame(im, header=header).codes.size for im in imgs]
    assert sizes[1] == max(sizes) and sorted(sizes)[-2] + 16 < sizes[1]
    slot = (sorted(sizes)[-2] + 15) // 16 * 16
    r = _run(mh, device, imgs, slot=slot)
    assert r["header_status"] == OK and np.array_equal(r["header"], header)
    _check_frames(mh, r, imgs, header, rejected={1: CAPACITY})


def test_python_surface(mh, device, bigbridge):
    """BatchEncoder.encode_shared_async: canon / header_status / status; decode() returns the
    inputs through decoder.decode with the one table; tables() builds it on the device;
    table_set() refuses; a rejected frame makes frames() and decode() raise."""
    import torch
    from metalhuffman_amd import codec
    from metalhuffman_amd import decoder as D
    from metalhuffman_amd.encoder import BatchEncoder
    imgs = _mixed(bigbridge)
    header = codec.shared_header(imgs)
    enc = BatchEncoder(256, 256, 4, device)
    grays = torch.from_numpy(np.stack(imgs)).to(device)
    a = enc.encode_shared_async(grays)
    assert a.shared and tuple(a.canon.shape) == (256,) and a.header_status.dtype == torch.int32
    out = a.decode()
    torch.cuda.synchronize(device)
    assert int(a.header_status.item()) == OK and not a.status.any()
    assert np.array_equal(a.canon.cpu().numpy(), header)
    assert torch.equal(out[..., :256], grays)
    assert a.shared_tables.check_status() > 0
    ref = mh.encode_frame(imgs[2], header=header)
    fr = a.frame(2)
    assert np.array_equal(fr.canon, header) and np.array_equal(fr.codes.cpu().numpy(), ref.codes)
    with pytest.raises(ValueError, match="tables"):
        a.table_set()
    # a supplied header (host array, then device tensor) gives the same bytes
    for hdr in (header, torch.from_numpy(header).to(device)):
        b = enc.encode_shared_async(grays, header=hdr)
        torch.cuda.synchronize(device)
        assert torch.equal(b.codes_len, a.codes_len) and torch.equal(b.block_offsets, a.block_offsets)
        t = b.tables()
        out = D.decode(b.frames(), t)
        torch.cuda.synchronize(device)
        assert torch.equal(out[..., :256], grays)
    # the per-frame methods are unchanged on the same encoder (one workspace for both)
    c = enc.encode_async(grays)
    with pytest.raises(ValueError, match="table_set"):
        c.tables()
    assert torch.equal(c.decode()[..., :256], grays)
    # a rejected frame: a header without a code for symbol 249, which only the two-symbol frame
    # (pixels 7, 0, 0, 7, ...: deltas 7, 249, 0) and the random frame use
    missing = header.copy()
    missing[249] = 0
    d = enc.encode_shared_async(grays, header=missing)
    torch.cuda.synchronize(device)
    assert int(d.header_status.item()) == OK
    assert d.status.cpu().tolist() == [0 if codec.frame_histogram(im)[249] == 0 else TABLE for im in imgs]
    assert d.status.cpu().tolist()[3] == TABLE
    with pytest.raises(mh.MHError):
        d.frames()
    with pytest.raises(mh.MHError):
        d.decode()
    assert d.frames(check=False).n_frames == 4
