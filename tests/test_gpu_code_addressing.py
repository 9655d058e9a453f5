"""Decode and encode at the 32-bit edges of code addressing.

The decode kernels address code bytes with u32 arithmetic: u32 bit offsets per block, a u32 frame
byte count clamped to 0xFFFFFFF0, u32 buffer offsets, a frame bit count that saturates at
0xFFFFFFFF past 512 MiB of codes. The contract allows values up to those limits; these tests go
there, always inside real allocations (no test declares a byte that is not allocated).

A. Block offsets high inside a frame (helpers.place_stream): `mid` straddles 2^31 inside tile 0,
   `top` puts the last block above 2^32 - 1024 (helpers.lead_top). 96x56 frames (84 blocks: tile 0
   full, tile 1 partial) of every step flavour through every decode entry and mh_check -- the
   entries that decode a part of each frame included: a region, windows and crops that hold the
   frame's last block, at full scale and reduced (SLICE_ROUTES) -- and one 8192x8192 frame under
   `top` through the pipelined loops.
B. Where frames lie and how big their slots are: a batch that starts at byte 4096, a batch beyond
   4 GiB, one frame declared with 0x20000000 / 0xFFFFFFE0 / 0xFFFFFFF0 bytes (0xFFFFFFF1 is
   refused), a batch whose slots exceed 4 GiB.
C. The GPU encoders at 2^32 code bits: 2^32 - 1024 bits encode (and decode back), 2^32 are refused
   and nothing is written.

The expected raster of every decode is the input image; for the small frames the oracle's shader
decode of the very stream under test must give it too. Every decode goes into a 0xA5-filled raster."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from helpers import (encode_with_header, exactly_uniform_image, frame_under_header, header_zoo, image_from_block_deltas,
                     lead_mid, lead_top, lead_top_bits, place_stream, placed_host_frame)

pytestmark = pytest.mark.gpu

W, H = 96, 56
NB = (W // 8) * (H // 8)
CLEAN = [0, 0, 0, 0xFFFFFFFF]
MH_ERR_CAPACITY = -4
MiB, GiB = 1 << 20, 1 << 30


@pytest.fixture(scope="module")
def cus(device):
    import torch
    return torch.cuda.get_device_properties(device).multi_processor_count


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    import torch
    torch.cuda.empty_cache()


def _need(device, nbytes):
    """The only skip of this file: less free device memory than the test allocates."""
    import torch
    free = torch.cuda.mem_get_info(device)[0]
    if free < nbytes + GiB:
        pytest.skip(f"{free >> 20} MiB of device memory free, the test needs {(nbytes + GiB) >> 20} MiB")


def _r16(x: int) -> int:
    return (x + 15) // 16 * 16


# ---- frames --------------------------------------------------------------------------------------

def _case_list():
    """(id, zoo header or None for the BigBridge header, format), one per step flavour."""
    zoo = header_zoo()
    by = {z.name: z for z in zoo}
    rnd = [z for z in zoo if z.kind == "random"]

    def shortest(z):
        return int(z.canon[z.canon > 0].min())

    noesc = next(z for z in rnd if z.longest == 13)
    flat = next(z for z in rnd if z.longest == shortest(z) and 4 <= z.longest <= 13)
    assert shortest(noesc) < 13
    return [("bigbridge", None, "delta"),                       # general step, 14-bit escapes
            (f"{noesc.name}-noesc", noesc, "delta"),            # escape-free
            (f"{flat.name}-flat", flat, "delta"),               # flat, swizzled stage
            ("8x256-flat8", by["8x256/a"], "delta"),            # uniform random bytes: the byte loop
            ("16x256", by["16x256/a"], "delta"),                # tile 0 oversize
            ("14x2", by["14x2/a"], "delta"),
            ("1x1", by["1x1/a"], "delta"),
            ("16x256-no_delta", by["16x256/a"], "no_delta"),
            ("16x256-init", by["16x256/a"], "init_zero_delta")]


CASES = _case_list()
PLACED = [(c, p) for c in CASES for p in (("mid", "top", "top_aligned") if c[0].startswith("16x256") else ("mid", "top"))]
PLACED_IDS = [f"{c[0]}-{p}" for c, p in PLACED]
ON_PLACED = pytest.mark.parametrize("case,placement", PLACED, ids=PLACED_IDS)
B_CASES = [c for c in CASES if c[0] in ("bigbridge", "8x256-flat8")]
ON_B = pytest.mark.parametrize("case", B_CASES, ids=[c[0] for c in B_CASES])
_FRAMES: dict = {}
_BB: dict = {}


def _bigbridge_header(mh, bigbridge):
    """The encoder's header of the whole BigBridge frame: all 256 symbols, longest code 14 bits."""
    if "canon" not in _BB:
        canon = mh.encode_frame(bigbridge).canon.copy()
        assert int(canon.max()) == 14 and (canon > 0).all()
        canon.setflags(write=False)
        _BB["canon"] = canon
    return _BB["canon"]


def _frames(mh, oracle, bigbridge, case):
    """Three frames under the case's header, built once: (canon, [(EncodedFrame, image)]). The
    image is also the oracle's shader decode of the stream."""
    name, z, fmt = case
    if name in _FRAMES:
        return _FRAMES[name]
    out = []
    if z is None:
        from metalhuffman_amd import codec as C
        canon = _bigbridge_header(mh, bigbridge)
        for y, x in ((700, 900), (1000, 300), (400, 1500)):
            img = np.ascontiguousarray(bigbridge[y: y + H, x: x + W])
            b = C.split_blocks(img).reshape(-1, 64).astype(np.int16)
            d = np.concatenate([b[:, :1], np.diff(b, axis=1)], axis=1).astype(np.uint8).reshape(-1)
            assert np.array_equal(image_from_block_deltas(d, W, H), img)
            out.append((encode_with_header(canon, d, W, H), img))
    else:
        canon = z.canon
        for k in range(3):
            out.append(frame_under_header(canon, W, H, seed=7000 + 10 * CASES.index(case) + k, no_delta=fmt == "no_delta",
                                          init_zero_delta=fmt == "init_zero_delta"))
    t1, t2 = oracle.split_tables(canon)
    for ef, img in out:
        got = oracle.decode_frame_shader(ef.block_offsets, ef.codes, t1, t2, W, H, block_init=ef.block_init,
                                         delta=fmt != "no_delta")
        assert np.array_equal(got, img), name
        assert oracle.check_frame(ef.block_offsets, ef.codes, t1, t2).tolist() == CLEAN, name
        img.setflags(write=False)
    if name.startswith("16x256") or name == "14x2":   # tile 0 leaves the staged path, tile 1 stays on it
        o = out[1][0].block_offsets.astype(np.int64)
        assert (o[64] - o[0]) // 8 > 4352 > (8 * out[1][0].payload_bytes - o[64]) // 8, name
    _FRAMES[name] = (canon, out)
    return _FRAMES[name]


def _lead(ef, placement):
    if placement == "mid":
        return lead_mid(ef)
    if placement == "top":
        return lead_top(ef)
    if placement == "top_aligned":
        return lead_top(ef, aligned=True)
    raise KeyError(placement)


def _placed(mh, oracle, bigbridge, case, placement):
    """(canon, frames, lead of frames[1] under the placement); the oracle's shader decode of the
    placed stream must be the image."""
    canon, frames = _frames(mh, oracle, bigbridge, case)
    ef, img = frames[1]
    lead = _lead(ef, placement)
    key = (case[0], placement)
    if key not in _FRAMES:
        pf = placed_host_frame(ef, lead)
        t1, t2 = oracle.split_tables(canon)
        got = oracle.decode_frame_shader(pf.block_offsets, pf.codes, t1, t2, W, H, block_init=pf.block_init,
                                         delta=case[2] != "no_delta")
        assert np.array_equal(got, img), key
        _FRAMES[key] = oracle.check_frame(pf.block_offsets, pf.codes, t1, t2).tolist()
        assert _FRAMES[key] == CLEAN, key
    return canon, frames, lead


def _pack(device, items, starts=None, end=None, alloc=None, uninitialised=False, garbage=None):
    """DeviceFrames built by hand: frame i = items[i] = (EncodedFrame, lead) placed (helpers.place_stream)
    at byte starts[i] of one device buffer. Default layout: back to back from 0, 16-byte aligned
    starts. alloc: the buffer's size (default `end`). uninitialised: torch.empty with only each
    frame's neighbourhood zeroed (for buffers of several GiB); garbage = (lo, hi): those bytes 0xFF.
    One frame at byte 0 gets no offset array, so codes_bytes is the buffer's size."""
    import torch
    from metalhuffman_amd import decoder as D
    n = len(items)
    if starts is None:
        starts, pos = [], 0
        for ef, lead in items:
            starts.append(pos)
            pos += lead + ef.codes.size if n == 1 else _r16(lead + ef.codes.size)
        end = pos
    size = alloc if alloc is not None else end
    assert all(s % 16 == 0 for s in starts) and end <= size
    codes = (torch.empty if uninitialised else torch.zeros)(size, dtype=torch.uint8, device=device)
    assert codes.data_ptr() % 16 == 0
    offs = []
    for (ef, lead), s in zip(items, starts):
        payload, o, total = place_stream(ef, lead)
        assert s + total <= end
        if uninitialised:
            assert lead == 0
            codes[s: min(size, s + _r16(total) + 8192)].zero_()
        codes[s + lead: s + total] = torch.from_numpy(payload).to(device)
        offs.append(o)
    if garbage is not None:
        codes[garbage[0]: garbage[1]].fill_(0xFF)
    ef0 = items[0][0]
    init = None
    if ef0.block_init is not None:
        init = torch.from_numpy(np.concatenate([ef.block_init for ef, _ in items])).to(device)
    fco = None
    if n > 1 or starts[0] != 0:
        fco = torch.tensor(list(starts) + [end], dtype=torch.int64, device=device)
    return D.DeviceFrames(W, H, n, torch.from_numpy(np.concatenate(offs).view(np.int32)).to(device), codes, fco, init,
                          ef0.flags, sum(ef.payload_bytes for ef, _ in items))


def _expect(out, wants, what):
    got = out[..., :W].cpu().numpy()
    n = len(wants)
    assert got.shape == (n, H, W)
    want = np.stack(wants)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).reshape(n, -1).any(axis=1))
        f = int(bad[0])
        ys, xs = np.nonzero(got[f] != want[f])
        blocks = np.unique((ys // 8) * (W // 8) + xs // 8)
        raise AssertionError(f"{what}: {bad.size} of {n} frame(s) wrong, first frame {f}: {ys.size} wrong pixel(s) in "
                             f"{blocks.size} block(s) {int(blocks[0])}..{int(blocks[-1])}, first at row {int(ys[0])}, "
                             f"column {int(xs[0])}: {int(got[f, ys[0], xs[0]]):#04x}, expected "
                             f"{int(want[f, ys[0], xs[0]]):#04x}")


ROUTES3 = ("small", "inkernel", "frames", "headers", "check")
ROUTES1 = ("frame", "inkernel", "frames", "headers", "check")
# the entries that decode a part of each frame (slice_decode's region, windows and crop tiles); the
# region, the first window and the first crop all hold the frame's last block, whose end bit wraps
# under `top`
SLICE_ROUTES = ("region", "region_scaled", "windows", "windows_scaled", "crops")
SLICE_REGION = (1, 1, 11, 6)
SLICE_WINDOWS = ((10, 3), ((2, 4), (0, 0)))
SLICE_CROPS = ((83, 21), ((13, 35), (3, 2)))
SLICE_K = {"region_scaled": 1, "windows_scaled": 2}


def _slice_route(device, route, fr, canon, wants, what):
    """One launch of a part-of-frame entry over `fr` into 0xA5-filled rasters, every pixel compared
    with the slice of `wants` (box-reduced at a scale, zeros beyond the picture). The region routes
    take one shared table and the rest a table per frame, so hdr_resolve sees both."""
    import torch
    from metalhuffman_amd import decoder as D
    from scaled_helpers import box_reduce_np
    n, k = fr.n_frames, SLICE_K.get(route, 0)
    c = 8 >> k
    assert SLICE_REGION[0] + SLICE_REGION[2] == W // 8 and SLICE_REGION[1] + SLICE_REGION[3] == H // 8
    assert SLICE_WINDOWS[1][0][0] + 10 == W // 8 and SLICE_WINDOWS[1][0][1] + 3 == H // 8
    assert SLICE_CROPS[1][0][0] + 83 == W and SLICE_CROPS[1][0][1] + 21 == H
    if route in ("region", "region_scaled"):
        tabs = D.DeviceTables.from_canonical_header(np.array(canon, np.uint8), device)   # (canon is read-only)
        assert tabs.check_status() >= 0 and tabs.lut is not None
        ts = None
    else:
        tabs = ts = D.DeviceTableSet.from_canonical_headers(np.stack([canon] * n), device)

    def full(slots, rows, cols):
        return torch.full((slots, rows, cols), 0xA5, dtype=torch.uint8, device=device)

    if route in ("region", "region_scaled"):
        bx0, by0, bw, bh = SLICE_REGION
        rects = [(f, 8 * bx0, 8 * by0, 8 * bw, 8 * bh) for f in range(n)]
        out = full(n, bh * c, bw * c)
        if k:
            assert D.decode_region_scaled(fr, tabs, D.Region(*SLICE_REGION), k, out=out) is out
        else:
            assert D.decode_region(fr, tabs, D.Region(*SLICE_REGION), out=out) is out
    elif route in ("windows", "windows_scaled"):
        (bw, bh), origins = SLICE_WINDOWS
        wins = [(f, bx0, by0) for f in range(n) for bx0, by0 in origins]
        rects = [(f, 8 * bx0, 8 * by0, 8 * bw, 8 * bh) for f, bx0, by0 in wins]
        out = full(len(wins), bh * c, bw * c)
        if k:
            got, st = D.decode_windows_scaled(fr, tabs, wins, (bw, bh), k, out=out, status=True)
        else:
            got, st = D.decode_windows(fr, tabs, wins, (bw, bh), out=out, status=True)
        assert got is out
    elif route == "crops":
        (w, h), origins = SLICE_CROPS
        crops = [(f, x0, y0) for f in range(n) for x0, y0 in origins]
        rects = [(f, x0, y0, w, h) for f, x0, y0 in crops]
        out = full(len(crops), h, (w + 7) // 8 * 8)
        got, st = D.decode_crops(fr, tabs, crops, (w, h), out=out, status=True)
        assert got is out
    else:
        raise KeyError(route)
    torch.cuda.synchronize(device)
    if ts is not None:
        assert not ts.status.any().item() and not st.any().item(), what
    got = out.cpu().numpy()
    for p, (f, x0, y0, w, h) in enumerate(rects):
        want = np.ascontiguousarray(wants[f][y0: y0 + h, x0: x0 + w])
        if k:
            want = box_reduce_np(want, k)
        sh, sw = want.shape
        if not np.array_equal(got[p, :sh, :sw], want):
            ys, xs = np.nonzero(got[p, :sh, :sw] != want)
            raise AssertionError(f"{what}: raster {p} (frame {f}, {w} x {h} at ({x0}, {y0}), k {k}): {ys.size} wrong "
                                 f"pixel(s), first at row {int(ys[0])}, column {int(xs[0])}: "
                                 f"{int(got[p, ys[0], xs[0]]):#04x}, expected {int(want[ys[0], xs[0]]):#04x}")
        if k:
            assert not got[p, :sh, sw:].any(), f"{what}: raster {p}: columns beyond the picture are not 0"


def _route(mh, oracle, device, cus, route, fr, canon, wants, what):
    """One decode entry over `fr` into a 0xA5-filled raster, every pixel compared; "check": mh_check,
    clean. The launch each route must take (launch() in mh_decode.hip) is asserted."""
    import torch
    from metalhuffman_amd import decoder as D
    n = fr.n_frames
    tiles = -(-NB // 64) * n
    what = f"{what}, {route}"
    if route in SLICE_ROUTES:
        return _slice_route(device, route, fr, canon, wants, what)
    out = torch.full((n, H, W), 0xA5, dtype=torch.uint8, device=device)
    if route in ("frame", "small", "large", "inkernel", "check"):
        t1, t2 = mh.Huffman.generateSplitLookupTables(canon)
        tabs = D.DeviceTables.upload(t1, t2, device, prepare_lut=route != "inkernel")
        if route == "frame":      # mh_decode_frame_kernel
            assert n == 1 and fr.frame_code_offsets is None and tiles <= 4 * cus
        elif route == "small":    # mh_decode_small_kernel
            assert fr.frame_code_offsets is not None and tiles <= 4 * cus
        elif route == "large":    # mh_decode_kernel with the prepared table
            assert tiles > 4 * cus and -(-tiles // cus) >= 5
        elif route == "inkernel":  # mh_decode_kernel building its table
            assert tabs.lut is None
        if route == "check":
            rep = D.check(fr, tabs).cpu().tolist()
            assert rep == [CLEAN] * n, (what, rep)
            return
        assert D.decode(fr, tabs, out=out) is out
    elif route == "frames":
        ts = D.DeviceTableSet.from_canonical_headers(np.stack([canon] * n), device)
        assert D.decode_frames(fr, ts, out=out) is out
        torch.cuda.synchronize(device)
        assert not ts.status.any().item(), what
    elif route == "headers":
        hst = torch.full((n,), 77, dtype=torch.int32, device=device)
        assert D.decode_headers(fr, np.stack([canon] * n), out=out, header_status=hst) is out
        torch.cuda.synchronize(device)
        assert not hst.any().item(), what
    else:
        raise KeyError(route)
    torch.cuda.synchronize(device)
    _expect(out, wants, what)


# ---- A. high bit offsets inside a frame ------------------------------------------------------------

@ON_PLACED
def test_one_placed_frame(mh, oracle, device, cus, bigbridge, case, placement):
    """One frame, its codes at the end of a buffer of 256 / 512 MiB: mh_decode with a prepared table
    (mh_decode_frame_kernel) and without (mh_decode_kernel, one frame), mh_decode_frames and
    mh_decode_headers with n = 1, mh_check, and the part-of-frame entries (SLICE_ROUTES)."""
    canon, frames, lead = _placed(mh, oracle, bigbridge, case, placement)
    _need(device, lead)
    fr = _pack(device, [(frames[1][0], lead)])
    assert fr.codes.numel() == lead + frames[1][0].codes.size and fr.frame_code_offsets is None
    for route in ROUTES1 + SLICE_ROUTES:
        _route(mh, oracle, device, cus, route, fr, canon, [frames[1][1]], f"{case[0]} {placement}")
    del fr


@ON_PLACED
def test_three_frames_the_middle_one_placed(mh, oracle, device, cus, bigbridge, case, placement):
    """Three frames with an offset array, frame 1 the placed one, frames 0 and 2 ordinary:
    mh_decode_small_kernel, mh_decode_kernel with its own table, mh_decode_frames,
    mh_decode_headers, mh_check, and the part-of-frame entries (SLICE_ROUTES)."""
    canon, frames, lead = _placed(mh, oracle, bigbridge, case, placement)
    _need(device, lead)
    fr = _pack(device, [(frames[0][0], 0), (frames[1][0], lead), (frames[2][0], 0)])
    for route in ROUTES3 + SLICE_ROUTES:
        _route(mh, oracle, device, cus, route, fr, canon, [f[1] for f in frames], f"{case[0]} {placement}")
    del fr


@ON_PLACED
def test_large_batch_two_frames_placed(mh, oracle, device, cus, bigbridge, case, placement):
    """4 x CUs // 2 + 1 frames (more than 4 x CUs tiles: mh_decode_kernel with the prepared table,
    the flavour from its lengths word), the last frame and a middle one placed, the rest ordinary."""
    canon, frames, lead = _placed(mh, oracle, bigbridge, case, placement)
    _need(device, 2 * lead)
    n = 4 * cus // 2 + 1
    placed = (n // 2, n - 1)
    items, wants = [], []
    for i in range(n):
        k = 1 if i in placed else (0, 2)[i % 2]
        items.append((frames[k][0], lead if i in placed else 0))
        wants.append(frames[k][1])
    fr = _pack(device, items)
    _route(mh, oracle, device, cus, "large", fr, canon, wants, f"{case[0]} {placement}")
    del fr


def test_pipelined_loops_under_top(mh, device, cus, bigbridge):
    """One 8192x8192 mirror-tile frame whose last block starts above 2^32 - 1024: 16,384 tiles,
    several per wave, through the software-pipelined loops of mh_decode_kernel (prepared table),
    mh_decode_multitable_kernel and mh_decode_headers_kernel. Encoded on the device (the expected
    raster is the image, whatever produced the codes), compared on the device."""
    import torch
    from metalhuffman_amd import decoder as D, encoder as E, frames as F
    S = 8192
    _need(device, 2 * GiB)
    img = torch.from_numpy(F.mirror_tile(bigbridge, S, S)).to(device)
    enc = E.Encoder(S, S, device).encode(img)
    nb = (S // 8) ** 2
    n = int(enc.codes.numel())
    offs = enc.block_offsets.to(torch.int64) & 0xFFFFFFFF
    lead = lead_top_bits(int(offs[-1].item()), 8 * (n - 4))
    assert lead % 16 and 2 ** 32 - 1024 < 8 * lead + int(offs[-1].item()) < 2 ** 32
    codes = torch.zeros(lead + n, dtype=torch.uint8, device=device)
    codes[lead:] = enc.codes
    moved = offs + 8 * lead
    moved = torch.where(moved >= 2 ** 31, moved - 2 ** 32, moved).to(torch.int32)   # the u32's bits
    fr = D.DeviceFrames(S, S, 1, moved, codes, None, None, 0, n - 4)
    tiles = nb // 64
    g, w = D.decode_frames_shape(fr)
    assert tiles == 16384 and tiles > 4 * cus and g * w < tiles, (g, w)   # a wave gets more than one tile
    g, w = D.decode_headers_shape(fr)
    assert g * w < tiles, (g, w)
    canon = torch.from_numpy(enc.canon.copy()).to(device)[None]
    tabs = D.DeviceTables.from_canonical_header(canon[0], device)
    assert tabs.check_status() >= 256 and tabs.lut is not None

    def run(what, fn):
        out = torch.full((1, S, S), 0xA5, dtype=torch.uint8, device=device)
        fn(out)
        torch.cuda.synchronize(device)
        if not torch.equal(out[0], img):
            ys, xs = torch.nonzero(out[0] != img, as_tuple=True)
            blocks = torch.unique((ys // 8) * (S // 8) + xs // 8)
            raise AssertionError(f"{what}: {ys.numel()} wrong pixel(s) in {blocks.numel()} block(s) "
                                 f"{int(blocks[0])}..{int(blocks[-1])} of {nb}, first at row {int(ys[0])}, column {int(xs[0])}")

    run("mh_decode, prepared table", lambda out: D.decode(fr, tabs, out=out))
    ts = D.DeviceTableSet.from_canonical_headers(canon, device)
    run("mh_decode_frames", lambda out: D.decode_frames(fr, ts, out=out))
    assert ts.status.cpu().tolist() == [0]
    hst = torch.full((1,), 77, dtype=torch.int32, device=device)
    run("mh_decode_headers", lambda out: D.decode_headers(fr, canon, out=out, header_status=hst))
    assert hst.cpu().tolist() == [0]
    del fr, codes, img, enc


# ---- B. where frames lie and how big their slots are -----------------------------------------------

@ON_B
def test_batch_that_starts_at_byte_4096(mh, oracle, device, cus, bigbridge, case):
    """frame_code_offsets[0] != 0: three frames back to back from byte 4096 of the buffer."""
    canon, frames = _frames(mh, oracle, bigbridge, case)
    starts, pos = [], 4096
    for ef, _ in frames:
        starts.append(pos)
        pos += _r16(ef.codes.size)
    fr = _pack(device, [(ef, 0) for ef, _ in frames], starts=starts, end=pos, garbage=(0, 4096))
    assert fr.frame_code_offsets.cpu().tolist() == starts + [pos]
    for route in ROUTES3:
        _route(mh, oracle, device, cus, route, fr, canon, [f[1] for f in frames], f"{case[0]} from byte 4096")


@ON_B
def test_batch_beyond_4_gib(mh, oracle, device, cus, bigbridge, case):
    """Three frames back to back from byte 2^32 + 32 of one 4 GiB + 1 MiB buffer, slots of ordinary
    size: the 64-bit frame offsets."""
    canon, frames = _frames(mh, oracle, bigbridge, case)
    size = 2 ** 32 + MiB
    _need(device, size)
    starts, pos = [], 2 ** 32 + 32
    for ef, _ in frames:
        starts.append(pos)
        pos += _r16(ef.codes.size)
    fr = _pack(device, [(ef, 0) for ef, _ in frames], starts=starts, end=pos, alloc=size, uninitialised=True)
    for route in ROUTES3:
        _route(mh, oracle, device, cus, route, fr, canon, [f[1] for f in frames], f"{case[0]} beyond 4 GiB")
    del fr


@ON_B
@pytest.mark.parametrize("size", [0x20000000, 0xFFFFFFE0, 0xFFFFFFF0], ids=hex)
def test_one_frame_declared_with_a_clamp_size(mh, oracle, device, cus, bigbridge, case, size):
    """One frame at the front of a real allocation of `size` bytes, codes_bytes = size: 0x20000000
    (the first value at which the frame's bit count saturates), 0xFFFFFFE0, and 0xFFFFFFF0, the
    accepted maximum, where the u32 sum size + 16 wraps."""
    canon, frames = _frames(mh, oracle, bigbridge, case)
    _need(device, size)
    fr = _pack(device, [(frames[1][0], 0)], alloc=size, uninitialised=True)
    assert fr.codes.numel() == size and fr.frame_code_offsets is None
    for route in ROUTES1:
        _route(mh, oracle, device, cus, route, fr, canon, [frames[1][1]], f"{case[0]} codes_bytes {size:#x}")
    del fr


def test_one_byte_over_the_maximum_is_refused(mh, oracle, device, cus, bigbridge):
    """codes_bytes = 0xFFFFFFF1 (allocated): MH_ERR_CAPACITY, nothing launched -- the raster keeps
    its fill."""
    import torch
    from metalhuffman_amd import decoder as D
    canon, frames = _frames(mh, oracle, bigbridge, B_CASES[0])
    size = 0xFFFFFFF1
    _need(device, size)
    fr = _pack(device, [(frames[1][0], 0)], alloc=size, uninitialised=True)
    t1, t2 = mh.Huffman.generateSplitLookupTables(canon)
    tabs = D.DeviceTables.upload(t1, t2, device)
    out = torch.full((1, H, W), 0xA5, dtype=torch.uint8, device=device)
    with pytest.raises(mh.MHError) as e:
        D.decode(fr, tabs, out=out)
    assert e.value.status == MH_ERR_CAPACITY
    torch.cuda.synchronize(device)
    assert bool((out == 0xA5).all())
    del fr


@ON_B
def test_batch_with_slots_over_4_gib(mh, oracle, device, cus, bigbridge, case):
    """offsets [0, 2^32 + 64, 2^33 + 128, 2^33 + 128 + small]: the slots of frames 0 and 1 exceed
    4 GiB (treated as 0xFFFFFFF0 bytes), frame 2 is ordinary; one allocation holds them all."""
    canon, frames = _frames(mh, oracle, bigbridge, case)
    small = _r16(frames[2][0].codes.size)
    starts = [0, 2 ** 32 + 64, 2 ** 33 + 128]
    end = starts[2] + small
    _need(device, end)
    fr = _pack(device, [(ef, 0) for ef, _ in frames], starts=starts, end=end, uninitialised=True)
    assert fr.codes.numel() == end
    for route in ROUTES3:
        _route(mh, oracle, device, cus, route, fr, canon, [f[1] for f in frames], f"{case[0]} slots over 4 GiB")
    del fr


def test_idle_lanes_read_inside_a_maximal_frame(mh, oracle, device, cus, bigbridge):
    """The flat 8-bit frame declared with 0xFFFFFFF0 bytes, the buffer's last 4 KiB 0xFF: the byte
    loop's lanes without a block (tile 1 holds 20 blocks) load at 0xFFFFFF00, which is now inside
    the frame; what they load must not reach the raster."""
    canon, frames = _frames(mh, oracle, bigbridge, B_CASES[1])
    size = 0xFFFFFFF0
    _need(device, size)
    fr = _pack(device, [(frames[1][0], 0)], alloc=size, uninitialised=True, garbage=(size - 4096, size))
    for route in ("frame", "inkernel", "frames", "headers"):
        _route(mh, oracle, device, cus, route, fr, canon, [frames[1][1]], "flat8, codes_bytes 0xfffffff0")
    del fr


# ---- C. the GPU encoders at 2^32 bits --------------------------------------------------------------

PASS_W, PASS_H = 32784, 16376      # 4098 x 2047 blocks, 2^29 - 128 pixels: 2^32 - 1024 code bits at 8 bits each
FAIL_W, FAIL_H = 32768, 16384      # 2^29 pixels: exactly 2^32 code bits


def _histogram_lengths(img):
    """mh_code_lengths of the image's histogram (host tree builder) -> (status, u8[256])."""
    import torch
    from metalhuffman_amd import _native as N
    flat = img.reshape(-1)
    counts = torch.zeros(256, dtype=torch.int64, device=img.device)
    for lo in range(0, flat.numel(), 1 << 26):
        counts += torch.bincount(flat[lo: lo + (1 << 26)].to(torch.int32), minlength=256)
    freq = counts.cpu().numpy().astype(np.uint64)
    canon = np.zeros(256, np.uint8)
    rc = N.lib().mh_code_lengths(freq.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                 canon.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    return rc, canon


def _block_order(img):
    h, w = img.shape
    return img.view(h // 8, 8, w // 8, 8).permute(0, 2, 1, 3).reshape(-1)


def _check_flat8_encoding(img, canon, codes, codes_len, offsets):
    """The no-delta encoding of an exactly uniform image: all lengths 8 (the histogram's Huffman
    lengths), codes_len = pixels + 4, offsets 512 b, the codes are the pixels in block order."""
    import torch
    px = img.numel()
    rc, want = _histogram_lengths(img)
    assert rc == 0 and (want == 8).all()
    assert np.array_equal(canon.cpu().numpy(), want)
    assert codes_len == px + 4
    o = offsets.to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(o, 512 * torch.arange(px // 64, dtype=torch.int64, device=img.device))
    assert int(o[-1]) == 2 ** 32 - 1024 - 512
    assert torch.equal(codes[:px], _block_order(img))
    assert not codes[px: px + 4].any().item()


def _same(out, img, what):
    import torch
    assert torch.equal(out, img), what


def test_encoder_accepts_2_pow_32_minus_1024_bits(mh, device):
    """Encoder.encode_async of the 2^32 - 1024 bit frame: status 0 and the exact encoding; decoded
    back by mh_decode (device-built table) and mh_decode_headers -- the byte loop with block offsets
    up to 2^32 - 1536."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D, encoder as E
    _need(device, 5 * GiB)
    img = exactly_uniform_image(PASS_W, PASS_H, seed=31, device=device)
    assert img.numel() == 2 ** 29 - 128
    enc = E.Encoder(PASS_W, PASS_H, device)
    a = enc.encode_async(img, flags=N.MH_FLAG_NO_DELTA)
    torch.cuda.synchronize(device)
    assert int(a.status.item()) == 0
    _check_flat8_encoding(img, a.canon, a.codes, int(a.codes_len.item()), a.block_offsets)
    fr = a.frames()
    tabs = a.tables()
    out = torch.full((1, PASS_H, PASS_W), 0xA5, dtype=torch.uint8, device=device)
    D.decode(fr, tabs, out=out)
    torch.cuda.synchronize(device)
    assert tabs.check_status() >= 256
    _same(out[0], img, "mh_decode")
    out.fill_(0xA5)
    hst = torch.full((1,), 77, dtype=torch.int32, device=device)
    D.decode_headers(fr, a.canon[None], out=out, header_status=hst)
    torch.cuda.synchronize(device)
    assert hst.cpu().tolist() == [0]
    _same(out[0], img, "mh_decode_headers")
    del out, fr, a, enc, img


def test_batch_encoder_accepts_2_pow_32_minus_1024_bits(mh, device):
    """BatchEncoder, n = 2: frame 0 the 2^32 - 1024 bit frame, frame 1 a constant image (one 1-bit
    code). Frame 0's exact encoding; both decoded back with a table per frame."""
    import torch
    from metalhuffman_amd import _native as N, encoder as E
    _need(device, 8 * GiB)
    grays = torch.empty((2, PASS_H, PASS_W), dtype=torch.uint8, device=device)
    grays[0] = exactly_uniform_image(PASS_W, PASS_H, seed=32, device=device)
    grays[1].fill_(0x5C)
    b = E.BatchEncoder(PASS_W, PASS_H, 2, device).encode_async(grays, flags=N.MH_FLAG_NO_DELTA)
    torch.cuda.synchronize(device)
    assert b.status.cpu().tolist() == [0, 0]
    nb = (PASS_W // 8) * (PASS_H // 8)
    assert b.frame_code_offsets.cpu().tolist() == [0, b.slot, 2 * b.slot]
    _check_flat8_encoding(grays[0], b.canon[0], b.codes[: b.slot], int(b.codes_len[0].item()), b.block_offsets[:nb])
    want1 = np.zeros(256, np.uint8)
    want1[0x5C] = 1
    assert np.array_equal(b.canon[1].cpu().numpy(), want1)
    assert int(b.codes_len[1].item()) == grays[1].numel() // 8 + 4
    out = torch.full((2, PASS_H, PASS_W), 0xA5, dtype=torch.uint8, device=device)
    b.decode(out=out)
    torch.cuda.synchronize(device)
    assert b.tables.status.cpu().tolist() == [0, 0]
    _same(out[0], grays[0], "frame 0")
    _same(out[1], grays[1], "frame 1")
    del out, b, grays


def _encode_async_raw(device, img, codes, offs):
    """mh_encode_frame_device_async (no-delta) into caller-filled buffers -> (status, codes_len)."""
    import torch
    from metalhuffman_amd import _native as N, encoder as E
    h, w = img.shape
    enc = E.Encoder(w, h, device)
    canon = torch.empty(256, dtype=torch.uint8, device=device)
    meta = torch.full((2,), -1, dtype=torch.int64, device=device)
    base = enc.workspace.data_ptr()
    aligned = (base + 255) // 256 * 256
    N.check(N.lib().mh_encode_frame_device_async(
        img.data_ptr(), w, h, N.MH_FLAG_NO_DELTA | N.MH_ENCODE_WORKSPACE_ZEROED, canon.data_ptr(), codes.data_ptr(),
        codes.numel(), meta.data_ptr(), offs.data_ptr(), None, meta.data_ptr() + 8, aligned,
        enc.workspace.numel() - (aligned - base), torch.cuda.current_stream(device).cuda_stream),
        "mh_encode_frame_device_async")
    torch.cuda.synchronize(device)
    return int(meta[1:2].view(torch.int32)[0].item()), int(meta[0].item())


def _untouched(t, fill):
    return bool((t == fill).all().item())


def test_encoder_refuses_2_pow_32_bits(mh, device):
    """Exactly 2^32 code bits: status MH_ERR_CAPACITY, codes_len 0, and not a byte of the
    0xAB-filled code buffer or of the block offsets written."""
    import torch
    _need(device, 4 * GiB)
    img = exactly_uniform_image(FAIL_W, FAIL_H, seed=33, device=device)
    assert img.numel() == 2 ** 29
    nb = img.numel() // 64
    codes = torch.full((nb * 128 + 32,), 0xAB, dtype=torch.uint8, device=device)
    offs = torch.full((nb,), 0x2B2B2B2B, dtype=torch.int32, device=device)
    status, codes_len = _encode_async_raw(device, img, codes, offs)
    assert status == MH_ERR_CAPACITY and codes_len == 0, (status, codes_len)
    assert _untouched(codes, 0xAB), "code bytes written for a refused frame"
    assert _untouched(offs, 0x2B2B2B2B), "block offsets written for a refused frame"
    del codes, offs, img


def test_batch_encoder_refuses_2_pow_32_bits_and_keeps_the_other_frame(mh, device):
    """n = 2: frame 0 has exactly 2^32 code bits -> MH_ERR_CAPACITY, its slot and offsets
    untouched; the constant frame 1 still encodes exactly and decodes back."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D, encoder as E
    _need(device, 8 * GiB)
    grays = torch.empty((2, FAIL_H, FAIL_W), dtype=torch.uint8, device=device)
    grays[0] = exactly_uniform_image(FAIL_W, FAIL_H, seed=34, device=device)
    grays[1].fill_(0xC7)
    be = E.BatchEncoder(FAIL_W, FAIL_H, 2, device)
    nb, slot = be.nb, be.slot
    codes = torch.full((2 * slot,), 0xAB, dtype=torch.uint8, device=device)
    assert codes.data_ptr() % 16 == 0
    offs = torch.full((2 * nb,), 0x2B2B2B2B, dtype=torch.int32, device=device)
    canon = torch.zeros((2, 256), dtype=torch.uint8, device=device)
    lens = torch.full((2,), -1, dtype=torch.int64, device=device)
    fco = torch.full((3,), -1, dtype=torch.int64, device=device)
    status = torch.full((2,), 77, dtype=torch.int32, device=device)
    base = be.workspace.data_ptr()
    aligned = (base + 255) // 256 * 256
    N.check(N.lib().mh_encode_frames_device_async(
        grays.data_ptr(), FAIL_H * FAIL_W, 2, FAIL_W, FAIL_H, N.MH_FLAG_NO_DELTA, canon.data_ptr(), codes.data_ptr(),
        slot, lens.data_ptr(), fco.data_ptr(), offs.data_ptr(), None, status.data_ptr(), aligned,
        be.workspace.numel() - (aligned - base), torch.cuda.current_stream(device).cuda_stream),
        "mh_encode_frames_device_async")
    torch.cuda.synchronize(device)
    px = FAIL_H * FAIL_W
    assert status.cpu().tolist() == [MH_ERR_CAPACITY, 0]
    assert lens.cpu().tolist() == [0, px // 8 + 4]
    assert fco.cpu().tolist() == [0, slot, 2 * slot]
    assert _untouched(codes[:slot], 0xAB), "code bytes written for a refused frame"
    assert _untouched(offs[:nb], 0x2B2B2B2B), "block offsets written for a refused frame"
    want1 = np.zeros(256, np.uint8)
    want1[0xC7] = 1
    assert np.array_equal(canon[1].cpu().numpy(), want1)
    o1 = offs[nb:].to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(o1, 64 * torch.arange(nb, dtype=torch.int64, device=device))
    assert not codes[slot: slot + px // 8 + 4].any().item()
    fr = D.DeviceFrames(FAIL_W, FAIL_H, 1, offs[nb:], codes[slot:], None, None, N.MH_FLAG_NO_DELTA, px // 8)
    out = torch.full((1, FAIL_H, FAIL_W), 0xA5, dtype=torch.uint8, device=device)
    hst = torch.full((1,), 77, dtype=torch.int32, device=device)
    D.decode_headers(fr, canon[1:2].contiguous(), out=out, header_status=hst)
    torch.cuda.synchronize(device)
    assert hst.cpu().tolist() == [0]
    _same(out[0], grays[1], "the constant frame")
    del out, fr, codes, offs, grays, be
