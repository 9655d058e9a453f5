"""mh_decode_crops_norm: crops at pixel origins decoded straight into binary16, bfloat16 or binary32
elements T[v] = cvt(fmaf(float32(v), scale, bias)), optionally mirrored, in one launch. Every slot is
prefilled with 0xA5 bytes; the expected elements are norm_helpers.table_bits (libm's fmaf, numpy's
float16 cast, integer rounding for bfloat16 -- never the code under test) indexed by the numpy slice
of the oracle's decode_frame_shader of the FULL frame (region_helpers.frame_set), reversed along x
where the crop is mirrored. Every comparison is on bit patterns; there is no tolerance.

The base frame is region_helpers': a 600 x 72 grid declared 597 x 67 (75 x 9 blocks, partial right
and bottom blocks), three distinct frames per flavour. A crop is (frame, x0, y0, flags); its size
(w, h) is the launch's. round_up(w, 8) elements of every row are written; columns >= w are not
compared. The whole slot of a rejected or skipped crop must keep the fill."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import norm_helpers as NH
import region_helpers as R
from norm_helpers import MIRROR, up8
from region_helpers import FILL, H, W

pytestmark = pytest.mark.gpu

MH_ERR_DIMS = -2
SCALE, BIAS = 1.0 / (255.0 * 0.229), -0.485 / 0.229    # the map of every test but the value test
FMTS = pytest.mark.parametrize("fmt", NH.FORMATS, ids=[NH.NAMES[f] for f in NH.FORMATS])

_TABLES: dict = {}


def table(fmt, scale=SCALE, bias=BIAS):
    key = (fmt, scale, bias)
    if key not in _TABLES:
        _TABLES[key] = NH.table_bits(fmt, scale, bias)
        _TABLES[key].setflags(write=False)
    return _TABLES[key]


def _efs(frames):
    return [f[0] for f in frames]


def _wants(frames):
    return [f[1] for f in frames]


def _filled(device, shape, fmt):
    """A tensor of the format's dtype whose every BYTE is FILL."""
    import torch
    raw = torch.full((int(np.prod(shape)) * NH.ESIZE[fmt],), FILL, dtype=torch.uint8, device=device)
    return raw.view(NH.torch_dtype(fmt)).view(*shape)


def _fill_bits(fmt):
    return NH.BITS[fmt](int.from_bytes(bytes([FILL]) * NH.ESIZE[fmt], "little"))


def decode_host(device, fr, tabs, crops, size, fmt, scale=SCALE, bias=BIAS, **kw):
    """decode_crops_normalized into slots prefilled with FILL bytes -> the bit patterns
    [n, h, round_up(w, 8)] on the host (and the per-crop status list when status=True is passed)."""
    import torch
    from metalhuffman_amd import decoder as D
    n = len(crops)
    out = _filled(device, (n, size[1], up8(size[0])), fmt)
    got = D.decode_crops_normalized(fr, tabs, crops, size, NH.torch_dtype(fmt), scale, bias, out=out, **kw)
    torch.cuda.synchronize(device)
    if kw.get("status") is True:
        assert got[0] is out
        return NH.bits_of(out, fmt), got[1].cpu().tolist()
    assert got is out
    return NH.bits_of(out, fmt)


def check(got, crops, size, wants, T):
    """Slot p holds T[the numpy slice of its frame's expected raster], mirrored where flagged, in its
    first w columns."""
    w, h = size
    assert got.shape == (len(crops), h, up8(w)) and got.dtype == T.dtype, (got.shape, got.dtype)
    for p, c in enumerate(crops):
        exp = NH.expected_crop(T, wants[int(c[0])], c, size)
        if not np.array_equal(got[p, :, :w], exp):
            ys, xs = np.nonzero(got[p, :, :w] != exp)
            raise AssertionError(f"crop {p} = {tuple(int(v) for v in c)} of {size}: {ys.size} wrong element(s), "
                                 f"first at row {int(ys[0])}, column {int(xs[0])}: {int(got[p, ys[0], xs[0]]):#x}, "
                                 f"expected {int(exp[ys[0], xs[0]]):#x}")


# ---- 1. every sub-block origin -------------------------------------------------------------------------

def _all_origins(w, h, mirror_alternate):
    """64 crops of w x h, (x0 & 7, y0 & 7) every pair, over the three frames and over the frame."""
    crops = []
    for dy in range(8):
        for dx in range(8):
            i = 8 * dy + dx
            bx = (i * 7) % ((W - w - 7) // 8 + 1)
            by = min((i * 5) % 7, (H - h - dy) // 8)
            crops.append((i % 3, 8 * bx + dx, 8 * by + dy, (i & 1) if mirror_alternate else 0))
    return crops


@FMTS
@pytest.mark.parametrize("tables", ["shared", "set"])
@pytest.mark.parametrize("w,mirrored", [(19, False), (24, True)])
def test_all_sub_block_origins(mh, oracle, device, tables, fmt, w, mirrored):
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames), tables)
    crops = _all_origins(w, 13, mirrored)
    assert {(c[1] & 7, c[2] & 7) for c in crops} == {(dx, dy) for dx in range(8) for dy in range(8)}
    assert {c[0] for c in crops} == {0, 1, 2} and max(c[2] for c in crops) == H - 13
    assert sum(c[3] for c in crops) == (32 if mirrored else 0)
    if mirrored:   # both parities of dx and every dy are mirrored somewhere
        assert {c[2] & 7 for c in crops if c[3]} == set(range(8)) and len({c[1] & 7 for c in crops if c[3]}) == 4
    got, st = decode_host(device, fr, tabs, crops, (w, 13), fmt, status=True)
    check(got, crops, (w, 13), _wants(frames), table(fmt))
    assert st == [0] * 64


# ---- 2. sizes ------------------------------------------------------------------------------------------

def _size_crops(w, h, flags):
    return [(0, 0, 0, flags), (1, W - w, H - h, flags), (2, W - w, 0, flags), (0, 0, H - h, flags), (1, 8, 8, flags),
            (2, 7, 7, flags), (0, 301, 33, flags), (1, 4, 58, flags), (2, 252, 3, flags), (0, 63, 1, flags)]


@FMTS
@pytest.mark.parametrize("h", [1, 8, 9])
@pytest.mark.parametrize("w,flags", [(1, 0), (7, 0), (8, 0), (9, 0), (17, 0), (8, MIRROR), (16, MIRROR), (24, MIRROR)])
def test_sizes(mh, oracle, device, w, flags, h, fmt):
    """The frame's first pixel, its last crop (W - w, H - h), the other two corners, and origins at
    every kind of offset, over the three frames; the widths that are multiples of 8 mirrored too."""
    frames = R.frame_set(mh, oracle, "general")
    fr, ts = R.upload(device, _efs(frames), "set")
    crops = _size_crops(w, h, flags)
    got = decode_host(device, fr, ts, crops, (w, h), fmt)
    check(got, crops, (w, h), _wants(frames), table(fmt))


# ---- 3. edges of a tile, of a row and of the frame ---------------------------------------------------------

EDGE_WIDTHS = {
    504: "63 words, one tile",
    512: "a second tile holding one word: a mirrored word crosses tiles",
    520: "two words in the second tile",
    592: "one row of 74 words, the right edge",
}


@FMTS
@pytest.mark.parametrize("flags", [0, MIRROR])
@pytest.mark.parametrize("w", list(EDGE_WIDTHS))
def test_tile_edges(mh, oracle, device, w, flags, fmt):
    """At (7, 5) -- dx = 7, dy = 5 -- and at the frame's right and bottom edge, mirrored and not."""
    frames = R.frame_set(mh, oracle, "general")
    fr, ts = R.upload(device, _efs(frames), "set")
    h = 10
    x0 = min(7, W - w)
    assert w % 8 == 0 and x0 + w <= W and (w != 592 or x0 == 5)
    crops = [(2, x0, 5, flags), (0, W - w, H - h, flags), (1, W - w, 0, flags)]
    got = decode_host(device, fr, ts, crops, (w, h), fmt)
    check(got, crops, (w, h), _wants(frames), table(fmt))


@FMTS
def test_whole_frame(mh, oracle, device, fmt):
    """597 x 67, unmirrored (the width is no multiple of 8): 75 words, two tiles a row, nine block rows."""
    frames = R.frame_set(mh, oracle, "general")
    fr, ts = R.upload(device, _efs(frames), "set")
    crops = [(f, 0, 0, 0) for f in (2, 0, 1)]
    got = decode_host(device, fr, ts, crops, (W, H), fmt)
    check(got, crops, (W, H), _wants(frames), table(fmt))


# ---- 4. step flavours ------------------------------------------------------------------------------------

FLAVOUR_MIXED = ((40, 20), [(0, 3, 5, 0), (1, 3, 47, MIRROR), (2, 3, 0, 0), (1, 297, 30, MIRROR), (2, 557, 12, MIRROR),
                            (0, 0, 0, MIRROR), (1, 584 - 27, 47, 0), (2, 251, 29, MIRROR), (0, 5, 40, 0),
                            (1, 123, 7, 0)])
FLAVOUR_WIDE = ((304, 20), [(0, 3, 5, 0), (1, 3, 47, MIRROR), (2, 3, 0, MIRROR), (1, 293, 30, 0)])


@FMTS
@pytest.mark.parametrize("flavour", R.FLAVOURS)
def test_flavours(mh, oracle, device, flavour, fmt):
    """Under each step flavour (region_helpers.build_set asserts its precondition) the new stage runs
    behind decode_block, flat8_block (flat8), the slow loops (off_grid) and decode_halves (oversize: 38
    blocks of 128 bytes at x0 = 3 exceed the stage window, and lane 31 takes its right half from the
    block lane 32 decodes beside it): one mixed list of ten crops of 40 x 20, half of them mirrored,
    and four of 304 x 20."""
    frames = R.frame_set(mh, oracle, flavour)
    assert bool(frames[0][0].flags & 1) == (flavour == "no_delta")
    assert (frames[0][0].block_init is not None) == (flavour == "block_init")
    if flavour == "oversize":
        o = frames[0][0].block_offsets.astype(np.int64)
        assert (o[38] - o[0]) // 8 > R.STAGE_BYTES
    fr, tabs = R.upload(device, _efs(frames))
    assert sum(c[3] for c in FLAVOUR_MIXED[1]) == 5 and ((3 & 7) + 304 + 7) // 8 == 39
    for size, crops in (FLAVOUR_MIXED, FLAVOUR_WIDE):
        got = decode_host(device, fr, tabs, crops, size, fmt)
        check(got, crops, size, _wants(frames), table(fmt))


# ---- 5. values ---------------------------------------------------------------------------------------------

_RAMP: dict = {}


def _ramp(mh, oracle):
    """A 256 x 8 frame holding every byte value, encoded with the host codec; expected = the oracle's decode."""
    if not _RAMP:
        img = np.ascontiguousarray(np.tile(np.arange(256, dtype=np.uint8), (8, 1)))
        img[1::2] = img[1::2, ::-1]
        img[3] = (img[3].astype(np.int32) * 7 % 256).astype(np.uint8)
        ef = mh.encode_frame(img)
        want = R.oracle_decode(oracle, ef)
        assert np.array_equal(want, img) and set(np.unique(want).tolist()) == set(range(256))
        _RAMP["v"] = (ef, want)
    return _RAMP["v"]


@FMTS
@pytest.mark.parametrize("pair", NH.PAIRS, ids=[f"pair{i}" for i in range(len(NH.PAIRS))])
def test_values(mh, oracle, device, pair, fmt):
    """All 256 byte values under each fixed (scale, bias) of the host test -- exact integers, ties,
    overflow to inf, binary16 and binary32 subnormals, a zero scale -- one crop of the whole frame,
    mirrored and not."""
    from metalhuffman_amd import codec
    ef, want = _ramp(mh, oracle)
    fr, tabs = R.upload(device, [ef])
    T = NH.table_bits(fmt, *pair)
    assert np.array_equal(codec.norm_table(NH.NAMES[fmt], *pair).view(NH.BITS[fmt]), T)
    crops = [(0, 0, 0, 0), (0, 0, 0, MIRROR)]
    got = decode_host(device, fr, tabs, crops, (256, 8), fmt, *pair)
    check(got, crops, (256, 8), [want], T)
    assert set(np.unique(got).tolist()) == set(np.unique(T).tolist())


# ---- 6. crops the kernel rejects, and a skipped frame ------------------------------------------------------

@FMTS
def test_rejected_and_skipped_crops(mh, oracle, device, fmt):
    """One launch of valid crops, one of each rejected kind and crops of a frame whose status word is
    non-zero (its header has a 17-bit length). The descriptors are a device tensor, so only the kernel
    sees them. Rejected slots keep the fill bytewise and report MH_ERR_DIMS -- also for the skipped
    frame (a rejected crop never reads the frame's word); skipped ones keep the fill and carry the
    frame's status; the valid ones among them are exact, status 0."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    efs = _efs(frames)
    fr = D.DeviceFrames.pack(efs, device, shared_table=False)
    too_long = np.zeros(256, np.uint8)
    too_long[7] = 17
    ts = D.DeviceTableSet.from_canonical_headers(np.stack([efs[0].canon, too_long, efs[2].canon]), device)
    assert ts.status.cpu().tolist() == [0, -3, 0]
    w, h = 19, 21
    desc = [(0, 3, 5, 0), (3, 0, 0, 0), (0, W - w + 1, 0, 0), (2, 0, H - h + 1, 0), (0, 0xFFFFFFFF, 0, 0),
            (2, 5, 2, 2), (2, W - w, H - h, 0), (0, 7, 7, 0x80000001), (0, 9, 9, MIRROR), (1, 30, 30, 0),
            (1, 30, 30, 2), (2, 0, H - h, 0), (1, W - w + 1, 0, 0), (0, W - w, 0, 0)]
    valid, skipped = [0, 6, 11, 13], [9]
    crops = torch.from_numpy(np.array(desc, np.uint32).view(np.int32)).to(device)
    n = len(desc)
    out = _filled(device, (n, h, up8(w)), fmt)
    status = torch.full((n,), 77, dtype=torch.int32, device=device)
    assert D.decode_crops_normalized(fr, ts, crops, (w, h), NH.torch_dtype(fmt), SCALE, BIAS, out=out,
                                     status=status) is out
    torch.cuda.synchronize(device)
    got, st = NH.bits_of(out, fmt), status.cpu().tolist()
    assert st == [0 if p in valid else -3 if p in skipped else MH_ERR_DIMS for p in range(n)], st
    for p in range(n):
        if p not in valid:
            assert (got[p] == _fill_bits(fmt)).all(), f"crop {p} = {desc[p]}: its slot was written"
    check(got[valid], [desc[p] for p in valid], (w, h), _wants(frames), table(fmt))
    # a width that is a multiple of 8 accepts the same mirrored descriptor
    got8 = decode_host(device, fr, ts, [desc[8], desc[0]], (24, h), fmt)
    check(got8, [desc[8], desc[0]], (24, h), _wants(frames), table(fmt))


# ---- 7. write containment ----------------------------------------------------------------------------------

@FMTS
@pytest.mark.parametrize("w,flags", [(19, 0), (24, MIRROR)])
@pytest.mark.parametrize("flavour", ["general", "flat8"])
def test_write_containment(mh, oracle, device, flavour, w, flags, fmt):
    """One mh_decode_crops_norm launch through the C-ABI into slots laid out inside a buffer of seeded
    random bytes: d_out at 16 mod 32, pitch = the row's bytes + 48, stride = h * pitch + 80, the first
    crop at the buffer's first byte and the last crop's last row ending at its last byte. The
    round_up(w, 8) * E bytes of each of the h rows may change -- the first w elements to their exact
    values -- and EVERY other byte of the buffer must be as it was: the rows of the first block row
    above the crop (dy of them), the row padding, the gaps between slots, and the rows below."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    E = NH.ESIZE[fmt]
    h = 13
    crops = [(0, 5, 1, flags), (1, 251, 54, flags), (2, W - w - 1, 3, flags), (1, 13, 9, flags), (2, 1, 47, flags),
             (0, 339, 30, flags)]
    assert all(c[1] & 7 and c[2] & 7 for c in crops)
    frames = R.frame_set(mh, oracle, flavour)
    fr, tabs = R.upload(device, _efs(frames))
    n, row = len(crops), up8(w) * E
    pitch, stride = row + 48, h * (row + 48) + 80
    assert pitch % 16 == 0 and stride % 16 == 0
    size = (n - 1) * stride + (h - 1) * pitch + row
    pattern = np.random.default_rng(w * 8 + fmt).integers(0, 256, 16 + size, dtype=np.uint8)
    buf = torch.from_numpy(pattern.copy()).to(device)
    assert buf.data_ptr() % 32 == 0
    d_out = buf.data_ptr() + 16                                   # 16 mod 32; the slots end with the buffer
    desc = torch.tensor([list(c) for c in crops], dtype=torch.int32, device=device)
    status = torch.full((n,), 77, dtype=torch.int32, device=device)
    st, _ = D._frames_entry(fr)
    N.check(N.lib().mh_decode_crops_norm(ctypes.byref(st), desc.data_ptr(), n, w, h, fmt, SCALE, BIAS,
                                         tabs.lut.data_ptr(), 0, None, status.data_ptr(), d_out, pitch, stride,
                                         torch.cuda.current_stream(device).cuda_stream), "mh_decode_crops_norm")
    torch.cuda.synchronize(device)
    assert status.cpu().tolist() == [0] * n
    after = buf.cpu().numpy()
    may = np.zeros(after.size, bool)
    T = table(fmt)
    for p, c in enumerate(crops):
        exp = NH.expected_crop(T, _wants(frames)[c[0]], c, (w, h))
        for y in range(h):
            o = 16 + p * stride + y * pitch
            may[o: o + row] = True
            got = after[o: o + w * E].view(NH.BITS[fmt])
            assert np.array_equal(got, exp[y]), (p, y)
    changed = np.flatnonzero((after != pattern) & ~may)
    assert changed.size == 0, f"{changed.size} byte(s) written outside the rows, first at {int(changed[0])}"


# ---- 8. flags, block_init ------------------------------------------------------------------------------------

@FMTS
@pytest.mark.parametrize("flavour", ["no_delta", "block_init"])
def test_no_delta_and_block_init(mh, oracle, device, flavour, fmt):
    frames = R.frame_set(mh, oracle, flavour)
    fr, ts = R.upload(device, _efs(frames), "set")
    size = (72, 21)
    crops = [(0, 0, 0, MIRROR), (2, 520, 0, 0), (1, 243, 46, MIRROR), (0, 517, 41, 0), (2, 1, 1, MIRROR)]
    got = decode_host(device, fr, ts, crops, size, fmt)
    check(got, crops, size, _wants(frames), table(fmt))


@FMTS
def test_any_order(mh, oracle, device, fmt):
    """MH_FLAG_ANY_ORDER: the launch may start while earlier work on the stream drains; the stream is
    idle here, and the picture is the same."""
    import torch
    from metalhuffman_amd import _native as N
    frames = R.frame_set(mh, oracle, "general")
    fr, ts = R.upload(device, _efs(frames), "set")
    size = (72, 21)
    crops = [(0, 0, 0, MIRROR), (2, 520, 0, 0), (1, 243, 46, MIRROR)]
    torch.cuda.synchronize(device)
    got = decode_host(device, fr, ts, crops, size, fmt, extra_flags=N.MH_FLAG_ANY_ORDER)
    check(got, crops, size, _wants(frames), table(fmt))


# ---- 9. the forms of `crops`, the default output and the launch shape ----------------------------------------------

@FMTS
def test_device_descriptors_in_place(mh, oracle, device, fmt):
    """An int32 [n, 4] device tensor is used where it lies: the launch reads the caller's own buffer --
    rewritten in place between two calls, the second call sees the new crops -- and the tensor is not
    changed. [n, 3] and host lists give the same picture; out = None is zero-filled and typed."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    fr, tabs = R.upload(device, _efs(frames))
    size = (80, 21)
    a = [(0, 0, 0, 0), (2, 517, 0, MIRROR), (1, 243, 46, 0), (0, 517, 41, MIRROR), (2, 1, 1, 0)]
    b = [(1, 5, 3, MIRROR), (0, 100, 20, 0), (2, 9, 9, MIRROR), (1, 0, 46, 0), (0, 517, 0, MIRROR)]
    c4 = torch.tensor(a, dtype=torch.int32, device=device)
    assert c4.is_contiguous() and c4.data_ptr() % 16 == 0
    ptr = c4.data_ptr()
    got = decode_host(device, fr, tabs, c4, size, fmt)
    check(got, a, size, _wants(frames), table(fmt))
    c4.copy_(torch.tensor(b, dtype=torch.int32, device=device))
    got = decode_host(device, fr, tabs, c4, size, fmt)
    check(got, b, size, _wants(frames), table(fmt))
    assert c4.data_ptr() == ptr and c4.cpu().tolist() == [list(x) for x in b]
    plain = [x[:3] for x in a]
    c3 = torch.tensor(plain, dtype=torch.int32, device=device)
    for form, want in ((c3, plain), (plain, plain), (np.asarray(plain), plain), (np.asarray(a), a)):
        got = decode_host(device, fr, tabs, form, size, fmt)
        check(got, want, size, _wants(frames), table(fmt))
    out, st = D.decode_crops_normalized(fr, tabs, [(0, 0, 0)], size, NH.torch_dtype(fmt), SCALE, BIAS, status=True)
    torch.cuda.synchronize(device)
    assert out.dtype is NH.torch_dtype(fmt) and tuple(out.shape) == (1, 21, 80) and st.cpu().tolist() == [0]
    check(NH.bits_of(out, fmt), [(0, 0, 0, 0)], size, _wants(frames), table(fmt))


def _tiles(size):
    ow = (size[0] + 7) // 8
    return ((size[1] + 14) // 8) * ((ow + 62) // 63)


@FMTS
@pytest.mark.parametrize("size,tiles", [((19, 13), 3), ((W, H), 20), ((512, 10), 6), ((504, 10), 3)])
def test_shape_rule(mh, oracle, device, size, tiles, fmt):
    """mh_decode_crops' rule with this kernel's occupancy: G = clamp(ceil(R / n_crops), 1, ceil(CBH S /
    8)), R = CUs x 1, 2 or 3 workgroups per CU (53,280 B of LDS admit no more)."""
    import torch
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    fr, _ = R.upload(device, _efs(frames))
    assert _tiles(size) == tiles
    most = -(-tiles // 8)
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    dt = NH.torch_dtype(fmt)
    occs = set()
    for n in (1, 2, 100, cus, 2 * cus, 3 * cus, 3 * cus + 1, 65536):
        G, waves = D.decode_crops_normalized_shape(fr, n, size, dt)
        assert waves == 8
        fit = [o for o in (1, 2, 3) if G == min(max(-(-cus * o // n), 1), most)]
        assert fit, (n, G, cus, most)
        occs.add(tuple(fit))
    assert D.decode_crops_normalized_shape(fr, 1, size, dt)[0] == most
    assert D.decode_crops_normalized_shape(fr, 65536, size, dt)[0] == 1
    assert set.intersection(*(set(f) for f in occs)), occs    # one occupancy explains every answer


@FMTS
def test_pipelined_loop_many_crops(mh, oracle, device, fmt):
    """So many crops of 520 x 60 -- S = 2, CBH = 9, 18 tiles -- that a crop gets ONE workgroup: every
    wave then owns >= 2 tiles, so header, span prefetch and decode of different tiles overlap in
    batch_loop's steady state, with the wide stores of one tile in flight under the next. Seeded
    origins, half of the crops mirrored."""
    from metalhuffman_amd import decoder as D
    frames = R.frame_set(mh, oracle, "general")
    fr, ts = R.upload(device, _efs(frames), "set")
    size = (520, 60)
    n = 768
    G, waves = D.decode_crops_normalized_shape(fr, n, size, NH.torch_dtype(fmt))
    while G > 1 and n < 8192:          # (a device with more resident workgroups)
        n *= 2
        G, waves = D.decode_crops_normalized_shape(fr, n, size, NH.torch_dtype(fmt))
    assert G == 1 and waves == 8 and _tiles(size) // (G * waves) >= 2, (n, G, waves)
    rng = np.random.default_rng(2026)
    crops = np.stack([rng.integers(0, 3, n), rng.integers(0, W - size[0] + 1, n),
                      rng.integers(0, H - size[1] + 1, n), rng.integers(0, 2, n)], axis=1)
    assert {int(v) for v in crops[:, 2]} == set(range(8)) and len({int(v) & 7 for v in crops[:, 1]}) == 8
    got = decode_host(device, fr, ts, crops, size, fmt)
    check(got, crops.tolist(), size, _wants(frames), table(fmt))
