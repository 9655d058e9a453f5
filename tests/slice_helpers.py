"""Helpers of the slice-decode limit and sweep tests (test_gpu_slice_limits.py, test_gpu_slice_sweep.py,
test_slice_sweep_cases.py): frames of zoo headers at any grid (the 65535-wide and 65535-high ones
included), one contained launch of any of the seven entries that go through slice_decode, and a seeded
case generator.

The expected picture of every entry is a numpy slice of the oracle's decode_frame_shader of the FULL
declared frame (itself asserted equal to the image the frame was made from), reduced with
scaled_helpers.box_reduce_np at a scale -- never another GPU decode."""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np

import region_helpers as R
import scaled_helpers as S
from helpers import check_containment, containment_plan, frame_under_header, header_zoo

ENTRIES = ("frames", "headers", "region", "region_scaled", "windows", "windows_scaled", "crops")
SCALED = ("region_scaled", "windows_scaled")

# name -> (grid W, grid H, declared W, declared H)
GEOMETRIES = {
    "wide": (65536, 16, 65535, 11),     # 8192 x 2 blocks: widest bw, right block 7 columns, bottom row 3 rows
    "tall": (16, 65536, 11, 65535),     # 2 x 8192 blocks: tallest bh, block row 8191 with 7 rows
    "tiny": (8, 8, 5, 3),               # one partial block, 63 dead lanes
    "one_row": (520, 8, 513, 1),        # 65 x 1 blocks, H = 1: the second tile is one block of one column
    "base": (R.GRID_W, R.GRID_H, R.W, R.H),   # region_helpers' base frame
}

# flavour -> (header, format)
FLAVOURS = {
    "escapes": ("escapes", "delta"),
    "noesc": ("noesc", "delta"),
    "flat": ("flat", "delta"),
    "8x256": ("8x256", "delta"),
    "16x256": ("16x256", "delta"),
    "no_delta": ("escapes", "no_delta"),
    "block_init": ("escapes", "init_zero_delta"),
}
HEADERS = ("escapes", "noesc", "flat", "8x256", "16x256")
FORMATS = ("delta", "no_delta", "init_zero_delta")
_HEADERS: dict = {}
_FRAMES: dict = {}


def _up8(v):
    return (v + 7) // 8 * 8


def _lens(canon):
    L = canon[canon > 0]
    return int(L.min()), int(L.max())


def headers():
    """The five headers, picked from the zoo by property as test_gpu_code_addressing._case_list does;
    every property is asserted."""
    if not _HEADERS:
        zoo = header_zoo()
        by = {z.name: z for z in zoo}
        rnd = [z for z in zoo if z.kind == "random"]
        esc = next(z for z in rnd if z.longest == 16 and _lens(z.canon)[0] < 13)
        noesc = next(z for z in rnd if z.longest == 13)
        flat = next(z for z in rnd if _lens(z.canon)[0] == z.longest and 4 <= z.longest <= 13)
        assert _lens(esc.canon)[1] == 16 and _lens(esc.canon)[0] < 13       # the 13-bit table with escapes
        assert _lens(noesc.canon)[1] == 13                                  # the escape-free step
        assert _lens(flat.canon)[0] == _lens(flat.canon)[1] and 4 <= _lens(flat.canon)[1] <= 13
        assert (by["8x256/a"].canon == 8).all() and (by["16x256/a"].canon == 16).all()
        _HEADERS.update(escapes=esc, noesc=noesc, flat=flat)
        _HEADERS["8x256"] = by["8x256/a"]
        _HEADERS["16x256"] = by["16x256/a"]
    return _HEADERS


def grid_of(name):
    return GEOMETRIES[name] if isinstance(name, str) else tuple(int(v) for v in name)


def one_frame(mh, oracle, name, header, fmt, j):
    """Frame j of `header` in format `fmt` at a geometry (a GEOMETRIES name or (grid W, grid H, W, H))
    -> (EncodedFrame declared W x H, expected raster). Built once per session; read-only. The expected
    raster is the oracle's decode of the declared frame and equals the source image's crop."""
    gw, gh, w, h = grid_of(name)
    key = (gw, gh, w, h, header, fmt, j)
    if key not in _FRAMES:
        assert gw % 8 == 0 and gh % 8 == 0 and gw - 8 < w <= gw and gh - 8 < h <= gh
        canon = headers()[header].canon
        seed = [gw, gh, HEADERS.index(header), FORMATS.index(fmt), j, 2026]
        ef, img = frame_under_header(canon, gw, gh, seed, no_delta=fmt == "no_delta",
                                     init_zero_delta=fmt == "init_zero_delta")
        assert bool(ef.flags & 1) == (fmt == "no_delta") and (ef.block_init is not None) == (fmt == "init_zero_delta")
        if header in ("8x256", "16x256"):
            # 16x256: every block is 128 bytes, so every tile of more than 34 blocks exceeds the stage
            # window (64 blocks: 8192 B > 4352 B) and decodes in decode_halves
            bits = 64 * int(header.split("x")[0])
            ends = np.append(ef.block_offsets.astype(np.int64), 8 * ef.payload_bytes)
            assert (np.diff(ends) == bits).all()
        ef = dataclasses.replace(ef, width=w, height=h)
        want = R.oracle_decode(oracle, ef)
        assert np.array_equal(want, img[:h, :w]), key
        want.setflags(write=False)
        _FRAMES[key] = (ef, want)
    return _FRAMES[key]


def limit_frames(mh, oracle, name, flavour, n):
    """n distinct frames of one header at a named geometry -> [(EncodedFrame, expected raster)]."""
    header, fmt = FLAVOURS[flavour]
    out = [one_frame(mh, oracle, name, header, fmt, j) for j in range(n)]
    assert len({ef.codes.tobytes() for ef, _ in out}) == n, "the frames of a set differ"
    return out


@dataclasses.dataclass
class Uploaded:
    frames: object            # decoder.DeviceFrames
    wants: list               # expected full rasters, one per frame
    canons: np.ndarray        # u8[n, 256]


def upload(device, frames, tables, entry):
    """-> (Uploaded, tabs). tables: "shared" (one prepared table at stride 0; the frames share a header)
    or "set" (a table per frame, built on the device). The whole-frame entries have no stride 0:
    mh_decode_frames always gets a table per frame and mh_decode_headers the headers themselves."""
    from metalhuffman_amd import decoder as D
    efs = [f[0] for f in frames]
    canons = np.stack([np.asarray(ef.canon, np.uint8) for ef in efs])
    if tables == "shared":
        assert all(np.array_equal(c, canons[0]) for c in canons)
    if entry == "headers":
        fr, tabs = D.DeviceFrames.pack(efs, device, shared_table=False), None
    elif entry == "frames":
        fr, tabs = R.upload(device, efs, "set")
    else:
        fr, tabs = R.upload(device, efs, tables)
    return Uploaded(fr, [f[1] for f in frames], canons), tabs


def counts(entry, width, height, what=None):
    """What a launch of `entry` over `what` covers, by the host layer's rules: S segments per block
    row, tiles per raster, block rows, and for crops OW output words and the most blocks NB a row of a
    crop touches."""
    gbw, gbh = (width + 7) // 8, (height + 7) // 8
    if entry in ("frames", "headers"):
        return {"S": -(-gbw // 64), "tiles": -(-gbw * gbh // 64), "rows": gbh}
    if entry in ("region", "region_scaled"):
        bw, bh = what[2:]
    else:
        bw, bh = what[1]
    if entry != "crops":
        return {"S": -(-bw // 64), "tiles": bh * -(-bw // 64), "rows": bh}
    ow = (bw + 7) // 8
    return {"S": -(-ow // 63), "tiles": ((bh + 14) // 8) * -(-ow // 63), "rows": (bh + 14) // 8, "OW": ow,
            "NB": max(((int(c[1]) & 7) + bw + 7) // 8 for c in what[0])}


def slots_of(entry, up, what, k):
    """-> (written columns, rows of a slot, [(expected picture, zero-filled beyond it)] per slot)."""
    fr, wants = up.frames, up.wants
    W, H, c = fr.width, fr.height, 8 >> k
    assert (k > 0) == (entry in SCALED)
    if entry in ("frames", "headers"):
        return _up8(W), H, [(w, False) for w in wants]
    if entry in ("region", "region_scaled"):
        pics = [S.box_reduce_np(R.crop(w, what, W, H), k) if k else R.crop(w, what, W, H) for w in wants]
        return what[2] * c, pics[0].shape[0], [(p, k > 0) for p in pics]
    rects, size = what
    if entry == "crops":
        w, h = size
        pics = []
        for f, x0, y0 in rects:
            assert 0 <= x0 and x0 + w <= W and 0 <= y0 and y0 + h <= H, ((f, x0, y0), size)
            pics.append((wants[f][y0: y0 + h, x0: x0 + w], False))
        return _up8(w), h, pics
    pics = []
    for f, bx0, by0 in rects:
        pic = R.crop(wants[f], (bx0, by0, size[0], size[1]), W, H)
        pics.append((S.box_reduce_np(pic, k) if k else pic, k > 0))
    return size[0] * c, size[1] * c, pics


def _launch(entry, up, tabs, what, k, d_out, pitch, stride, device):
    """The C-ABI call of `entry`; -> the per-raster status tensor the entry filled (or None)."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    fr = up.frames
    st, _ = D._frames_entry(fr)
    stream = torch.cuda.current_stream(device).cuda_stream
    L = N.lib()
    if entry == "headers":
        hdr = torch.from_numpy(up.canons.copy()).to(device)
        verdict = torch.full((fr.n_frames,), 77, dtype=torch.int32, device=device)
        N.check(L.mh_decode_headers(ctypes.byref(st), hdr.data_ptr(), None, verdict.data_ptr(), d_out, pitch, stride,
                                    stream), "mh_decode_headers")
        torch.cuda.synchronize(device)
        return verdict
    if isinstance(tabs, D.DeviceTables):
        luts, lstride, fstatus = tabs.lut.data_ptr(), 0, None
    else:
        luts, lstride, fstatus = tabs.luts.data_ptr(), tabs.stride, tabs.status.data_ptr()
    status = None
    if entry == "frames":
        rc = L.mh_decode_frames(ctypes.byref(st), luts, lstride, fstatus, d_out, pitch, stride, stream)
    elif entry in ("region", "region_scaled"):
        rg = N.mh_region(*what)
        if entry == "region":
            rc = L.mh_decode_region(ctypes.byref(st), ctypes.byref(rg), luts, lstride, fstatus, d_out, pitch, stride, stream)
        else:
            rc = L.mh_decode_region_scaled(ctypes.byref(st), ctypes.byref(rg), k, luts, lstride, fstatus, d_out, pitch,
                                           stride, stream)
    else:
        rects, size = what
        n = len(rects)
        desc = torch.tensor([[int(v) for v in r] + [0] for r in rects], dtype=torch.int32, device=device)
        assert desc.shape == (n, 4) and desc.data_ptr() % 16 == 0
        status = torch.full((n,), 77, dtype=torch.int32, device=device)
        head = (ctypes.byref(st), desc.data_ptr(), n, size[0], size[1])
        tail = (luts, lstride, fstatus, status.data_ptr(), d_out, pitch, stride, stream)
        if entry == "windows":
            rc = L.mh_decode_windows(*head, *tail)
        elif entry == "windows_scaled":
            rc = L.mh_decode_windows_scaled(*head, k, *tail)
        elif entry == "crops":
            rc = L.mh_decode_crops(*head, *tail)
        else:
            raise KeyError(entry)
    N.check(rc, "mh_decode_" + entry)
    torch.cuda.synchronize(device)
    if not isinstance(tabs, D.DeviceTables):
        assert not tabs.status.any().item(), "a header of the set was rejected"
    return status


def run_contained(entry, device, geom, up, tabs, what=None, k=0, care=None):
    """One launch of any of the seven entries through the C ABI into rasters laid out inside
    helpers.containment_plan's pattern-filled buffer, then a check of EVERY byte of it: slot p may be
    written in its first rows_p rows x `cols` columns and nowhere else, holds its expected picture in
    the picture's columns and, at a scale, zeros in the written columns beyond.
    what: None (frames, headers), a block region (bx0, by0, bw, bh), ([(frame, bx0, by0)], (bw, bh))
    for windows or ([(frame, x0, y0)], (w, h)) for crops. geom: "tight", "loose"
    (scaled_helpers.scaled_geometry with c = 8 >> k) or (pitch, stride, lead, tail). Per-window and
    per-crop status words must be 0, as must the headers' verdicts.
    care: None, or one bool[H, W] per frame (uniform over every 8 x 8 block): a picture's pixels are
    compared only where its frame's mask is True; the guard bytes are compared everywhere."""
    import torch
    c = 8 >> k
    cols, rows, pics = slots_of(entry, up, what, k)
    n = len(pics)
    cares = None
    if care is not None:
        # a scaled cell lies inside one block, so the mask's cells reduce to 0 or 255 exactly
        masks = dataclasses.replace(up, wants=[np.where(m, 255, 0).astype(np.uint8) for m in care])
        cares = [m == 255 for m, _ in slots_of(entry, masks, what, k)[2]]
        assert all(m.shape == pic.shape for m, (pic, _) in zip(cares, pics))
    if isinstance(geom, str):
        pitch, stride, lead = S.scaled_geometry(geom, cols, rows, c)
        tail = 8 * pitch + 4096
    else:
        pitch, stride, lead, tail = geom
    if geom == "loose":
        assert pitch % (2 * c) == c and stride % (2 * c) == c
    rects = [(what[0][p], what[1]) if entry in ("windows", "windows_scaled", "crops") else what for p in range(n)]
    run_slots(device, cols, rows, pics, (pitch, stride, lead, tail),
              lambda d_out: _launch(entry, up, tabs, what, k, d_out, pitch, stride, device),
              label=lambda p: f"{entry}, slot {p} = {rects[p]}, k {k}", cares=cares,
              align=(256, 0) if geom == "tight" else (2 * c, c) if geom == "loose" else (16, 8))


def run_slots(device, cols, rows, pics, geom, launch, label=lambda p: f"slot {p}", cares=None, align=None):
    """run_contained's body for any launch: pics = [(picture u8[ph <= rows, pw <= cols], zeros beyond
    it)] per slot, geom = (pitch, stride, lead, tail), launch(d_out) -> a status tensor (every word
    must be 0) or None, cares = None or a bool mask per picture (compare only where True), align =
    (modulus, remainder) d_out must have."""
    import torch
    pitch, stride, lead, tail = geom
    n = len(pics)
    base = containment_plan(n, 1, rows, pitch, stride, lead, tail, written_cols=cols)
    may = np.zeros(base.size, bool)
    for p, (pic, _) in enumerate(pics):
        assert pic.shape[0] <= rows and pic.shape[1] <= cols, (p, pic.shape, rows, cols)
        np.lib.stride_tricks.as_strided(may[lead + p * stride:], (pic.shape[0], cols), (pitch, 1))[...] = True
    assert int(may.sum()) == cols * sum(pic.shape[0] for pic, _ in pics)
    # the guard check is check_containment's, over the per-slot mask; the pictures differ in size from
    # slot to slot (a window at the frame's edge is clipped), so they are compared below
    plan = dataclasses.replace(base, W=0, may_write=may)
    buf = torch.from_numpy(base.pattern.copy()).to(device)
    d_out = buf.data_ptr() + plan.d_out
    if align is not None:
        assert d_out % align[0] == align[1], (d_out, align)
    status = launch(d_out)
    if status is not None:
        st = status.cpu().tolist()
        assert st == [0] * len(st), st
    torch.cuda.synchronize(device)
    after = buf.cpu().numpy()
    del buf
    check_containment(after, plan, [np.empty((rows, 0), np.uint8)] * n)
    got = base.frame_view(after, cols)
    for p, (pic, zeros) in enumerate(pics):
        ph, pw = pic.shape
        wrong = got[p, :ph, :pw] != pic
        if cares is not None:
            wrong &= cares[p]
        if wrong.any():
            ys, xs = np.nonzero(wrong)
            y, x = int(ys[0]), int(xs[0])
            raise AssertionError(f"{label(p)}: {ys.size} wrong pixel(s) of {ph} x {pw}, first at "
                                 f"row {y}, column {x}: {int(got[p, y, x]):#04x}, expected {int(pic[y, x]):#04x}; last at "
                                 f"row {int(ys[-1])}, column {int(xs[-1])}")
        if zeros:
            assert (got[p, :ph, pw:] == 0).all(), f"{label(p)}: written columns >= SW = {pw} are not 0"


# ---- the seeded sweep -------------------------------------------------------------------------------------

GBW_PICKS = (1, 2, 7, 8, 9, 31, 32, 33, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 191, 192, 193)
GBH_PICKS = (1, 2, 3, 7, 8, 9, 17)
SWEEP_SALT = 22
SWEEP_DEFAULT_CASES = 40


@dataclasses.dataclass(frozen=True)
class SweepCase:
    entry: str
    i: int
    grid: tuple               # (grid W, grid H, declared W, declared H)
    flavour: str              # frame 0's; fixes the format of every frame
    frames: tuple             # (header, j) per frame
    tables: str               # "shared" or "set"
    what: object              # run_contained's `what`
    k: int
    geom: str

    @property
    def fmt(self):
        return FLAVOURS[self.flavour][1]

    def rects(self):
        """[(frame or None, x0, y0, w, h)] in pixels, clipped to the frame."""
        _, _, W, H = self.grid
        if self.entry in ("frames", "headers"):
            return [(None, 0, 0, W, H)]
        if self.entry in ("region", "region_scaled"):
            return [(None, *R.region_pixels(self.what, W, H))]
        rs, size = self.what
        if self.entry == "crops":
            return [(f, x0, y0, size[0], size[1]) for f, x0, y0 in rs]
        return [(f, *R.region_pixels((bx0, by0, size[0], size[1]), W, H)) for f, bx0, by0 in rs]

    def describe(self):
        gw, gh, W, H = self.grid
        return (f"sweep_case({self.entry!r}, {self.i}): grid {gw // 8} x {gh // 8} blocks declared {W} x {H}, "
                f"{self.flavour} frames {list(self.frames)}, tables {self.tables}, what {self.what}, k {self.k}, "
                f"geom {self.geom}")


def _axis(r, total, size):
    """An origin for an extent of `size` inside `total`: the far edge pinned to the frame's with
    probability 1/2, else the near edge pinned to the origin with probability 1/2, else uniform."""
    if r.random() < 0.5:
        return total - size
    if r.random() < 0.5:
        return 0
    return int(r.integers(0, total - size + 1))


def _size(r, total):
    """An extent in 1..total: the whole with probability 1/4, else uniform."""
    return total if r.random() < 0.25 else int(r.integers(1, total + 1))


def sweep_case(entry, i):
    """Case i of `entry`: everything follows from (entry, i) alone."""
    e, i = ENTRIES.index(entry), int(i)
    r = np.random.default_rng([e, i, SWEEP_SALT])
    # every other case walks the tile-boundary picks in turn, so any 40 cases in a row visit (all but
    # one of) them whatever the seed; the rest are uniform
    gbw = GBW_PICKS[(i // 2 + 3 * e) % len(GBW_PICKS)] if i % 2 == 0 else int(r.integers(1, 201))
    gbh = GBH_PICKS[(i // 2 + e) % len(GBH_PICKS)] if i % 4 in (0, 3) else int(r.integers(1, 25))
    W, H = 8 * gbw - int(r.integers(0, 8)), 8 * gbh - int(r.integers(0, 8))
    n = int(r.integers(1, 4))
    flavour = str(r.choice(list(FLAVOURS)))
    tables = "shared" if r.random() < 0.5 else "set"
    header = FLAVOURS[flavour][0]
    frames = [(header, 0)]
    for f in range(1, n):
        other = str(r.choice(HEADERS)) if tables == "set" and r.random() < 0.5 else header
        frames.append((other, f))
    k = int(r.integers(1, 4)) if entry in SCALED else 0
    geom = "tight" if r.random() < 0.5 else "loose"
    what = None
    if entry in ("region", "region_scaled"):
        bw, bh = _size(r, gbw), _size(r, gbh)
        what = (_axis(r, gbw, bw), _axis(r, gbh, bh), bw, bh)
    elif entry in ("windows", "windows_scaled"):
        bw, bh = _size(r, gbw), _size(r, gbh)
        what = ([(int(r.integers(0, n)), _axis(r, gbw, bw), _axis(r, gbh, bh)) for _ in range(int(r.integers(1, 6)))],
                (bw, bh))
    elif entry == "crops":
        w, h = _size(r, W), _size(r, H)
        what = ([(int(r.integers(0, n)), _axis(r, W, w), _axis(r, H, h)) for _ in range(int(r.integers(1, 6)))],
                (w, h))
    return SweepCase(entry, int(i), (8 * gbw, 8 * gbh, W, H), flavour, tuple(frames), tables, what, k, geom)


def sweep_frames(mh, oracle, case):
    """The case's frames -> [(EncodedFrame, expected raster)]."""
    return [one_frame(mh, oracle, case.grid, header, case.fmt, j) for header, j in case.frames]


def sweep_range():
    """(first, count) of the default sweep, or of a longer one asked for through the environment."""
    import os
    return int(os.environ.get("MH_SLICE_SWEEP_FIRST", "0")), int(os.environ.get("MH_SLICE_SWEEP_CASES",
                                                                                str(SWEEP_DEFAULT_CASES)))
