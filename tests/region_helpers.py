"""Helpers of the region-decode tests (test_region_abi.py, test_gpu_region.py): frame sets of
one step flavour each on the base grid, the oracle's expectation of a region, and one decode
through mh_decode_region into a pattern-guarded buffer."""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np

from helpers import (check_containment, containment_plan, encode_with_header, fibonacci_deltas,
                     image_from_block_deltas, image_of_symbols, shift_stream)

# The base frame: a 600 x 72 grid (75 x 9 blocks) declared 597 x 67 -- partial right and bottom blocks
GRID_W, GRID_H, W, H = 600, 72, 597, 67
GBW, GBH = GRID_W // 8, GRID_H // 8
NB = GBW * GBH
STAGE_BYTES = 4352   # kStageBytes (mh_decode.hip)
FILL = 0xA5

REGIONS = {
    "full": (0, 0, 75, 9),
    "w64": (3, 2, 64, 5),
    "w65": (3, 2, 65, 5),          # second tile of every row: one live lane
    "w70": (5, 1, 70, 7),
    "right_edge": (11, 0, 64, 9),  # RW = 509
    "bottom_edge": (0, 4, 10, 5),  # RH = 35
    "last_block": (74, 8, 1, 1),
    "first_block": (0, 0, 1, 1),
    "column": (37, 0, 1, 9),
    "last_row": (0, 8, 75, 1),
}


def region_pixels(region, width=W, height=H):
    """(x0, y0, RW, RH) of a block region inside a width x height frame."""
    bx0, by0, bw, bh = region
    return (8 * bx0, 8 * by0, min(width, 8 * (bx0 + bw)) - 8 * bx0, min(height, 8 * (by0 + bh)) - 8 * by0)


def crop(img, region, width=W, height=H):
    x0, y0, rw, rh = region_pixels(region, width, height)
    return np.ascontiguousarray(np.asarray(img)[y0: y0 + rh, x0: x0 + rw])


def oracle_decode(O, ef):
    t1, t2 = ef.tables()
    return O.decode_frame_shader(ef.block_offsets, ef.codes, t1, t2, ef.width, ef.height,
                                 block_init=ef.block_init, delta=not (ef.flags & 1))


def lens(ef):
    L = ef.canon[ef.canon > 0]
    return int(L.min()), int(L.max()), int(L.size)


def _flat_symbols(n_values, nb, seed):
    assert (nb * 64) % n_values == 0
    d = np.repeat(np.arange(n_values, dtype=np.uint8), nb * 64 // n_values)
    np.random.default_rng(seed).shuffle(d)
    return d


FLAVOURS = ("general", "general14", "noesc", "flat4", "flat8", "off_grid", "no_delta", "block_init", "oversize")
N_DISTINCT = 3


def build_set(mh, flavour, grid_w=GRID_W, grid_h=GRID_H, width=W, height=H, n=N_DISTINCT):
    """n frames of one canonical table on the grid, declared width x height -> [(EncodedFrame, image
    crop)]. The flavour's precondition on the canonical lengths is asserted here:
      general    17-symbol Fibonacci histogram: codes of 1..16 bits (13-bit table with escapes)
      general14  15 symbols: 1..14 bits (escapes)
      noesc      14 symbols: 1..13 bits (escape-free step)
      flat4      16 symbols of 4 bits (escape-free, swizzled stage)
      flat8      the {8: 256} header: byte loop
      off_grid   flat8 with the stream moved 1 + i bits: no block on the byte grid, the slow loop
      no_delta   the general histogram as pixels (MH_FLAG_NO_DELTA)
      block_init general14's images with every block's first delta in block_init (13- or 14-bit codes)
      oversize   the {16: 256} header: every block is 128 bytes, every window escapes"""
    from metalhuffman_amd import frames as F
    nb = (grid_w // 8) * (grid_h // 8)
    kw = {}
    if flavour in ("flat8", "off_grid", "oversize"):
        bits = 16 if flavour == "oversize" else 8
        canon = np.full(256, bits, np.uint8)
        efs, imgs = [], []
        for i in range(n):
            d = np.random.default_rng(70 + i).integers(0, 256, nb * 64, dtype=np.uint8)
            efs.append(encode_with_header(canon, d, grid_w, grid_h))
            imgs.append(image_of_symbols(d, grid_w, grid_h))
        assert lens(efs[0]) == (bits, bits, 256)
        for ef in efs:
            assert (np.diff(ef.block_offsets.astype(np.int64)) == 64 * bits).all()
        if flavour == "off_grid":
            efs = [shift_stream(ef, 1 + i) for i, ef in enumerate(efs)]
            assert all((ef.block_offsets % 8 != 0).all() for ef in efs)
    else:
        if flavour in ("general", "no_delta"):
            d, want = fibonacci_deltas(17, nb * 64, seed=1), (1, 16, 17)
        elif flavour in ("general14", "block_init"):
            d, want = fibonacci_deltas(15, nb * 64, seed=1), (1, 14, 15)
        elif flavour == "noesc":
            d, want = fibonacci_deltas(14, nb * 64, seed=1), (1, 13, 14)
        elif flavour == "flat4":
            d, want = _flat_symbols(16, nb, 3), (4, 4, 16)
        else:
            raise KeyError(flavour)
        if flavour == "no_delta":  # the symbols are the pixels
            base = np.ascontiguousarray(d.reshape(grid_h, grid_w))
            kw = {"flags": mh.MH_FLAG_NO_DELTA}
        else:
            base = image_from_block_deltas(d, grid_w, grid_h)
        if flavour == "block_init":
            kw = {"init_zero_delta": True}
        imgs = [F.block_shuffle(base, 40 + s) for s in range(n)]
        efs = [mh.encode_frame(im, **kw) for im in imgs]
        if flavour == "block_init":  # (moving the first deltas out of the codes shifts the histogram a little)
            assert all(ef.block_init is not None for ef in efs) and 13 <= lens(efs[0])[1] <= 14
        else:
            assert lens(efs[0]) == want, (flavour, lens(efs[0]))
    for ef in efs:
        assert (ef.width, ef.height) == (grid_w, grid_h) and np.array_equal(ef.canon, efs[0].canon)
    efs = [dataclasses.replace(ef, width=width, height=height) for ef in efs]
    assert len({ef.codes.tobytes() for ef in efs}) == len(efs), "the frames of a set differ"
    return [(ef, np.ascontiguousarray(im[:height, :width])) for ef, im in zip(efs, imgs)]


_SETS: dict = {}


def frame_set(mh, O, flavour, **kw):
    """Encoded once per session: [(frame, expected full raster)], expected = the oracle's decode of
    the whole declared frame, which must also be the image the frame was made from. Read-only."""
    key = (flavour, tuple(sorted(kw.items())))
    if key not in _SETS:
        out = []
        for ef, img in build_set(mh, flavour, **kw):
            want = oracle_decode(O, ef)
            assert np.array_equal(want, img), key
            want.setflags(write=False)
            out.append((ef, want))
        _SETS[key] = out
    return _SETS[key]


def upload(device, efs, tables="shared"):
    """-> (DeviceFrames, DeviceTables | DeviceTableSet). tables: "shared" (one prepared table, stride
    0; the frames share a header) or "set" (a table per frame, built on the device)."""
    from metalhuffman_amd import decoder as D
    if tables == "shared":
        fr = D.DeviceFrames.pack(efs, device)
        t1, t2 = efs[0].tables()
        return fr, D.DeviceTables.upload(t1, t2, device)
    assert tables == "set"
    fr = D.DeviceFrames.pack(efs, device, shared_table=False)
    return fr, D.DeviceTableSet.from_canonical_headers(np.stack([ef.canon for ef in efs]), device)


def decode_region_host(device, fr, tabs, region, **kw):
    """decode_region into a raster prefilled with FILL -> u8[n, RH, 8 bw] on the host."""
    import torch
    from metalhuffman_amd import decoder as D
    _, _, rw, rh = region_pixels(region, fr.width, fr.height)
    out = torch.full((fr.n_frames, rh, 8 * region[2]), FILL, dtype=torch.uint8, device=device)
    got = D.decode_region(fr, tabs, D.Region(*region), out=out, **kw)
    assert got is out
    torch.cuda.synchronize(device)
    return out.cpu().numpy()


def check_region(got, region, expected_frames, width=W, height=H):
    """got[n, RH, 8 bw] holds the region's rectangle of every expected full raster in its first RW
    columns (columns RW .. 8 bw - 1 of a right-edge block row are written with unspecified bytes)."""
    _, _, rw, rh = region_pixels(region, width, height)
    assert got.shape == (len(expected_frames), rh, 8 * region[2]), got.shape
    for f, want in enumerate(expected_frames):
        exp = crop(want, region, width, height)
        if not np.array_equal(got[f, :, :rw], exp):
            ys, xs = np.nonzero(got[f, :, :rw] != exp)
            raise AssertionError(f"region {region}, frame {f}: {ys.size} wrong pixel(s), first at row {int(ys[0])}, "
                                 f"column {int(xs[0])}: {int(got[f, ys[0], xs[0]]):#04x}, expected "
                                 f"{int(exp[ys[0], xs[0]]):#04x}")


def geometry(geom, rw, rh):
    """-> (pitch, stride, lead): test_gpu_write_containment.py's two geometries for an rw x rh raster."""
    w8 = (rw + 7) // 8 * 8
    if geom == "tight":
        return w8, rh * w8, 4096
    pitch = w8 + 8 if (w8 + 8) % 16 else w8 + 16
    assert pitch % 8 == 0 and pitch % 16 == 8 and pitch > w8
    return pitch, rh * pitch + 40, 4096 + 8


def decode_region_contained(device, geom, fr, tabs, region, expected_frames):
    """One mh_decode_region launch through the C-ABI into a raster laid out inside a pattern-filled
    buffer (helpers.containment_plan with W = RW, H = RH), then a check of EVERY byte of it."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    n = fr.n_frames
    _, _, rw, rh = region_pixels(region, fr.width, fr.height)
    pitch, stride, lead = geometry(geom, rw, rh)
    plan = containment_plan(n, rw, rh, pitch, stride, lead, 8 * pitch + 4096, written_cols=8 * region[2])
    buf = torch.from_numpy(plan.pattern.copy()).to(device)
    d_out = buf.data_ptr() + plan.d_out
    assert d_out % 256 == 0 if geom == "tight" else (d_out % 16 == 8 and stride - rh * pitch == 40)
    st, _ = D._frames_entry(fr)
    rg = N.mh_region(*region)
    if isinstance(tabs, D.DeviceTables):
        luts, lstride, status = tabs.lut.data_ptr(), 0, None
    else:
        luts, lstride, status = tabs.luts.data_ptr(), tabs.stride, tabs.status.data_ptr()
    N.check(N.lib().mh_decode_region(ctypes.byref(st), ctypes.byref(rg), luts, lstride, status, d_out, pitch, stride,
                                     torch.cuda.current_stream(device).cuda_stream), "mh_decode_region")
    torch.cuda.synchronize(device)
    check_containment(buf.cpu().numpy(), plan, [crop(e, region, fr.width, fr.height) for e in expected_frames])
