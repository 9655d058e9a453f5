"""Helpers of the frame-set tests (test_gpu_set_crops.py, test_gpu_set_crops_planes.py): seeded images
of different sizes encoded once per session, their upload as a DeviceFrameSet, and launches of the two
set entries through the C-ABI into GUARDED buffers -- a guard zone in front of the first slot and behind
the last, gaps between rows (the pitch is wider than a row), between planes and between slots, all
prefilled with FILL bytes. check() compares EVERY byte of such a buffer: what an accepted crop writes,
against the source image's own [y0: y0 + h, x0: x0 + w] (cross-checked once with codec.decode_frame_cpu);
everything else against FILL. The only bytes not compared are the contract's unspecified ones: elements
w .. round_up(w, 8) - 1 of a written row."""
from __future__ import annotations

import ctypes

import numpy as np

import norm_helpers as NH

FILL = 0xA5
MH_ERR_DIMS, MH_ERR_INVALID_ARG = -2, -1
GUARD, ROW_GAP, PLANE_GAP, SLOT_GAP = 256, 16, 32, 64   # bytes; multiples of 16, the widest alignment rule
FORMATS = ("delta", "raw", "delta_init", "raw_init")     # delta or raw pixels, with block_init or without
TABLES = ("set", "shared")                               # a table per frame, or one for all

_CACHE: dict = {}


def up8(v):
    return (v + 7) // 8 * 8


def image(w, h, seed):
    """A seeded h x w picture: a smooth ramp plus noise with a few outliers, so the deltas' histogram
    is skewed (codes of many lengths) and no two frames are alike."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 96 + 3 * xx + 2 * yy + rng.normal(0, 6, (h, w))
    out = np.where(rng.random((h, w)) < 0.02, rng.integers(0, 256, (h, w)), base)
    return np.ascontiguousarray(np.clip(out, 0, 255).astype(np.uint8))


def encoded(mh, sizes, fmt="delta", shared=False, seed=0):
    """[(EncodedFrame, image)] for sizes = ((w, h), ...), encoded once and left unchanged. shared: all
    under one header (codec.shared_header); else each under its own tree. Every frame is checked here
    against the CPU decoder: the image IS the expected raster."""
    key = (tuple(sizes), fmt, shared, seed)
    if key not in _CACHE:
        flags = mh.MH_FLAG_NO_DELTA if fmt.startswith("raw") else 0
        init = fmt.endswith("_init")
        imgs = [image(w, h, 1000 * seed + 17 * i + w + 256 * h) for i, (w, h) in enumerate(sizes)]
        hdr = mh.shared_header(imgs, flags, init, limit_lengths=True) if shared else None
        out = []
        for im in imgs:
            ef = mh.encode_frame(im, flags=flags, init_zero_delta=init, limit_lengths=True, header=hdr)
            assert np.array_equal(mh.decode_frame_cpu(ef), im), key
            assert (ef.block_init is not None) == init
            im.setflags(write=False)
            out.append((ef, im))
        _CACHE[key] = out
    return _CACHE[key]


def upload(device, efs, shared=False):
    """-> (DeviceFrameSet, DeviceTables | DeviceTableSet)."""
    from metalhuffman_amd import decoder as D
    fs = D.DeviceFrameSet.pack(efs, device)
    if shared:
        assert all(np.array_equal(ef.canon, efs[0].canon) for ef in efs)
        t1, t2 = efs[0].tables()
        return fs, D.DeviceTables.upload(t1, t2, device)
    return fs, D.DeviceTableSet.from_canonical_headers(np.stack([ef.canon for ef in efs]), device)


def table_args(tabs, frame_status="tables"):
    """(d_luts, stride, d_frame_status) of a table argument; frame_status: "tables" (the table set's
    own status words, none for a shared table), None, or an int32 device tensor."""
    from metalhuffman_amd import decoder as D
    if isinstance(tabs, D.DeviceTables):
        luts, stride, st = tabs.lut, 0, None
    else:
        luts, stride, st = tabs.luts, tabs.stride, tabs.status
    if frame_status != "tables":
        st = frame_status
    return luts.data_ptr(), stride, (st.data_ptr() if st is not None else None)


class Launch:
    """One guarded launch's result: the whole buffer's bytes on the host, its layout and the
    per-descriptor status words."""

    def __init__(self, buf, status, n, C, size, esize, rc):
        self.buf, self.status, self.n, self.C, self.size, self.esize, self.rc = buf, status, n, C, size, esize, rc
        w, h = size
        self.row = up8(w) * esize
        self.pitch = self.row + ROW_GAP
        self.plane = h * self.pitch + PLANE_GAP
        self.slot = C * self.plane + SLOT_GAP
        self.total = 2 * GUARD + n * self.slot

    def offset(self, p, c, y):
        return GUARD + p * self.slot + c * self.plane + y * self.pitch


def _layout(n, C, size, esize):
    return Launch(None, None, n, C, size, esize, None)


def run_crops(device, fs, tabs, desc, size, frame_status="tables", crop_status=True, geoms=None,
              total_blocks=None):
    """mh_decode_set_crops of desc = int32-able [n, 4] (frame, x0, y0, reserved) into a guarded buffer.
    geoms / total_blocks: records and a count other than the set's own (a [n_frames, 4] array)."""
    return _run(device, fs, tabs, desc, size, None, frame_status, crop_status, geoms, total_blocks)


def run_planes(device, fs, tabs, desc, size, fmt, pairs, plane_stride=1, frame_status="tables",
               crop_status=True, geoms=None, total_blocks=None):
    """mh_decode_set_crops_norm_planes of desc = [n, 4] (frame, x0, y0, flags), one (scale, bias) of
    `pairs` per plane, into a guarded buffer of the format's elements."""
    return _run(device, fs, tabs, desc, size, (fmt, list(pairs), plane_stride), frame_status, crop_status, geoms,
                total_blocks)


def _run(device, fs, tabs, desc, size, norm, frame_status, crop_status, geoms, total_blocks):
    import torch
    from metalhuffman_amd import _native as N
    desc = np.ascontiguousarray(np.asarray(desc, np.int64).astype(np.uint32).view(np.int32).reshape(-1, 4))
    n = desc.shape[0]
    C = len(norm[1]) if norm else 1
    esize = NH.ESIZE[norm[0]] if norm else 1
    lay = _layout(n, C, size, esize)
    buf = torch.full((lay.total,), FILL, dtype=torch.uint8, device=device)
    d_desc = torch.from_numpy(desc).to(device)
    st = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=device) if crop_status is True else crop_status
    g = fs.geoms if geoms is None else torch.from_numpy(
        np.ascontiguousarray(np.asarray(geoms, np.int64).astype(np.uint32).view(np.int32).reshape(-1, 4))).to(device)
    tb = fs.total_blocks if total_blocks is None else total_blocks
    luts, stride, fst = table_args(tabs, frame_status)
    fr = fs.frame_struct()
    w, h = size
    out = buf.data_ptr() + GUARD
    assert out % 16 == 0 and g.data_ptr() % 16 == 0 and d_desc.data_ptr() % 16 == 0
    if norm:
        arr = ctypes.c_float * C
        rc = N.lib().mh_decode_set_crops_norm_planes(
            ctypes.byref(fr), g.data_ptr(), tb, d_desc.data_ptr(), n, w, h, norm[0], C, norm[2],
            arr(*[p[0] for p in norm[1]]), arr(*[p[1] for p in norm[1]]), luts, stride, fst,
            st.data_ptr() if st is not None else None, out, lay.pitch, lay.plane, lay.slot, None)
    else:
        rc = N.lib().mh_decode_set_crops(ctypes.byref(fr), g.data_ptr(), tb, d_desc.data_ptr(), n, w, h, luts,
                                         stride, fst, st.data_ptr() if st is not None else None, out, lay.pitch,
                                         lay.slot, None)
    torch.cuda.synchronize(device)
    lay.rc = rc
    lay.buf = buf.cpu().numpy()
    lay.status = st.cpu().tolist() if st is not None else None
    return lay


def check(lay, expected):
    """Every byte of the guarded buffer. expected[p]: None for a descriptor that must have written
    nothing, else the list (one per plane) of the [h, w] arrays the slot's planes must hold -- uint8
    pixels, or the format's bit patterns."""
    w, h = lay.size
    exp = np.full(lay.total, FILL, np.uint8)
    care = np.ones(lay.total, bool)
    assert len(expected) == lay.n
    for p, planes in enumerate(expected):
        if planes is None:
            continue
        assert len(planes) == lay.C
        for c, px in enumerate(planes):
            assert px.shape == (h, w), (px.shape, lay.size)
            rows = np.ascontiguousarray(px).view(np.uint8).reshape(h, w * lay.esize)
            for y in range(h):
                o = lay.offset(p, c, y)
                exp[o: o + w * lay.esize] = rows[y]
                care[o + w * lay.esize: o + lay.row] = False
    bad = np.flatnonzero((lay.buf != exp) & care)
    if bad.size:
        o = int(bad[0])
        rel = o - GUARD
        p, r = divmod(rel, lay.slot) if rel >= 0 else (-1, rel)
        c, r2 = divmod(r, lay.plane)
        y, x = divmod(r2, lay.pitch)
        raise AssertionError(f"{bad.size} wrong byte(s) of {lay.total}; first at offset {o} (slot {p}, plane {c}, "
                             f"row {y}, byte {x}): {int(lay.buf[o]):#x}, expected {int(exp[o]):#x}")


def pixels(imgs, d, size):
    """The source image's own slice for descriptor d = (frame, x0, y0, ...)."""
    w, h = size
    f, x0, y0 = int(d[0]), int(d[1]), int(d[2])
    px = imgs[f][y0: y0 + h, x0: x0 + w]
    assert px.shape == (h, w), (d, size, imgs[f].shape)
    return px


def fits(sizes, d, size):
    """The contract's verdict on a raw-crop descriptor (frame, x0, y0, reserved), from the sizes alone."""
    f, x0, y0, r = (int(v) for v in d)
    if not 0 <= f < len(sizes) or r != 0:
        return False
    W, H = sizes[f]
    return size[0] <= W and size[1] <= H and 0 <= x0 <= W - size[0] and 0 <= y0 <= H - size[1]
