"""Helpers of the scaled-decode tests (test_box_reduce.py, test_scaled_abi.py, test_gpu_scaled.py):
the one numpy statement of the box filter's definition, the scaled sizes, and one decode through
mh_decode_region_scaled into a pattern-guarded buffer. box_reduce_np calls nothing from the product."""
from __future__ import annotations

import ctypes

import numpy as np

from helpers import check_containment, containment_plan
from region_helpers import FILL, crop, region_pixels


def box_reduce_np(img, k):
    """The definition: the H x W image at scale s = 2^k -> u8[ceil(H / s), ceil(W / s)], every byte
    floor((2 S + n) / (2 n)) over the cell's n pixels INSIDE the image, 0 where n = 0. Zero-pad to
    a multiple of s, reshape-sums in int64, counts from an array of ones."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    s = 1 << k
    h, w = img.shape
    sh, sw = -(-h // s), -(-w // s)
    pad = np.zeros((sh * s, sw * s), np.int64)
    ones = np.zeros((sh * s, sw * s), np.int64)
    pad[:h, :w] = img
    ones[:h, :w] = 1
    S = pad.reshape(sh, s, sw, s).sum(axis=(1, 3))
    n = ones.reshape(sh, s, sw, s).sum(axis=(1, 3))
    out = np.where(n > 0, (2 * S + n) // np.maximum(2 * n, 1), 0)
    assert out.max(initial=0) <= 255
    return out.astype(np.uint8)


def scaled_size(region, k, width, height):
    """(SW, SH, written columns bw * c) of a block region at scale 2^k."""
    _, _, rw, rh = region_pixels(region, width, height)
    s = 1 << k
    return -(-rw // s), -(-rh // s), region[2] * (8 >> k)


def expected_scaled(want_full, region, k, width, height):
    """The region's crop of a full expected raster, reduced: u8[SH, SW]."""
    return box_reduce_np(crop(want_full, region, width, height), k)


def decode_scaled_host(device, fr, tabs, region, k, **kw):
    """decode_region_scaled into a raster prefilled with FILL -> u8[n, SH, bw * c] on the host."""
    import torch
    from metalhuffman_amd import decoder as D
    _, sh, cols = scaled_size(region, k, fr.width, fr.height)
    out = torch.full((fr.n_frames, sh, cols), FILL, dtype=torch.uint8, device=device)
    got = D.decode_region_scaled(fr, tabs, D.Region(*region), k, out=out, **kw)
    assert got is out
    torch.cuda.synchronize(device)
    return out.cpu().numpy()


def check_scaled(got, region, k, expected_frames, width, height):
    """got[n, SH, bw * c]: the reduced crop of every expected full raster in its first SW columns,
    zeros in the columns beyond (cells of a right-edge block wholly outside the frame)."""
    sw, sh, cols = scaled_size(region, k, width, height)
    assert got.shape == (len(expected_frames), sh, cols), (got.shape, (sh, cols))
    for f, want in enumerate(expected_frames):
        exp = expected_scaled(want, region, k, width, height)
        assert exp.shape == (sh, sw)
        if not np.array_equal(got[f, :, :sw], exp):
            ys, xs = np.nonzero(got[f, :, :sw] != exp)
            raise AssertionError(f"region {region}, k {k}, frame {f}: {ys.size} wrong pixel(s), first at row "
                                 f"{int(ys[0])}, column {int(xs[0])}: {int(got[f, ys[0], xs[0]])}, expected "
                                 f"{int(exp[ys[0], xs[0]])}")
        assert (got[f, :, sw:] == 0).all(), f"region {region}, k {k}, frame {f}: columns >= SW are not 0"


def scaled_geometry(geom, cols, sh, c):
    """-> (pitch, stride, lead) for a raster of sh rows of `cols` written bytes, store width c.
    tight: no slack at all, d_out aligned to 256. loose: slack in the pitch and between frames, and
    d_out, the pitch and the stride multiples of c but not of 2 c."""
    assert cols % c == 0
    if geom == "tight":
        return cols, sh * cols, 4096
    pitch = cols + c if (cols + c) % (2 * c) else cols + 2 * c
    stride = sh * pitch + 5 * c
    if stride % (2 * c) == 0:
        stride += c
    assert pitch % (2 * c) == c and stride % (2 * c) == c and pitch > cols and stride > sh * pitch
    return pitch, stride, 4096 + c


def decode_scaled_contained(device, geom, fr, tabs, region, k, expected_frames):
    """One mh_decode_region_scaled launch through the C ABI into a raster laid out inside a
    pattern-filled buffer (helpers.containment_plan with W = SW, H = SH, written columns bw * c),
    then a check of EVERY byte of the buffer: nothing outside rows < SH x bw * c columns changed,
    the picture in the first SW columns, zeros in the written columns beyond."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    n, c = fr.n_frames, 8 >> k
    sw, sh, cols = scaled_size(region, k, fr.width, fr.height)
    pitch, stride, lead = scaled_geometry(geom, cols, sh, c)
    plan = containment_plan(n, sw, sh, pitch, stride, lead, 8 * pitch + 4096, written_cols=cols)
    buf = torch.from_numpy(plan.pattern.copy()).to(device)
    d_out = buf.data_ptr() + plan.d_out
    assert d_out % 256 == 0 if geom == "tight" else d_out % (2 * c) == c
    st, _ = D._frames_entry(fr)
    rg = N.mh_region(*region)
    if isinstance(tabs, D.DeviceTables):
        luts, lstride, status = tabs.lut.data_ptr(), 0, None
    else:
        luts, lstride, status = tabs.luts.data_ptr(), tabs.stride, tabs.status.data_ptr()
    N.check(N.lib().mh_decode_region_scaled(ctypes.byref(st), ctypes.byref(rg), k, luts, lstride, status, d_out,
                                            pitch, stride, torch.cuda.current_stream(device).cuda_stream),
            "mh_decode_region_scaled")
    torch.cuda.synchronize(device)
    after = buf.cpu().numpy()
    check_containment(after, plan, [expected_scaled(e, region, k, fr.width, fr.height) for e in expected_frames])
    assert (plan.frame_view(after, cols)[:, :, sw:] == 0).all(), "written columns >= SW are not 0"
