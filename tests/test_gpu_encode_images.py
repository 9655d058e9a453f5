"""mh_encode_images_device_async and mh_encode_images_shared_device_async (built and supplied header)
on the GPU: interleaved, pitched pixels in, C-plane frames out, every output into guarded buffers and
compared byte for byte with the host codec on codec.image_planes of the same pixels
(encode_images_helpers / encode_helpers; never another GPU encode), twice over one workspace, and
decoded back on the device.

Shapes are the smallest at which the fetch can go wrong: one block, partial right and bottom blocks,
frames narrower than a packer step (16 blocks) and than a tile, a width at which a tile's lanes wrap
into the next block row, and the tile / step / packer-workgroup thresholds of encode_helpers."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

import encode_helpers as EH
import encode_images_helpers as IH
from helpers import fibonacci_deltas, image_of_symbols

pytestmark = pytest.mark.gpu

ENTRY = pytest.mark.parametrize("entry", IH.ENTRIES)
RGB = IH.Pixels(3, 0, 3)
RGB_OF_RGBA = IH.Pixels(4, 0, 3)
GBA_OF_RGBA = IH.Pixels(4, 1, 3)


def _aligned(px, w, h, pad=0, gap=0):
    """px with the row pitch and the image stride rounded up to multiples of 4 (plus pad, gap): the
    dword-load path for pixel strides <= 4."""
    pp = (-w * px.ps) % 4 + pad
    span = (h - 1) * (w * px.ps + pp) + w * px.ps
    return dataclasses.replace(px, pitch_pad=pp, gap=(-span) % 4 + gap)


# ---- 1. channels, strides, orders, pitches, base offsets, image strides --------------------------------------

# (pitch_pad, delta, gap, plane_major): exact / + 4 / odd pitch, base at 0 / 1 / 4, exact and padded image stride.
# 36 pixels a row: 36 * ps is a multiple of 4 for every ps, so the first, second and last variant are the
# dword-load path for ps <= 4; the odd pitch, the base at byte 1 and the odd image stride are the byte path.
VARIANTS = [(0, 0, 0, False), (4, 4, 8, True), (3, 0, 0, False), (0, 1, 5, True), (4, 0, 11, False), (0, 4, 4, True)]


@ENTRY
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_channels_strides_and_placements(mh, device, bigbridge, entry, C):
    w, h, n = 36, 19, 2
    seen = set()
    for ps in sorted({C, C + 1, 5, 7}):
        for k, (pad, delta, gap, major) in enumerate(VARIANTS):
            for fc in sorted({0, ps - C}) if k < 2 else [(ps - C) // 2]:
                px = IH.Pixels(ps, fc, C, major, delta, pad, gap)
                pix = IH.natural_pixels(bigbridge, w, h, n, px, seed=ps + k)
                IH.run_checked(mh, device, entry, pix, px, decode=k < 2)
                seen.add((ps <= 4, px.wide(w, h, n)))
    assert seen == {(True, True), (True, False), (False, False)}      # (stride <= 4, dword loads taken)


@ENTRY
def test_rgba_three_planes_taken(mh, device, bigbridge, entry):
    """RGB of RGBA and planes 1..3 of 4, both orders, on the dword path (13 x 11: partial blocks)."""
    for base in (RGB_OF_RGBA, GBA_OF_RGBA):
        for major in (False, True):
            px = dataclasses.replace(_aligned(base, 13, 11, gap=12), plane_major=major)
            assert px.wide(13, 11, 3)
            IH.run_checked(mh, device, entry, IH.natural_pixels(bigbridge, 13, 11, 3, px, seed=5), px)


# ---- 2. flags ---------------------------------------------------------------------------------------------

@ENTRY
@pytest.mark.parametrize("px", [RGB, IH.Pixels(5, 1, 3, True, 3, 7, 9)], ids=["dwords", "bytes"])
def test_no_delta_and_init_bytes(mh, device, bigbridge, entry, px):
    w, h = 44, 21
    px = _aligned(px, w, h) if px.ps <= 4 else px
    pix = IH.natural_pixels(bigbridge, w, h, 2, px, seed=9)
    IH.run_checked(mh, device, entry, pix, px, flags=EH.NO_DELTA)
    IH.run_checked(mh, device, entry, pix, px, init_zero=True, ws_fill=0xA7)
    IH.run_checked(mh, device, entry, pix, px, flags=EH.NO_DELTA, init_zero=True)


@ENTRY
@pytest.mark.parametrize("limit", [False, True])
def test_a_deep_tree_plane(mh, device, bigbridge, entry, limit):
    """Plane 1 of image 0 has a tree 18 deep: with MH_ENCODE_LIMIT_LENGTHS it is encoded under the
    length-limited code, without it that frame alone (per-frame tables) or the header (one table
    built from the batch; a supplied header is always a usable code) is MH_ERR_CODE_TOO_LONG."""
    bw, bh = 16, 11                                        # 176 blocks hold one Fibonacci histogram of 19 symbols
    w, h = 8 * bw, 8 * bh
    px = _aligned(RGB_OF_RGBA, w, h)
    frames = EH.natural_frames(bigbridge, w, h, 6, seed=3)
    d = fibonacci_deltas(EH.DEEP_SYMBOLS, bw * bh * 64, seed=1)
    frames[1] = image_of_symbols(d, w, h)
    pix = IH.pixel_array(frames, px)
    _, exp = IH.run_checked(mh, device, entry, pix, px, flags=EH.LIMIT if limit else 0)
    if entry == "batch":
        assert [s for s, _ in exp.frames] == [EH.OK if limit or f != 1 else EH.TOO_LONG for f in range(6)]
    elif entry == "shared_built" and not limit:
        assert exp.header_status in (EH.OK, EH.TOO_LONG)   # the summed histogram decides


@pytest.mark.parametrize("header_from", ["own", "other"])
def test_supplied_headers(mh, device, bigbridge, header_from):
    """A supplied header: the batch's own (every frame accepted), or another batch's, under which a
    frame with a symbol the header lacks is MH_ERR_TABLE and the rest are exact."""
    w, h = 40, 24
    px = _aligned(RGB, w, h)
    pix = IH.natural_pixels(bigbridge, w, h, 2, px, seed=21)
    other = IH.natural_pixels(bigbridge, w, h, 2, px, seed=22)
    src = pix if header_from == "own" else other
    header = EH.supplied_header(IH.planes(mh, src, px))
    _, exp = IH.run_checked(mh, device, "shared_supplied", pix, px, header=header)
    if header_from == "own":
        assert all(s == EH.OK for s, _ in exp.frames)


# ---- 3. geometries ------------------------------------------------------------------------------------------

GEOMETRIES = [(8, 8), (13, 11), (9, 8), (100, 20), (200, 9), (2056, 16)]


@ENTRY
@pytest.mark.parametrize("w,h", GEOMETRIES, ids=[f"{w}x{h}" for w, h in GEOMETRIES])
def test_geometries(mh, device, bigbridge, entry, w, h):
    """One block; partial right and bottom blocks; 13 blocks a row (narrower than a packer step); 25
    (narrower than a tile); 257 (a tile's lanes wrap into the next block row). Dword path (RGB, RGB of
    RGBA, two-byte pixels) and byte path."""
    for px in (_aligned(RGB, w, h, gap=4), _aligned(GBA_OF_RGBA, w, h, pad=4), _aligned(IH.Pixels(2, 1, 1), w, h),
               IH.Pixels(3, 0, 3, True, 1, 1, 3), IH.Pixels(7, 2, 4, False, 0, 0, 0)):
        n = 2 if w * h < 4096 else 1
        IH.run_checked(mh, device, entry, IH.natural_pixels(bigbridge, w, h, n, px, seed=w + h), px)


@pytest.mark.parametrize("entry,bw", [("batch", 2), ("shared_built", 33), ("shared_supplied", 17)])
def test_threshold_shapes(mh, device, bigbridge, entry, bw):
    """encode_helpers.threshold_shapes: block counts on, just below and just above one packer step, one
    tile and one packer workgroup of tiles, W on the block edge and one pixel into the last block."""
    shapes = EH.threshold_shapes("batch", bw)
    assert len(shapes) >= 10
    for k, (w, h) in enumerate(shapes):
        px = _aligned(RGB, w, h) if k % 3 else IH.Pixels(4, 1, 2, bool(k % 2), 2, 5, 7)
        IH.run_checked(mh, device, entry, IH.natural_pixels(bigbridge, w, h, 1, px, seed=k), px, decode=k % 4 == 0)


# ---- 4. nothing but the samples counts -----------------------------------------------------------------------

@ENTRY
@pytest.mark.parametrize("px", [IH.Pixels(4, 0, 3, False, 0, 8, 24), IH.Pixels(3, 0, 2, True, 4, 5, 13),
                                IH.Pixels(5, 2, 3, False, 1, 6, 9)], ids=["rgba-dwords", "rgb-dwords", "bytes"])
def test_padding_independence(mh, device, bigbridge, entry, px):
    """The same images twice, every byte that is not a selected sample -- row padding, unselected
    channels, gaps between images, the bytes in front and behind -- changed in between: every output
    is identical (and right)."""
    w, h, n = 29, 13, 3
    assert px.wide(w, h, n) == (px.ps <= 4)
    pix = IH.natural_pixels(bigbridge, w, h, n, px, seed=11)
    a, _, mask = IH.pixel_bytes(pix, px)
    b = np.where(mask, a, a ^ (np.random.default_rng(77).integers(0, 256, a.size, dtype=np.uint8) | 1)).astype(np.uint8)
    assert (a[mask] == b[mask]).all() and (a[~mask] != b[~mask]).all()
    frames = IH.planes(mh, pix, px)
    header = EH.supplied_header(frames) if entry == "shared_supplied" else None
    ra = IH.run(mh, device, entry, pix, px, init_zero=True, header=header, buf=a, rounds=1)[0]
    rb = IH.run(mh, device, entry, pix, px, init_zero=True, header=header, buf=b, rounds=1)[0]
    for k in ra.host:
        assert np.array_equal(ra.host[k], rb.host[k]), f"{k} depends on a byte that is not a sample"
    EH.check(mh, [ra, rb], frames, EH.expect(mh, entry, frames, init_zero=True, slot=ra.slot, header=header))


# ---- 5. the degenerate layout is the frames entry -------------------------------------------------------------

@ENTRY
@pytest.mark.parametrize("w,h,delta,pad", [(64, 24, 0, 0), (64, 24, 8, 64), (45, 19, 0, 0), (45, 19, 3, 5), (272, 16, 4, 4)])
def test_degenerate_layout_is_the_frames_twin(mh, device, bigbridge, entry, w, h, delta, pad):
    """C = 1, pixel stride 1, pitch W: every output equals mh_encode_frames[_shared]_device_async's on
    the same planar data, slot for slot and guard for guard (and both are the host codec's)."""
    n = 3
    frames = EH.natural_frames(bigbridge, w, h, n, seed=w)
    px = IH.Pixels(1, 0, 1, False, delta, 0, pad)
    pix = IH.pixel_array(frames, px)
    header = EH.supplied_header(frames) if entry == "shared_supplied" else None
    mine = IH.run(mh, device, entry, pix, px, init_zero=True, header=header)
    twin = EH.run(mh, device, entry, frames, init_zero=True, header=header, layout=EH.Layout(delta=delta, stride=w * h + pad))
    exp = EH.expect(mh, entry, frames, init_zero=True, slot=mine[0].slot, header=header)
    EH.check(mh, mine, frames, exp)
    EH.check(mh, twin, frames, exp)
    for k in twin[1].host:
        assert np.array_equal(mine[1].host[k], twin[1].host[k]), k


# ---- 6. a rejected plane ---------------------------------------------------------------------------------------

@ENTRY
@pytest.mark.parametrize("major", [False, True])
def test_a_rejected_plane_stands_alone(mh, device, bigbridge, entry, major):
    """One noisy plane of one image does not fit its slot: MH_ERR_CAPACITY for that frame alone, its
    slot and offsets unwritten (encode_helpers.check), its sibling planes and the other images exact."""
    w, h, n, C = 40, 24, 2, 3
    px = dataclasses.replace(_aligned(RGB_OF_RGBA, w, h), plane_major=major)
    frames = EH.natural_frames(bigbridge, w, h, n * C, seed=31)
    frames[4] = np.random.default_rng(5).integers(0, 256, (h, w), dtype=np.uint8)      # image 1, plane 1
    pix = IH.pixel_array(frames, px)
    order = IH.planes(mh, pix, px)
    header = EH.supplied_header(order) if entry == "shared_supplied" else None
    roomy = EH.expect(mh, entry, order, header=header)
    assert all(s == EH.OK for s, _ in roomy.frames)
    sizes = sorted(EH.r16(EH.r4(ef.codes.size)) for _, ef in roomy.frames)
    assert sizes[-1] > sizes[-2]
    _, exp = IH.run_checked(mh, device, entry, pix, px, slot=sizes[-2], header=header)
    noisy = 4 if not major else 1 * n + 1                  # c * n + i
    assert [s for s, _ in exp.frames] == [EH.CAPACITY if f == noisy else EH.OK for f in range(n * C)]


# ---- 7. limits ----------------------------------------------------------------------------------------------------

def _strided_on_device(device, frames, px, w, h, pitch):
    """One image whose rows are `pitch` bytes apart, built on the device (the span is ~2 GiB: only the
    rows are written, the rest is whatever the allocation held)."""
    import torch
    pix = IH.pixel_array(frames, px)
    span = (h - 1) * pitch + w * px.ps
    t = torch.empty(span + 512, dtype=torch.uint8, device=device)
    o = (t.data_ptr() + 255) // 256 * 256 - t.data_ptr() + px.delta
    t[o:].as_strided((h, w * px.ps), (pitch, 1)).copy_(torch.from_numpy(pix[0].reshape(h, w * px.ps)).to(device))
    return pix, t, t.data_ptr() + o


@pytest.mark.parametrize("entry,px", [("batch", RGB), ("shared_built", IH.Pixels(3, 0, 3, True, 1))], ids=["dwords", "bytes"])
def test_the_pitch_limit(mh, device, bigbridge, entry, px):
    """The largest addressable pitch, (rows - 1) * pitch + W * ps = MH_IMAGE_TILE_SPAN_MAX (rounded down
    to a multiple of 4 on the dword path), with a 13 x 3 image; one byte more is refused untouched."""
    w, h = 13, 3
    pitch = (IH.SPAN_MAX - w * px.ps) // (h - 1)
    if px.delta == 0:
        pitch -= pitch % 4
    frames = EH.natural_frames(bigbridge, w, h, 3, seed=2)
    pix, t, p = _strided_on_device(device, frames, px, w, h, pitch)
    order = IH.planes(mh, pix, px)
    runs = IH.run(mh, device, entry, pix, px, dev=(t, p), lay_over=dict(row_pitch=pitch, image_stride=0))
    EH.check(mh, runs, order, EH.expect(mh, entry, order, slot=runs[0].slot))
    over = (IH.SPAN_MAX - w * px.ps) // (h - 1) + 1
    refused = IH.run(mh, device, entry, pix, px, dev=(t, p), lay_over=dict(row_pitch=over, image_stride=0), launches=False)
    EH.check_untouched(refused, EH.CAPACITY)


@pytest.mark.parametrize("w,h", [(65535, 11), (11, 65535)])
def test_max_dim(mh, device, bigbridge, w, h):
    """MH_MAX_DIM in one dimension, 11 in the other, three planes of RGBA."""
    px = _aligned(RGB_OF_RGBA, w, h)
    IH.run_checked(mh, device, "batch", IH.natural_pixels(bigbridge, w, h, 1, px, seed=1), px)


# ---- 8. end to end through Python -----------------------------------------------------------------------------

@pytest.mark.parametrize("major", [False, True])
def test_strided_view_to_normalised_planes(mh, device, bigbridge, major):
    """imgs[:, y0:y1, x0:x1, :3] of an RGBA batch -> encode_images_async (no copy) -> table_set() ->
    decode_crops_normalized_planes with the batch's plane_frame_stride: bit for bit codec.norm_table
    lookups of the original pixels, one crop mirrored."""
    import torch
    from metalhuffman_amd import decoder as D
    from metalhuffman_amd.encoder import BatchEncoder
    n, H0, W0, w, h, x0, y0 = 2, 40, 52, 37, 27, 9, 6
    frames = EH.natural_frames(bigbridge, W0, H0, n * 4, seed=8)
    rgba = torch.from_numpy(IH.pixel_array(frames, IH.Pixels(4, 0, 4))).to(device)
    view = rgba[:, y0:y0 + h, x0:x0 + w, :3]
    assert not view.is_contiguous() and view.data_ptr() != rgba.data_ptr()
    enc = BatchEncoder(w, h, n * 3, device)
    batch = enc.encode_images_async(view, plane_major=major)
    assert (batch.n_planes, batch.plane_frame_stride, batch.n_frames) == (3, n if major else 1, n * 3)
    ts = batch.table_set()
    cw, ch = 24, 13                                        # a mirrored crop's width is a multiple of 8
    crops = [(i if major else 3 * i, cx, cy, fl) for i, (cx, cy, fl) in enumerate([(5, 3, 0), (8, 14, mh.MH_CROP_MIRROR)])]
    scale, bias = mh.norm_coefficients([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    out = D.decode_crops_normalized_planes(batch.frames(), ts, crops, (cw, ch), torch.float32, scale, bias,
                                           plane_stride=batch.plane_frame_stride)
    torch.cuda.synchronize(device)
    got = out.cpu().numpy()
    src = view.cpu().numpy()
    for p, (_, cx, cy, fl) in enumerate(crops):
        for c in range(3):
            want = mh.norm_table(np.float32, scale[c], bias[c])[src[p, cy:cy + ch, cx:cx + cw, c]]
            if fl:
                want = want[:, ::-1]
            assert np.array_equal(got[p, c, :, :cw].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (p, c)
    # the shared entry takes the same view
    shared = enc.encode_images_shared_async(view, plane_major=major)
    assert shared.shared and (shared.n_planes, shared.plane_frame_stride) == (3, n if major else 1)
    ref = mh.image_planes(src, 0, 3, major)
    dec = shared.decode().cpu().numpy()
    assert np.array_equal(dec[:, :, :w], ref)
