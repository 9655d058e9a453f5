"""encoder.encode_image_set_async -> AsyncEncodedSet.table_set() -> decode_set_crops and
decode_set_crops_normalized_planes on one stream with no host step between them: crops that touch
every frame and the frames' four corners, against the source pixels (the normalised entry with
norm_helpers' reference), and against the same crops of a DeviceFrameSet.pack of the host-encoded
planes."""
from __future__ import annotations

import numpy as np
import pytest

import norm_helpers as NH
import set_encode_helpers as SH

pytestmark = pytest.mark.gpu

SIZES = [(264, 120), (37, 50), (2056, 16)]   # three-plane images of three sizes
CROP = (24, 11)
PAIRS = [(1.0 / 255.0, -0.5), (0.0078125, 0.25), (-2.0, 3.0)]


def corner_crops(sizes, planes, size):
    """(frame, x0, y0) over every frame: its four corners and its middle."""
    w, h = size
    out = []
    for i, (W, H) in enumerate(sizes):
        for c in range(planes):
            for x0, y0 in ((0, 0), (W - w, 0), (0, H - h), (W - w, H - h), ((W - w) // 2, (H - h) // 2)):
                out.append((i * planes + c, x0, y0))
    return out


@pytest.fixture(scope="module")
def encoded(mh, device, bigbridge):
    import torch
    from metalhuffman_amd import decoder as D
    from metalhuffman_amd import encoder as E
    planes_of = [SH.images(bigbridge, [s] * 3, seed=23 + 5 * i) for i, s in enumerate(SIZES)]
    # [H, W, 4] images whose first three channels are taken: views of RGBA tensors, no copy
    images = []
    for planes in planes_of:
        h, w = planes[0].shape
        rgba = np.random.default_rng([w, h]).integers(0, 256, (h, w, 4), dtype=np.uint8)
        for c in range(3):
            rgba[:, :, c] = planes[c]
        images.append(torch.from_numpy(rgba).to(device))
    es = E.encode_image_set_async(images, n_planes=3, init_zero_delta=True)
    tabs = es.table_set()
    fs = es.frame_set()
    flat = [p for planes in planes_of for p in planes]
    host = D.DeviceFrameSet.pack([mh.encode_frame(p, init_zero_delta=True) for p in flat], device)
    host_tabs = D.DeviceTableSet.from_canonical_headers(np.stack([mh.encode_frame(p, init_zero_delta=True).canon
                                                                  for p in flat]), device)
    return es, fs, tabs, flat, host, host_tabs, images


def test_the_set_is_the_host_packers(mh, device, encoded):
    import torch
    es, fs, tabs, flat, host, host_tabs, _ = encoded
    assert es.n_planes == 3 and es.plane_frame_stride == 1 and es.n_frames == 9
    assert es.totals.fetch_mode == 4
    assert fs.geoms.data_ptr() == es.plan.data_ptr() + es.totals.geoms_offset      # a view into the plan
    assert torch.equal(fs.geoms, host.geoms) and fs.total_blocks == host.total_blocks
    assert (fs.width, fs.height, fs.sizes) == (host.width, host.height, host.sizes)
    assert es.status.cpu().tolist() == [0] * 9 and tabs.status.cpu().tolist() == [0] * 9
    assert torch.equal(fs.block_offsets, host.block_offsets) and torch.equal(fs.block_init, host.block_init)
    assert torch.equal(es.canon.cpu(), host_tabs._headers.cpu())
    off = es.frame_code_offsets.cpu().tolist()
    assert off == [int(v) for v in np.concatenate([[0], np.cumsum(es.slots)])]
    lens = es.codes_len.cpu().tolist()
    hoff = host.frame_code_offsets.cpu().tolist()
    for f in range(9):
        assert torch.equal(es.codes[off[f]: off[f] + lens[f]], host.codes[hoff[f]: hoff[f] + lens[f]]), f


def test_crops_decode_to_the_source_pixels(mh, device, encoded):
    import torch
    from metalhuffman_amd import decoder as D
    es, fs, tabs, flat, host, host_tabs, _ = encoded
    crops = corner_crops(SIZES, 3, CROP)
    out, st = D.decode_set_crops(fs, tabs, crops, CROP, status=True)
    ref, rst = D.decode_set_crops(host, host_tabs, crops, CROP, status=True)
    torch.cuda.synchronize(device)
    assert st.cpu().tolist() == [0] * len(crops) == rst.cpu().tolist()
    got = out.cpu().numpy()
    for p, (f, x0, y0) in enumerate(crops):
        assert np.array_equal(got[p, :, :CROP[0]], flat[f][y0: y0 + CROP[1], x0: x0 + CROP[0]]), (p, f, x0, y0)
    assert torch.equal(out[:, :, :CROP[0]], ref[:, :, :CROP[0]])


@pytest.mark.parametrize("fmt", NH.FORMATS, ids=[NH.NAMES[f] for f in NH.FORMATS])
def test_normalised_planes_decode_to_the_source_pixels(mh, device, encoded, fmt):
    import torch
    from metalhuffman_amd import decoder as D
    es, fs, tabs, flat, host, host_tabs, _ = encoded
    w, h = CROP
    crops = [(f, x0, y0, NH.MIRROR if k % 3 == 2 else 0)
             for k, (f, x0, y0) in enumerate(c for c in corner_crops(SIZES, 3, CROP) if c[0] % 3 == 0)]
    scale, bias = [p[0] for p in PAIRS], [p[1] for p in PAIRS]
    dt = NH.torch_dtype(fmt)
    out, st = D.decode_set_crops_normalized_planes(fs, tabs, crops, CROP, dt, scale, bias, n_planes=es.n_planes,
                                                   plane_stride=es.plane_frame_stride, status=True)
    ref, rst = D.decode_set_crops_normalized_planes(host, host_tabs, crops, CROP, dt, scale, bias, status=True)
    torch.cuda.synchronize(device)
    assert st.cpu().tolist() == [0] * len(crops) == rst.cpu().tolist()
    bits = NH.bits_of(out, fmt).reshape(len(crops), 3, h, NH.up8(w))
    for p, crop in enumerate(crops):
        for c in range(3):
            T = NH.table_bits(fmt, *PAIRS[c])
            assert np.array_equal(bits[p, c, :, :w], NH.expected_crop(T, flat[crop[0] + c], crop, CROP)), (p, c, crop)
    assert np.array_equal(bits[..., :w], NH.bits_of(ref, fmt).reshape(bits.shape)[..., :w])


# ---- encode_set_async over views: _plane_source's stride rules ---------------------------------------------

def _assert_set_is_the_host_codecs(mh, es, views, init=False):
    """Every frame of an AsyncEncodedSet against codec.encode_frame of the view's own pixels."""
    st, lens, off = es.status.cpu().tolist(), es.codes_len.cpu().tolist(), es.frame_code_offsets.cpu().tolist()
    codes, canon, offs = es.codes.cpu().numpy(), es.canon.cpu().numpy(), es.block_offsets.cpu().numpy().view(np.uint32)
    geoms = es.geoms.cpu().numpy()
    assert st == [0] * len(views), st
    assert off == [int(v) for v in np.concatenate([[0], np.cumsum(es.slots)])]
    for f, v in enumerate(views):
        ef = mh.encode_frame(np.ascontiguousarray(v.cpu().numpy()), init_zero_delta=init, limit_lengths=True)
        assert tuple(geoms[f, 1:3]) == (v.shape[1], v.shape[0]) == es.sizes[f]
        assert lens[f] == ef.codes.size and np.array_equal(canon[f], ef.canon), f
        assert np.array_equal(codes[off[f]: off[f] + lens[f]], ef.codes), f
        first = int(geoms[f, 0])
        assert np.array_equal(offs[first: first + ef.block_offsets.size], ef.block_offsets), f
        if init:
            assert np.array_equal(es.block_init.cpu().numpy()[first: first + ef.block_init.size], ef.block_init), f


@pytest.fixture(scope="module")
def pictures(device, bigbridge):
    """One [H, W] and one [H, W, 4] tensor whose views the tests below encode."""
    import torch
    gray = SH.images(bigbridge, [(200, 90)], seed=71)[0]
    rgba = np.stack(SH.images(bigbridge, [(70, 50)] * 4, seed=73), axis=2)
    return torch.from_numpy(gray).to(device), torch.from_numpy(np.ascontiguousarray(rgba)).to(device)


def _views(gray, rgba):
    return {"window": gray[7:47, 13:173],               # an odd address, a pitch wider than the frame
            "every other pixel": gray[:, ::2],          # pixel stride 2
            "every third row": gray[::3],               # a tripled pitch
            "row of a transposed view": gray.t()[5:6],  # height 1: strides (1, 200), the row stride never stepped over
            "column": gray[:, 17:18],                   # width 1: any pixel stride
            "alpha alone": rgba[..., 3]}                # pixels % 4 == 3 at stride 4, no sibling plane


def test_views_encode_as_their_pixels(mh, device, pictures):
    """Each view alone (a window and the odd shapes by bytes, [:, ::2] by dwords at stride 2, [::3] at
    stride 1, alpha alone at stride 4) and all of them in one set, against codec.encode_frame of the
    view's pixels."""
    import torch
    from metalhuffman_amd import _native as N
    from metalhuffman_amd import encoder as E
    views = _views(*pictures)
    assert [tuple(v.shape) for v in views.values()] == [(40, 160), (90, 100), (30, 200), (1, 90), (90, 1), (50, 70)]
    assert not any(v.is_contiguous() for k, v in views.items() if k not in ("row of a transposed view", "column"))
    modes = {"window": N.MH_SET_FETCH_BYTES, "every other pixel": 2, "every third row": 1, "alpha alone": 4}
    for name, v in views.items():
        es = E.encode_set_async([v], limit_lengths=True)
        torch.cuda.synchronize(device)
        if name in modes:
            assert es.totals.fetch_mode == modes[name], name
        _assert_set_is_the_host_codecs(mh, es, [v])
    es = E.encode_set_async(list(views.values()), init_zero_delta=True, limit_lengths=True)
    torch.cuda.synchronize(device)
    assert es.totals.fetch_mode == N.MH_SET_FETCH_BYTES
    _assert_set_is_the_host_codecs(mh, es, list(views.values()), init=True)


def test_views_that_are_refused(mh, device, pictures):
    """ValueError from the stride rules, before the planner and any launch: a pixel stride above 255, a
    row stride below 1, another dtype, another device type -- alone, and behind a good plane."""
    import torch
    from metalhuffman_amd import encoder as E
    gray, rgba = pictures
    wide = torch.zeros((4, 300), dtype=torch.uint8, device=device)
    bad = {"pixel stride 300": wide.t(), "row stride 0": gray[0:1].expand(5, 200),
           "int8": gray.view(torch.int8), "float": gray.float(), "3-D": rgba, "host": gray.cpu()}
    assert wide.t().stride() == (1, 300) and bad["row stride 0"].stride(0) == 0
    for name, v in bad.items():
        for planes in ([v], [gray, v]):
            with pytest.raises(ValueError):
                E.encode_set_async(planes)
    with pytest.raises(ValueError):
        E.encode_set_async([])
    with pytest.raises(ValueError):
        E.encode_set_async([gray, gray[::3]], slot_bytes=[4096])
    torch.cuda.synchronize(device)


# ---- slot_bytes, a rejected frame, and the decoders behind it on one side stream -----------------------------

def _small_images(device, bigbridge):
    import torch
    sizes = [(72, 40), (37, 50), (120, 24)]
    planes_of = [SH.images(bigbridge, [s] * 3, seed=91 + 5 * i) for i, s in enumerate(sizes)]
    flat = [p for planes in planes_of for p in planes]
    images = [torch.from_numpy(np.ascontiguousarray(np.stack(planes, axis=2))).to(device) for planes in planes_of]
    torch.cuda.synchronize(device)
    return sizes, flat, images


def _decode_and_compare(mh, device, es, flat, sizes, rejected, stream):
    """decode_set_crops and decode_set_crops_normalized_planes behind the encode on `stream`, no host
    step in between; then, after one synchronisation: the rejected frames' crops report -4 and leave
    their slots as they were, the others are the source pixels."""
    import torch
    from metalhuffman_amd import decoder as D
    crop = (24, 11)
    w, h = crop
    crops = corner_crops(sizes, 3, crop)
    samples = [(f, x0, y0, 0) for f, x0, y0 in crops if f % 3 == 0]
    with torch.cuda.stream(stream):
        tabs = es.table_set(stream)
        fs = es.frame_set()
        out = torch.full((len(crops), h, NH.up8(w)), 0xA5, dtype=torch.uint8, device=device)
        _, st = D.decode_set_crops(fs, tabs, crops, crop, out=out, status=True, stream=stream)
        nout = torch.full((len(samples), 3, h, NH.up8(w)), 7.0, dtype=torch.float32, device=device)
        _, nst = D.decode_set_crops_normalized_planes(fs, tabs, samples, crop, torch.float32, [1.0] * 3, [0.0] * 3,
                                                      n_planes=es.n_planes, plane_stride=es.plane_frame_stride, out=nout,
                                                      status=True, stream=stream)
    torch.cuda.synchronize(device)
    want = [-4 if f in rejected else 0 for f in range(len(flat))]
    assert es.status.cpu().tolist() == want and tabs.status.cpu().tolist() == want
    assert st.cpu().tolist() == [want[f] for f, _, _ in crops]
    got = out.cpu().numpy()
    for p, (f, x0, y0) in enumerate(crops):
        if f in rejected:
            assert (got[p] == 0xA5).all(), (p, f)
        else:
            assert np.array_equal(got[p, :, :w], flat[f][y0: y0 + h, x0: x0 + w]), (p, f, x0, y0)
    # a sample is skipped whole when one of its planes was rejected, and reports that plane's status
    assert nst.cpu().tolist() == [-4 if any(f + c in rejected for c in range(3)) else 0 for f, _, _, _ in samples]
    ngot = nout.cpu().numpy()
    for p, (f, x0, y0, _) in enumerate(samples):
        if any(f + c in rejected for c in range(3)):
            assert (ngot[p] == 7.0).all(), (p, f)
        else:
            for c in range(3):
                assert np.array_equal(ngot[p, c, :, :w], flat[f + c][y0: y0 + h, x0: x0 + w].astype(np.float32)), (p, c)


def test_slot_bytes_and_a_rejected_frame_on_a_side_stream(mh, device, bigbridge):
    """slot_bytes as an int, as a list per frame and (encode_image_set_async) as a list per image; a too
    small slot gives that frame -4 in es.status, table_set().status carries it, and both set decoders
    skip its crops and report it while the other frames' crops are the source pixels -- all on a
    non-default stream with no host step between the encode and the decodes."""
    import torch
    from metalhuffman_amd import encoder as E
    sizes, flat, images = _small_images(device, bigbridge)
    planes = [im[:, :, c] for im in images for c in range(3)]
    roomy = [E.default_slot_bytes(*s) for s in sizes for _ in range(3)]
    stream = torch.cuda.Stream(device)
    # an int: every slot that size
    es = E.encode_set_async(planes, init_zero_delta=True, stream=stream, limit_lengths=True, slot_bytes=max(roomy), n_planes=3)
    assert es.slots == (max(roomy),) * 9 and es.totals.codes_bytes == 9 * max(roomy)
    _decode_and_compare(mh, device, es, flat, sizes, set(), stream)
    # one per frame: frame 4 (image 1, plane 1) gets 16 bytes
    per_frame = list(roomy)
    per_frame[4] = 16
    es = E.encode_set_async(planes, init_zero_delta=True, stream=stream, limit_lengths=True, slot_bytes=per_frame, n_planes=3)
    assert es.slots == tuple(per_frame)
    _decode_and_compare(mh, device, es, flat, sizes, {4}, stream)
    # one per image: image 2's three planes get 16 bytes each
    per_image = [roomy[0], roomy[3], 16]
    es = E.encode_image_set_async(images, init_zero_delta=True, stream=stream, limit_lengths=True, slot_bytes=per_image)
    assert es.slots == tuple(roomy[:6] + [16] * 3) and es.n_planes == 3
    _decode_and_compare(mh, device, es, flat, sizes, {6, 7, 8}, stream)
    # ... and per frame through the images entry
    es = E.encode_image_set_async(images, init_zero_delta=True, stream=stream, limit_lengths=True, slot_bytes=per_frame)
    assert es.slots == tuple(per_frame)
    _decode_and_compare(mh, device, es, flat, sizes, {4}, stream)
    with pytest.raises(ValueError):
        E.encode_image_set_async(images, slot_bytes=[4096, 4096])
