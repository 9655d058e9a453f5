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
