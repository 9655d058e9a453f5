"""BatchEncoder's four methods through Python: encode_async, encode_shared_async, encode_images_async
and encode_images_shared_async with every keyword they take -- init_zero_delta, flags, limit_lengths,
a side stream, a header as a host array or a device tensor, plane_major -- on one small batch, every
frame's header, code bytes, block offsets and init bytes compared with the host codec on
codec.image_planes of the same pixels; and the ValueError text of each method's bad arguments.

The batch: two RGBA images of 52 x 40, of which the strided view [:, 6:33, 9:46, :3] goes in without
a copy: 37 x 27 pixels (5 x 4 blocks, partial right and bottom blocks), six plane frames. The two
frames methods take the same six planes as a contiguous [6, 27, 37] tensor. The kernels' shapes and
layouts are test_gpu_encode_images.py's and test_gpu_encode_batch.py's business, not this file's."""
from __future__ import annotations

import numpy as np
import pytest

import encode_helpers as EH

pytestmark = pytest.mark.gpu

N_IMG, H0, W0, W, H, X0, Y0, C = 2, 40, 52, 37, 27, 9, 6, 3
N = N_IMG * C
METHODS = ("encode_async", "encode_shared_async", "encode_images_async", "encode_images_shared_async")
# mode -> the keywords it adds (the side stream is made per call)
MODES = {"default": {}, "init_zero_delta": dict(init_zero_delta=True), "no_delta": dict(flags=EH.NO_DELTA),
         "limit_lengths": dict(limit_lengths=True), "stream": {}}


def _cases():
    for m in METHODS:
        for mode in MODES:
            for header in (("built", "host", "device") if "shared" in m else ("none",)):
                for major in ((False, True) if "images" in m else (False,)):
                    yield pytest.param(m, mode, header, major, id=f"{m}-{mode}-{header}-{'major' if major else 'minor'}")


@pytest.fixture(scope="module")
def pixels(device, bigbridge):
    """(the RGBA batch on the device, its strided RGB view, the view's pixels on the host)."""
    import torch
    planes = EH.natural_frames(bigbridge, W0, H0, N_IMG * 4, seed=8)
    rgba = torch.from_numpy(np.stack(planes).reshape(N_IMG, 4, H0, W0).transpose(0, 2, 3, 1).copy()).to(device)
    view = rgba[:, Y0:Y0 + H, X0:X0 + W, :C]
    assert not view.is_contiguous() and view.data_ptr() != rgba.data_ptr() and tuple(view.shape) == (N_IMG, H, W, C)
    return rgba, view, view.cpu().numpy()


_EXPECTED = {}


def _expected(mh, src, major, flags, init, limit, header):
    """(the plane frames, the shared header or None, codec.encode_frame of every frame): computed once
    per combination and shared, never changed."""
    key = (major, flags, init, limit, header)
    if key not in _EXPECTED:
        frames = mh.image_planes(src, 0, C, major)
        hdr = None
        if header == "built":
            hdr = mh.shared_header(frames, flags, init, limit_lengths=limit)
        elif header != "none":
            hdr = EH.supplied_header(frames, flags, init)
        efs = [mh.encode_frame(f, flags=flags, init_zero_delta=init, limit_lengths=limit and hdr is None, header=hdr)
               for f in frames]
        _EXPECTED[key] = (frames, hdr, efs)
    return _EXPECTED[key]


@pytest.mark.parametrize("method,mode,header,major", list(_cases()))
def test_method_matches_the_host_codec(mh, device, pixels, method, mode, header, major):
    import torch
    from metalhuffman_amd.encoder import BatchEncoder
    _, view, src = pixels
    kw = dict(MODES[mode])
    flags, init, limit = kw.get("flags", 0), kw.get("init_zero_delta", False), kw.get("limit_lengths", False)
    frames, hdr, efs = _expected(mh, src, major, flags, init, limit, header)
    shared, images = "shared" in method, "images" in method
    if header == "host":
        kw["header"] = hdr.copy()
    elif header == "device":
        kw["header"] = torch.from_numpy(hdr.copy()).to(device)
    if images:
        kw["plane_major"] = major
        arg = view
    else:
        arg = torch.from_numpy(frames).to(device)
        assert arg.is_contiguous() and tuple(arg.shape) == (N, H, W)
    stream = None
    if mode == "stream":
        stream = torch.cuda.Stream(device)
        stream.wait_stream(torch.cuda.current_stream(device))
        kw["stream"] = stream
    enc = BatchEncoder(W, H, N, device)
    batch = getattr(enc, method)(arg, **kw)
    (stream or torch.cuda.current_stream(device)).synchronize()

    assert (batch.width, batch.height, batch.n_frames, batch.slot, batch.flags) == (W, H, N, enc.slot, flags)
    assert batch.shared == shared
    assert (batch.n_planes, batch.plane_frame_stride) == ((C, N_IMG if major else 1) if images else (1, 1))
    status = batch.status.cpu().numpy()
    assert status.dtype == np.int32 and status.shape == (N,) and not status.any(), status
    canon = batch.canon.cpu().numpy()
    if shared:
        hs = batch.header_status.cpu().numpy()
        assert hs.dtype == np.int32 and hs.shape == (1,) and hs[0] == 0, hs
        assert canon.shape == (256,) and np.array_equal(canon, hdr)
    else:
        assert batch.header_status is None and canon.shape == (N, 256)
    lens = batch.codes_len.cpu().numpy()
    codes = batch.codes.cpu().numpy()
    assert codes.shape == (N * enc.slot,) and batch.codes.data_ptr() % 16 == 0
    assert np.array_equal(batch.frame_code_offsets.cpu().numpy(), np.arange(N + 1, dtype=np.int64) * enc.slot)
    offs = batch.block_offsets.cpu().numpy().view(np.uint32).reshape(N, enc.nb)
    assert (batch.block_init is not None) == init
    inits = batch.block_init.cpu().numpy().reshape(N, enc.nb) if init else None
    for f, ef in enumerate(efs):
        assert np.array_equal(canon if shared else canon[f], ef.canon), f
        k = ef.codes.size
        assert int(lens[f]) == k, (f, int(lens[f]), k)
        assert np.array_equal(codes[f * enc.slot: f * enc.slot + k], ef.codes), f
        assert np.array_equal(offs[f], ef.block_offsets), f
        if init:
            assert np.array_equal(inits[f], ef.block_init), f


# ---- bad arguments: the text of every ValueError ------------------------------------------------------------

GRAYS = f"grays must be contiguous uint8 [{N}, {H}, {W}]"
GRAYS_DEVICE = "grays must live on the encoder's device"
IMAGES = "images must be a uint8 tensor [n, H, W, K]"
IMAGES_SHAPE = f"images must be [n, {H}, {W}, K] with n * n_planes == {N}"
IMAGES_DEVICE = "images must live on the encoder's device"
CHANNELS = "the channels of a pixel must be adjacent bytes (stride 1)"
HEADER = "header must hold 256 code lengths"


def _raises(text, fn, *a, **kw):
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    assert str(e.value) == text


@pytest.mark.parametrize("method", METHODS[:2])
def test_frames_methods_bad_arguments(mh, device, pixels, method):
    import torch
    from metalhuffman_amd.encoder import BatchEncoder
    fn = getattr(BatchEncoder(W, H, N, device), method)
    good = torch.zeros((N, H, W), dtype=torch.uint8, device=device)
    _raises(GRAYS, fn, good.to(torch.int8))                                       # dtype
    _raises(GRAYS, fn, good[:N - 1])                                              # frames
    _raises(GRAYS, fn, good.reshape(N, W, H))                                     # H and W swapped
    _raises(GRAYS, fn, torch.zeros((N, H, W + 1), dtype=torch.uint8, device=device)[:, :, :W])  # not contiguous
    _raises(GRAYS_DEVICE, fn, good.cpu())
    _raises(GRAYS, fn, good.cpu().to(torch.int16))                                # the dtype wins over the device
    if "shared" in method:
        _raises(HEADER, fn, good, header=np.zeros(255, np.uint8))
        _raises(HEADER, fn, good, header=torch.zeros(255, dtype=torch.uint8, device=device))
        _raises(GRAYS, fn, good[:1], header=np.zeros(255, np.uint8))              # grays win over the header


@pytest.mark.parametrize("method", METHODS[2:])
def test_images_methods_bad_arguments(mh, device, pixels, method):
    import torch
    from metalhuffman_amd.encoder import BatchEncoder
    rgba, view, _ = pixels
    fn = getattr(BatchEncoder(W, H, N, device), method)
    _raises(IMAGES, fn, view.to(torch.int8))                                      # dtype
    _raises(IMAGES, fn, view[0])                                                  # three dimensions
    full = rgba[:, Y0:Y0 + H, X0:X0 + W]                                          # all four channels
    _raises("planes 2..4 of 4-channel pixels", fn, full, first_channel=2, n_planes=3)
    _raises("planes -1..1 of 4-channel pixels", fn, full, first_channel=-1, n_planes=3)
    _raises("planes 1..0 of 4-channel pixels", fn, full, first_channel=1, n_planes=0)
    _raises(IMAGES_SHAPE, fn, rgba[:, Y0:Y0 + H, X0:X0 + W + 1, :C])              # width
    _raises(IMAGES_SHAPE, fn, rgba[:, Y0:Y0 + H + 1, X0:X0 + W, :C])              # height
    _raises(IMAGES_SHAPE, fn, full)                                               # 2 * 4 planes for six frames
    _raises(IMAGES_SHAPE, fn, view[:1])                                           # 1 * 3 planes
    wide = torch.zeros((N_IMG, H, W, 8), dtype=torch.uint8, device=device)[..., ::2]
    assert wide.stride(3) == 2
    _raises(CHANNELS, fn, wide, n_planes=C)
    _raises(IMAGES_DEVICE, fn, view.cpu())
    _raises(IMAGES_SHAPE, fn, view.cpu()[:1])                                     # the shape wins over the device
    cpu_wide = torch.zeros((N_IMG, H, W, 8), dtype=torch.uint8)[..., ::2]
    _raises(CHANNELS, fn, cpu_wide, n_planes=C)                                   # ... and so does the channel stride
    if "shared" in method:
        _raises(HEADER, fn, view, header=np.zeros(255, np.uint8))
        _raises(HEADER, fn, view, header=torch.zeros(255, dtype=torch.uint8, device=device))
        _raises(IMAGES_DEVICE, fn, view.cpu(), header=np.zeros(255, np.uint8))    # the images win over the header
