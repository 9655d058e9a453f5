"""MH_ENCODE_LIMIT_LENGTHS on the device: the limiter inside the tree workgroup of all
three encoder paths (fused, four-kernel, batched) gives the host codec's frame byte for
byte -- header, code bytes, byte count, block offsets, init bytes, status MH_OK -- for
frames whose Huffman tree is deeper than 16, and the existing device chain decodes it
back to the input. Without the flag such a frame still reports MH_ERR_CODE_TOO_LONG."""
from __future__ import annotations

import numpy as np
import pytest

import limit_helpers as LH

pytestmark = pytest.mark.gpu


def _image(freq, w, h, seed, fmt):
    no_delta, _ = LH.FORMATS[fmt]
    return LH.image_from_histogram(freq, w, h, seed, no_delta=no_delta)


def _host(mh, img, fmt, limit=True):
    no_delta, init = LH.FORMATS[fmt]
    return mh.encode_frame(img, flags=1 if no_delta else 0, init_zero_delta=init, limit_lengths=limit)


def _host_rejects(mh, img, fmt) -> bool:
    try:
        _host(mh, img, fmt, limit=False)
    except mh.MHError as e:
        assert e.status == -3
        return True
    return False


def _same_frame(dev, host, init):
    """A DeviceEncodedFrame against the host's EncodedFrame."""
    assert np.array_equal(dev.canon, host.canon)
    assert dev.codes.numel() == host.codes.size
    assert np.array_equal(dev.codes.cpu().numpy(), host.codes)
    assert np.array_equal(dev.block_offsets.cpu().numpy().view(np.uint32), host.block_offsets)
    if init:
        assert np.array_equal(dev.block_init.cpu().numpy(), host.block_init)
    assert dev.flags == host.flags and not dev.flags & 0x200


def _check_sync(mh, device, enc, img, fmt):
    """Encoder.encode (host header and byte count), then upload tables and decode."""
    import torch
    from metalhuffman_amd import decoder as D
    no_delta, init = LH.FORMATS[fmt]
    host = _host(mh, img, fmt)
    dev = enc.encode(torch.from_numpy(img).to(device), 1 if no_delta else 0, init, limit_lengths=True)
    _same_frame(dev, host, init)
    t1, t2 = mh.Huffman.generateSplitLookupTables(dev.canon)
    out = D.decode(dev.frames(), D.DeviceTables.upload(t1, t2, device))
    torch.cuda.synchronize(device)
    assert np.array_equal(out[0, :, : img.shape[1]].cpu().numpy(), img)


def _check_async(mh, device, enc, img, fmt, limit=True):
    """Encoder.encode_async -> device tables -> decode, no host step in between."""
    import torch
    from metalhuffman_amd import decoder as D
    no_delta, init = LH.FORMATS[fmt]
    host = _host(mh, img, fmt)
    a = enc.encode_async(torch.from_numpy(img).to(device), 1 if no_delta else 0, init, limit_lengths=limit)
    out = D.decode(a.frames(), a.tables())
    torch.cuda.synchronize(device)
    assert int(a.status.item()) == 0
    assert int(a.codes_len.item()) == host.codes.size
    assert not a.flags & 0x200
    _same_frame(a.result(), host, init)
    assert np.array_equal(out[0, :, : img.shape[1]].cpu().numpy(), img)


@pytest.mark.parametrize("fmt", list(LH.FORMATS))
@pytest.mark.parametrize("nsym", [18, 19, 24])
def test_fused_path_small_frames(mh, device, fmt, nsym):
    """128 x 64 (two code tiles, the fused kernel): 18 Fibonacci symbols are depth 17, the
    smallest that trips; through Encoder.encode and encode_async."""
    from metalhuffman_amd.encoder import Encoder
    img = _image(LH.fib_histogram(nsym, 128 * 64, seed=nsym), 128, 64, nsym, fmt)
    assert _host_rejects(mh, img, fmt)
    enc = Encoder(128, 64, device)
    _check_sync(mh, device, enc, img, fmt)
    _check_async(mh, device, enc, img, fmt)


def test_fused_path_alternating_frames_on_one_encoder(mh, device, bigbridge):
    """Limited, ordinary, limited on one Encoder: the workspace and the fused path's table
    tags are reused; the ordinary frame is the unflagged frame, and without the flag the
    deep frame is still rejected and the encoder goes on."""
    import torch
    from metalhuffman_amd.encoder import Encoder
    w, h = 128, 64
    deep = [_image(LH.fib_histogram(n, w * h, seed=n), w, h, n, "delta") for n in (20, 23)]
    plain = np.ascontiguousarray(bigbridge[:h, 300:300 + w])
    assert not _host_rejects(mh, plain, "delta")
    enc = Encoder(w, h, device)
    for img in (deep[0], plain, deep[1], plain, deep[0]):
        _check_async(mh, device, enc, img, "delta")
    a = enc.encode_async(torch.from_numpy(deep[0]).to(device))
    b = enc.encode_async(torch.from_numpy(plain).to(device))
    torch.cuda.synchronize(device)
    assert int(a.status.item()) == -3 and int(a.codes_len.item()) == 0
    _same_frame(b.result(), mh.encode_frame(plain), False)
    _check_async(mh, device, enc, plain, "delta", limit=False)


def test_four_kernel_path_64bit_ranking(mh, device):
    """2056 x 2048: 515 code tiles (past the fused path) and 4,210,688 symbols (past the
    32-bit key range, so the tree ranks on 64-bit keys); 30 Fibonacci symbols."""
    from metalhuffman_amd.encoder import Encoder
    w, h = 2056, 2048
    img = _image(LH.fib_histogram(30, w * h, seed=30), w, h, 30, "delta")
    assert _host_rejects(mh, img, "delta")
    _check_async(mh, device, Encoder(w, h, device), img, "delta")


@pytest.fixture(scope="module")
def chain_image():
    return LH.image_from_histogram(LH.chain_histogram(), 1024, 1024, 5)


def test_full_level_lists_single_frame(mh, device, chain_image):
    """All 256 symbols present and a depth-17 tree: level lists of 511 items."""
    from metalhuffman_amd.encoder import Encoder
    assert _host_rejects(mh, chain_image, "delta")
    _check_async(mh, device, Encoder(1024, 1024, device), chain_image, "delta")


def _check_batch(mh, device, enc, imgs, fmt, limit, deep):
    """One batched call against the host, frame by frame; returns the AsyncEncodedBatch."""
    import torch
    no_delta, init = LH.FORMATS[fmt]
    a = enc.encode_async(torch.from_numpy(np.stack(imgs)).to(device), 1 if no_delta else 0, init,
                         limit_lengths=limit)
    torch.cuda.synchronize(device)
    st = a.status.cpu().numpy()
    lens = a.codes_len.cpu().numpy()
    assert not a.flags & 0x200
    for f, img in enumerate(imgs):
        if deep[f] and not limit:
            assert st[f] == -3 and lens[f] == 0, (f, st[f], lens[f])
            continue
        assert st[f] == 0, (f, st[f])
        host = _host(mh, img, fmt)
        assert lens[f] == host.codes.size, f
        _same_frame(a.frame(f), host, init)
    return a


def test_full_level_lists_inside_a_batch(mh, device, chain_image, bigbridge):
    import torch
    from metalhuffman_amd.encoder import BatchEncoder
    imgs = [np.ascontiguousarray(bigbridge[:1024, :1024]), chain_image,
            np.ascontiguousarray(bigbridge[200:1224, 700:1724])]
    a = _check_batch(mh, device, BatchEncoder(1024, 1024, 3, device), imgs, "delta", True, [False, True, False])
    out = a.decode()
    torch.cuda.synchronize(device)
    assert torch.equal(out[..., :1024].cpu(), torch.from_numpy(np.stack(imgs)))


@pytest.fixture(scope="module")
def batch_calls():
    """Four calls of 64 histograms (kind, image) for 256 x 256 frames."""
    calls = []
    for call in range(4):
        hs = LH.batch_histograms(1000 + call)
        calls.append([(kind, LH.image_from_histogram(f, 256, 256, 64 * call + i)) for i, (kind, f) in enumerate(hs)])
    return calls


def test_batch_generator_is_mostly_deep(mh, batch_calls):
    """Over the four calls' 256 histograms at least half are rejected without the flag
    (the host codec's verdict), and every kind of frame is in every call."""
    deep = 0
    for frames in batch_calls:
        assert {k for k, _ in frames} == {"deep", "ordinary", "one", "two", "uniform"}
        for kind, img in frames:
            rejected = _host_rejects(mh, img, "delta")
            assert rejected == (kind == "deep"), kind
            deep += rejected
    assert deep >= 128


@pytest.mark.parametrize("call", range(4))
def test_batch_of_64_mixed_frames_in_one_call(mh, device, batch_calls, call):
    """64 frames (deep, ordinary, one-symbol, two-symbol, uniform) in one call: flagged,
    every status is MH_OK, every frame is the host's and the batch decodes to the 64
    images; the same encoder unflagged right afterwards rejects exactly the deep frames
    (-3, codes_len 0) and encodes the others exactly."""
    import torch
    from metalhuffman_amd.encoder import BatchEncoder
    frames = batch_calls[call]
    imgs = [img for _, img in frames]
    deep = [kind == "deep" for kind, _ in frames]
    enc = BatchEncoder(256, 256, 64, device)
    a = _check_batch(mh, device, enc, imgs, "delta", True, deep)
    out = a.decode()
    torch.cuda.synchronize(device)
    assert not a.tables.status.cpu().numpy().any()
    assert torch.equal(out[..., :256].cpu(), torch.from_numpy(np.stack(imgs)))
    _check_batch(mh, device, enc, imgs, "delta", False, deep)
