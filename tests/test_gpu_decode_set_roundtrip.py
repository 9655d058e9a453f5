"""encode set -> tables -> decode set, closed on the device: encoder.encode_set_async(...).decode() and
encoder.encode_image_set_async(...).decode() on three small images of different sizes give back the
input planes, each at its own size, in one decode launch. Between the encode call and the decode call's
return nothing reads the device: Tensor.cpu / .item / .tolist / .numpy, torch.cuda.synchronize and
Stream.synchronize are counted through the API and must not be called before the final comparison."""
from __future__ import annotations

import contextlib

import numpy as np
import pytest

import set_helpers as SH

pytestmark = pytest.mark.gpu

SIZES = ((200, 120), (97, 61), (520, 72))   # (W, H): 375, 104 and 585 blocks; 520 x 72 has ten tiles


@contextlib.contextmanager
def no_host_reads(monkeypatch):
    """Counts every call that would wait for the device or copy from it; the block must make none."""
    import torch
    calls = []

    def counted(m, owner, name):
        real = getattr(owner, name)

        def wrapper(*a, **kw):
            calls.append(f"{owner.__name__}.{name}")
            return real(*a, **kw)
        m.setattr(owner, name, wrapper)
    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy"):
            counted(m, torch.Tensor, name)
        counted(m, torch.cuda, "synchronize")
        counted(m, torch.cuda.Stream, "synchronize")
        yield calls
    assert calls == [], f"host reads between encode and decode: {calls}"


def _planes(device):
    import torch
    imgs = [SH.image(w, h, 77 + i) for i, (w, h) in enumerate(SIZES)]
    return imgs, [torch.from_numpy(im).to(device) for im in imgs]


@pytest.mark.parametrize("side_stream", [False, True], ids=["current_stream", "side_stream"])
def test_encode_set_async_decode(mh, device, monkeypatch, side_stream):
    import torch
    from metalhuffman_amd import encoder as E
    imgs, planes = _planes(device)
    stream = torch.cuda.Stream(device) if side_stream else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(device))
    torch.cuda.synchronize(device)
    with no_host_reads(monkeypatch):
        es = E.encode_set_async(planes, stream=stream, limit_lengths=True)
        frames, status = es.decode(status=True, stream=stream)
    torch.cuda.synchronize(device)
    assert es.status.cpu().tolist() == [0, 0, 0] and status.cpu().tolist() == [0, 0, 0]
    assert len(frames) == 3
    for f, (got, im) in enumerate(zip(frames, imgs)):
        assert tuple(got.shape) == im.shape and got.dtype is torch.uint8, f
        assert np.array_equal(got.cpu().numpy(), im), f
    # again on the same object: the frame set and its uploaded plan are kept, the tables rebuilt
    fs = es.decoded_set
    with no_host_reads(monkeypatch):
        again = es.decode(stream=stream)
    torch.cuda.synchronize(device)
    assert es.decoded_set is fs and all(np.array_equal(g.cpu().numpy(), im) for g, im in zip(again, imgs))


def test_encode_image_set_async_decode(mh, device, monkeypatch):
    """Interleaved RGB images of three sizes: frame i * 3 + c is plane c of image i; with block_init."""
    import torch
    from metalhuffman_amd import encoder as E
    rgb = [np.stack([SH.image(w, h, 300 + 10 * i + c) for c in range(3)], axis=2) for i, (w, h) in enumerate(SIZES)]
    images = [torch.from_numpy(np.ascontiguousarray(im)).to(device) for im in rgb]
    torch.cuda.synchronize(device)
    with no_host_reads(monkeypatch):
        es = E.encode_image_set_async(images, init_zero_delta=True, limit_lengths=True)
        frames = es.decode()
    torch.cuda.synchronize(device)
    assert es.status.cpu().tolist() == [0] * 9 and es.tables.status.cpu().tolist() == [0] * 9
    assert len(frames) == 9
    for i, im in enumerate(rgb):
        for c in range(3):
            got = frames[3 * i + c].cpu().numpy()
            assert got.shape == im.shape[:2] and np.array_equal(got, im[:, :, c]), (i, c)


def test_a_rejected_frame_is_skipped_on_the_device(mh, device, monkeypatch):
    """A slot too small for its frame: the encoder rejects it (MH_ERR_CAPACITY), the table set carries the
    word, the decode skips the frame -- its view keeps the zeros it was allocated with and its status
    word is the encoder's -- and the other two frames are exact; all without a host read in between."""
    import torch
    from metalhuffman_amd import encoder as E
    imgs, planes = _planes(device)
    slots = [E.default_slot_bytes(w, h) for w, h in SIZES]
    slots[1] = 64
    torch.cuda.synchronize(device)
    with no_host_reads(monkeypatch):
        es = E.encode_set_async(planes, limit_lengths=True, slot_bytes=slots)
        frames, status = es.decode(status=True)
    torch.cuda.synchronize(device)
    assert es.status.cpu().tolist() == [0, -4, 0] and status.cpu().tolist() == [0, -4, 0]
    assert np.array_equal(frames[0].cpu().numpy(), imgs[0]) and np.array_equal(frames[2].cpu().numpy(), imgs[2])
    assert not frames[1].cpu().numpy().any()
