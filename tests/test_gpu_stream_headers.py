"""The stream in table-per-frame mode (mh_stream_create_headers / HeaderFrameStream): frames
with unrelated histograms streamed from pinned host memory, each with its own 256-byte
canonical header, must arrive bit-exactly -- compared with the encoder inputs and the oracle --
with slots reused in turn, init bytes carried, a rejected header reported and harmless, and
the same result from graph replays (MH_STREAM_GRAPHS=1) as from direct launches."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import fibonacci_deltas

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _crops(mh, bigbridge, w, h, n, **kw):
    """n crops of a mirror-tiled BigBridge at n origins with n different histograms -> (images,
    frames). (Plain tiling makes every full-size crop a cyclic shift: 8 histograms in all.)"""
    from metalhuffman_amd import frames as F
    bh, bw = bigbridge.shape
    src = F.mirror_tile(bigbridge, 2 * bh, 2 * bw)
    imgs, efs = [], []
    for k in range(4 * n + 16):
        im = np.ascontiguousarray(src[37 * k % bh:, 101 * k % bw:][:h, :w])
        try:
            efs.append(mh.encode_frame(im, **kw))
        except mh.MHError as e:
            assert e.status == -3
            continue
        imgs.append(im)
        if len(imgs) == n:
            return imgs, efs
    raise AssertionError("too few encodable crops")


def _host(ef, packed):
    """Pinned (header, codes, offsets): views of one buffer in slot layout, or three buffers."""
    import torch
    from metalhuffman_amd.stream import pinned_frame_with_header
    if packed:
        return pinned_frame_with_header(ef)
    return (torch.from_numpy(np.ascontiguousarray(ef.canon, np.uint8)).pin_memory(),
            torch.from_numpy(np.ascontiguousarray(ef.codes)).pin_memory(),
            torch.from_numpy(np.ascontiguousarray(ef.block_offsets, np.uint32).view(np.int32)).pin_memory())


def _run(mh, oracle, device, imgs, efs, slots, packed, init_zero=False, oracle_frames=()):
    import torch
    from metalhuffman_amd.stream import HeaderFrameStream
    h, w = imgs[0].shape
    fs = HeaderFrameStream(w, h, max(ef.codes.size for ef in efs), slots=slots, block_init=init_zero, device=device)
    hosts = [_host(ef, packed) for ef in efs]
    inits = [torch.from_numpy(ef.block_init).pin_memory() for ef in efs] if init_zero else None

    def check(j, sj):
        assert fs.slot_status(sj) == 0, j
        got = fs.output(sj)[:, :w].cpu().numpy()
        assert np.array_equal(got, imgs[j]), j
        if j in oracle_frames:
            t1, t2 = efs[j].tables()
            assert np.array_equal(got, oracle.decode_frame_shader(efs[j].block_offsets, efs[j].codes, t1, t2, w, h,
                                                                  block_init=efs[j].block_init)), j
        assert fs.slot_time_ms(sj) > 0

    pending = []
    for i, (hd, c, o) in enumerate(hosts):
        pending.append((i, fs.submit(hd, c, o, inits[i] if init_zero else None)))
        assert pending[-1][1] == i % slots
        if len(pending) == slots:          # oldest frame: wait, check before its slot is reused
            j, sj = pending.pop(0)
            fs.wait(sj)
            check(j, sj)
    fs.synchronize()
    for j, sj in pending:
        check(j, sj)
    fs.close()


def test_seven_headers_three_slots_init_bytes(mh, oracle, device, bigbridge):
    """7 crops of 1000 x 768 with 7 distinct headers through 3 slots, with init bytes; each is
    checked before its slot is reused."""
    imgs, efs = _crops(mh, bigbridge, 1000, 768, 7, init_zero_delta=True)
    assert len({ef.canon.tobytes() for ef in efs}) == 7
    _run(mh, oracle, device, imgs, efs, slots=3, packed=True, init_zero=True, oracle_frames=(3,))


@pytest.mark.parametrize("packed", [True, False], ids=["one_dma", "separate_buffers"])
def test_ten_frames_two_slots_both_host_layouts(mh, oracle, device, bigbridge, packed):
    """10 frames of 2048 x 1536 through 2 slots: natural crops with distinct headers and one
    uniform-random frame (the flat 8-bit identity code: the byte-arithmetic path, no table)."""
    from metalhuffman_amd import frames as F
    imgs, efs = _crops(mh, bigbridge, 2048, 1536, 9)
    assert len({ef.canon.tobytes() for ef in efs}) == 9
    rnd = F.uniform_random(1536, 2048, 5)
    imgs.insert(4, rnd)
    efs.insert(4, mh.encode_frame(rnd))
    assert (efs[4].canon == 8).all()
    _run(mh, oracle, device, imgs, efs, slots=2, packed=packed, oracle_frames=(5,))


def test_rejected_header_mid_sequence(mh, device, bigbridge):
    """A too-long header submitted mid-sequence into caller-owned outputs prefilled with a
    pattern (creating the stream leaves them alone): its slot_status is -3 and its raster keeps
    what it held; the next frame into the same slot is exact, with status 0."""
    import torch
    from metalhuffman_amd import _native as N
    from metalhuffman_amd.stream import HeaderFrameStream
    w, h = 520, 264
    imgs, efs = _crops(mh, bigbridge, w, h, 4)
    too_long = np.zeros(256, np.uint8)
    freq = np.bincount(fibonacci_deltas(19, 65536, seed=2), minlength=256).astype(np.uint64)
    assert N.lib().mh_code_lengths(freq.ctypes.data_as(N._u64p), too_long.ctypes.data_as(N._u8p)) == -3
    pattern = ((np.arange(h * w, dtype=np.uint32) * 167 + 13) & 0xFF).astype(np.uint8).reshape(h, w)
    outs = [torch.from_numpy(pattern.copy()).to(device) for _ in range(2)]
    fs = HeaderFrameStream(w, h, max(ef.codes.size for ef in efs), slots=2, device=device, outputs=outs)
    fs.synchronize()
    torch.cuda.synchronize(device)
    assert all(np.array_equal(o.cpu().numpy(), pattern) for o in outs)
    assert fs.slot_status(0) == 0 and fs.slot_status(1) == 0     # unused slots
    hosts = [_host(ef, True) for ef in efs]
    bad = (torch.from_numpy(too_long).pin_memory(),) + hosts[1][1:]
    assert fs.submit(*hosts[0]) == 0
    assert fs.submit(*bad) == 1                                  # slot 1 still holds the pattern
    assert fs.submit(*hosts[2]) == 0
    assert fs.slot_status(1) == -3
    assert np.array_equal(fs.output(1).cpu().numpy(), pattern)
    assert fs.slot_status(0) == 0 and np.array_equal(fs.output(0).cpu().numpy(), imgs[2])
    assert fs.submit(*hosts[3]) == 1
    assert fs.slot_status(1) == 0 and np.array_equal(fs.output(1).cpu().numpy(), imgs[3])
    # the table-mode submit is refused on this stream
    import ctypes
    slot = ctypes.c_uint32(9)
    assert N.lib().mh_stream_submit(fs._h, hosts[0][1].data_ptr(), hosts[0][1].numel(), hosts[0][2].data_ptr(), None,
                                    ctypes.byref(slot)) == -1
    fs.close()


_CHILD = """
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
import metalhuffman_amd as mh
from metalhuffman_amd import frames as F
from metalhuffman_amd.stream import HeaderFrameStream, pinned_frame_with_header
src = F.bigbridge()
dev = torch.device("cuda:0")
w, h = 1000, 520
imgs = [np.ascontiguousarray(src[40 * k: 40 * k + h, 90 * k: 90 * k + w]) for k in range(5)]
efs = [mh.encode_frame(im) for im in imgs]
assert len({{ef.canon.tobytes() for ef in efs}}) == 5
fs = HeaderFrameStream(w, h, max(ef.codes.size for ef in efs), slots=2, device=dev)
hosts = [pinned_frame_with_header(ef) for ef in efs]
for i, hst in enumerate(hosts):
    s = fs.submit(*hst)
    assert fs.slot_status(s) == 0
    assert np.array_equal(fs.output(s)[:, :w].cpu().numpy(), imgs[i]), i
fs.close()
print("child ok")
"""


@pytest.mark.parametrize("graphs", ["0", "1"])
def test_graph_replays_and_direct_launches_decode_the_same(mh, device, graphs):
    """MH_STREAM_GRAPHS=0 (direct launches, also the header-mode default) and =1 (per-slot graph
    replays), each in a child process (the variable is read when a stream is created; the child
    starts fresh)."""
    env = dict(os.environ, MH_STREAM_GRAPHS=graphs)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
