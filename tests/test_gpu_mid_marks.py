"""GPU parity of the single-frame decode from mid-block marks (mh_decode_marked,
mh_decode_frame_marked_kernel).

Every case decodes one frame three ways through the C-ABI -- with its marks, without them, and
the encoder's input -- into a raster with canary rows above and below it and canary pitch padding
beside it, and compares the WHOLE buffers byte for byte. The shapes are the smallest at which the
lane mapping can go wrong: one lane pair, exactly one wave, a second wave with one live pair, a
32-block tile that does not end with a block row, partial edge blocks; then each table flavour,
each format, the unstaged fallback and the bench's frame once. The containment cases feed the
kernel marks it must not trust.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import pytest

import helpers as H
import mid_marks_helpers as M

pytestmark = pytest.mark.gpu

CANARY = 0x5A
GUARD = 8       # canary rows above and below the raster
PAD = 16        # canary bytes of pitch behind round_up(W, 8)
NO_DELTA, ANY_ORDER = 0x1, 0x4


def _crop(bigbridge, h, w, y0=100, x0=300):
    reps = (-(-(h + y0) // bigbridge.shape[0]), -(-(w + x0) // bigbridge.shape[1]))
    return np.ascontiguousarray(np.tile(bigbridge, reps)[y0:y0 + h, x0:x0 + w])


class Launch:
    """One frame on the device with its tables; decode() returns the whole guarded buffer."""

    def __init__(self, ef, device):
        from metalhuffman_amd import decoder as D
        assert ef.mid_marks is not None
        t1, t2 = ef.tables()
        self.ef, self.device = ef, device
        self.tabs = D.DeviceTables.upload(t1, t2, device, prepare_lut=True)
        self.fr = D.DeviceFrames.pack([ef], device)
        assert self.fr.mid_marks is not None and self.fr.frame_code_offsets is None
        self.w8 = (ef.width + 7) // 8 * 8
        self.pitch = self.w8 + PAD

    def decode(self, marks="own", extra_flags=0, buf=None, sync=True):
        import torch
        from metalhuffman_amd import _native as N, decoder as D
        h = self.ef.height
        if buf is None:
            buf = torch.full(((h + 2 * GUARD) * self.pitch,), CANARY, dtype=torch.uint8, device=self.device)
        st = D._frame_struct(self.fr, self.tabs, extra_flags)
        out = buf.data_ptr() + GUARD * self.pitch
        sp = torch.cuda.current_stream(self.device).cuda_stream
        if marks is None:
            rc = N.lib().mh_decode(ctypes.byref(st), out, self.pitch, h * self.pitch, sp)
        else:
            m = self.fr.mid_marks if isinstance(marks, str) else marks
            rc = N.lib().mh_decode_marked(ctypes.byref(st), m.data_ptr(), out, self.pitch, h * self.pitch, sp)
        N.check(rc, "mh_decode_marked")
        if not sync:
            return buf
        torch.cuda.synchronize(self.device)
        return buf.cpu().numpy().reshape(h + 2 * GUARD, self.pitch)

    def canaries_intact(self, got):
        h = self.ef.height
        return bool((got[:GUARD] == CANARY).all() and (got[GUARD + h:] == CANARY).all()
                    and (got[:, self.w8:] == CANARY).all())


def _parity(ef, img, device, extra_flags=0):
    L = Launch(ef, device)
    with_marks, without = L.decode("own", extra_flags), L.decode(None, extra_flags)
    assert L.canaries_intact(with_marks)
    assert np.array_equal(with_marks, without), "marked and unmarked decodes differ somewhere in the buffer"
    assert np.array_equal(with_marks[GUARD:GUARD + ef.height, :ef.width], img)
    return L


# (w, h): one block, one lane pair; exactly one wave; a second wave with one live pair; a tile
# boundary that does not fall at a block-row end (257 blocks per row); partial edge blocks
@pytest.mark.parametrize("wh", [(8, 8), (256, 8), (264, 8), (2056, 16), (1, 1), (9, 9), (257, 17)])
def test_shapes(mh, device, bigbridge, wh):
    w, h = wh
    img = _crop(bigbridge, h, w)
    _parity(mh.encode_frame(img), img, device)


def test_two_level_table(mh, device):
    """Codes of 15 and 16 bits: the 13-bit table with escapes, copied over the 14-bit one."""
    img = M.deep_code_image()
    ef = mh.encode_frame(img)
    assert ef.canon.max() >= 15
    _parity(ef, img, device)


@pytest.mark.parametrize("shift", [0, 3])
def test_flat8(mh, device, shift):
    """The flat 8-bit code's byte arithmetic from a mark, on and off the byte grid."""
    img = M.flat8_deltas_image(264, 16, 9)
    ef = mh.encode_frame(img)
    assert ef.canon.min() == ef.canon.max() == 8
    if shift:
        moved = H.shift_stream(ef, shift)  # new code bytes: the frame's marks are made again ...
        ef = moved.with_mid_marks()
        assert np.array_equal(ef.mid_marks, moved.mid_marks)  # ... and are the same words: relative to the offsets
    _parity(ef, img, device)


@pytest.mark.parametrize("mode", ["no_delta", "block_init"])
def test_formats(mh, device, bigbridge, mode):
    img = _crop(bigbridge, 24, 264)
    ef = mh.encode_frame(img, flags=NO_DELTA if mode == "no_delta" else 0, init_zero_delta=mode == "block_init")
    assert (ef.block_init is not None) == (mode == "block_init")
    _parity(ef, img, device)


def test_any_order_back_to_back(mh, device, bigbridge):
    """Four frames back to back into four rasters, every launch but the first MH_FLAG_ANY_ORDER."""
    import torch
    imgs = [_crop(bigbridge, 24, 264, y0=40 * k) for k in range(4)]
    launches = [Launch(mh.encode_frame(im), device) for im in imgs]
    bufs = [L.decode("own", ANY_ORDER if k else 0, sync=False) for k, L in enumerate(launches)]
    torch.cuda.synchronize(device)
    for L, b, im in zip(launches, bufs, imgs):
        got = b.cpu().numpy().reshape(-1, L.pitch)
        assert L.canaries_intact(got)
        assert np.array_equal(got, L.decode(None))
        assert np.array_equal(got[GUARD:GUARD + 24, :264], im)


def test_oversize_span_fallback(mh, device):
    """13 bits per symbol: the first wave's 32 blocks span 3328 bytes, over the marked kernel's
    staged window, so that wave decodes whole blocks on its lower lanes; the second wave (one
    block) stays on the marked path."""
    d = np.random.default_rng(2).integers(0, 128, size=264 * 8, dtype=np.uint8)
    img = H.image_from_block_deltas(d, 264, 8)
    ef = mh.encode_frame(img, header=M.high_entropy_header()).with_mid_marks()
    assert int(ef.block_offsets[32]) // 8 > 3072
    _parity(ef, img, device)


def test_bench_frame(mh, device, bigbridge):
    L = _parity(mh.encode_frame(bigbridge), bigbridge, device)
    # the Python path: decode() passes the marks of a packed frame
    from metalhuffman_amd import decoder as D
    out = D.decode(L.fr, L.tabs)
    ref = D.decode(dataclasses.replace(L.fr, mid_marks=None), L.tabs)
    assert np.array_equal(out.cpu().numpy(), ref.cpu().numpy())
    assert np.array_equal(out.cpu().numpy()[0, :, :2048], bigbridge)


@pytest.mark.parametrize("marks", ["ones", "random"])
@pytest.mark.parametrize("wh", [(264, 24), (257, 17)])
def test_untrusted_marks_are_contained(mh, device, bigbridge, marks, wh):
    """Marks of all ones, and seeded random words: the device clamps the bit count, so every
    canary stays intact, rows 0-3 of every block are correct (a wrong mark may spoil rows 4-7 of
    its own block only) and the launch completes without a status."""
    w, h = wh
    img = _crop(bigbridge, h, w)
    ef = mh.encode_frame(img)
    nb = ef.n_blocks
    words = (np.full(nb, 0xFFFFFFFF, np.uint32) if marks == "ones"
             else np.random.default_rng(17).integers(0, 2 ** 32, size=nb, dtype=np.uint64).astype(np.uint32))
    L = Launch(dataclasses.replace(ef, mid_marks=words), device)  # packed beside the offsets, as a producer's
    assert np.array_equal(L.fr.mid_marks.cpu().numpy().view(np.uint32), words)
    got = L.decode("own")
    assert L.canaries_intact(got)
    ref = L.decode(None)
    # the marks were consumed: with these words some block's rows 4-7 cannot equal the unmarked decode
    # (a launch that quietly ignored the marks would pass every parity case of this file)
    assert not np.array_equal(got, ref)
    top = (np.arange(h) % 8) < 4
    assert np.array_equal(got[GUARD:GUARD + h][top], ref[GUARD:GUARD + h][top])
    assert np.array_equal(got[GUARD:GUARD + h][top][:, :w], img[top])


def test_decode_passes_marks_only_while_they_are_bound(mh, device, bigbridge):
    """decoder.decode's one rule (DeviceFrames.marks_for): the marks go to the kernel while the
    object holds the tensors they were packed with and the tables are the frame's own code. Seen
    with marks that spoil rows 4-7: used, the raster differs from the picture; in each documented
    fallback -- unkeyed tables, foreign tables, a re-seated buffer -- the decode is mh_decode's."""
    import torch
    from metalhuffman_amd import decoder as D
    img = _crop(bigbridge, 24, 264)
    ef = mh.encode_frame(img)
    words = np.random.default_rng(23).integers(0, 2 ** 32, size=ef.n_blocks, dtype=np.uint64).astype(np.uint32)
    fr = D.DeviceFrames.pack([dataclasses.replace(ef, mid_marks=words)], device)
    t1, t2 = ef.tables()
    own = D.DeviceTables.upload(t1, t2, device)
    got = lambda frames, tables: D.decode(frames, tables)[0, :, :264].cpu().numpy()
    spoiled = got(fr, own)
    top = (np.arange(24) % 8) < 4
    assert np.array_equal(spoiled[top], img[top]) and not np.array_equal(spoiled, img)
    unkeyed = D.DeviceTables.from_canonical_header(torch.from_numpy(ef.canon).to(device), device)
    assert unkeyed.key is None and np.array_equal(got(fr, unkeyed), img)
    assert D.DeviceTables.from_canonical_header(ef.canon, device).key == own.key
    other = D.DeviceTables.upload(t1, t2, device)
    other.key ^= 1  # stands for another code's tables
    assert np.array_equal(got(fr, other), img)
    assert np.array_equal(got(dataclasses.replace(fr, codes=fr.codes.clone()), own), img)
    fr.block_offsets = fr.block_offsets.clone()
    assert np.array_equal(got(fr, own), img)
