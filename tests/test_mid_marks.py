"""Mid-block marks on the host: the encoder's marks (mh_encode_frame_marks) equal the walk's
(mh_mid_marks) and the marks computed here from the picture and the code lengths; bits <= 512 and
the top byte is 0 everywhere. CPU only."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

import helpers as H
import mid_marks_helpers as M

NO_DELTA = 0x1


def _check(mh, img, flags=0, init=False, **kw):
    ef = mh.encode_frame(img, flags=flags, init_zero_delta=init, **kw)
    assert ef.mid_marks is not None and ef.mid_marks.dtype == np.uint32 and ef.mid_marks.shape == (ef.n_blocks,)
    walked = dataclasses.replace(ef, mid_marks=None).with_mid_marks().mid_marks
    want = M.expected_marks(img, ef.canon, bool(flags & NO_DELTA), init)
    assert np.array_equal(ef.mid_marks, want)
    assert np.array_equal(walked, want)
    assert int((ef.mid_marks & 0xFFFF).max()) <= 512 and not (ef.mid_marks >> 24).any()
    # the marks entry changes no other buffer of the frame
    plain = mh.encode_frame(img, flags=flags, init_zero_delta=init, header=ef.canon)
    assert plain.mid_marks is None
    assert np.array_equal(plain.codes, ef.codes) and np.array_equal(plain.block_offsets, ef.block_offsets)
    return ef


def test_bigbridge(mh, bigbridge):
    ef = _check(mh, bigbridge)
    assert ef.canon.max() == 14


def test_deep_codes(mh):
    ef = _check(mh, M.deep_code_image())
    assert ef.canon.max() >= 15


def test_long_first_halves(mh):
    """13-bit codes throughout under a foreign header (walk only): 416 bits to every mark."""
    d = np.random.default_rng(2).integers(0, 128, size=264 * 8, dtype=np.uint8)
    img = H.image_from_block_deltas(d, 264, 8)
    ef = mh.encode_frame(img, header=M.high_entropy_header())
    got = ef.with_mid_marks().mid_marks
    assert np.array_equal(got, M.expected_marks(img, ef.canon, False, False))
    assert ((got & 0xFFFF) == 32 * 13).all()


def test_flat8(mh):
    ef = _check(mh, M.flat8_deltas_image(64, 64, 5))
    assert ef.canon.min() == ef.canon.max() == 8
    assert ((ef.mid_marks & 0xFFFF) == 256).all()


@pytest.mark.parametrize("w,h", [(1, 1), (9, 9), (257, 17), (64, 40)])
@pytest.mark.parametrize("mode", ["delta", "no_delta", "block_init"])
def test_sizes_and_formats(mh, bigbridge, w, h, mode):
    img = np.ascontiguousarray(bigbridge[100:100 + h, 300:300 + w])
    ef = _check(mh, img, flags=NO_DELTA if mode == "no_delta" else 0, init=mode == "block_init")
    if mode == "no_delta":
        assert not (ef.mid_marks >> 16).any()


def test_golden_reference_buffers(mh):
    """Frames of the reference encoder (walk only): the hand-written frames of golden.json and the
    recorded histogram streams, whose symbols are known."""
    from metalhuffman_amd.codec import EncodedFrame
    n = 0
    for name, fx in H.golden()["small_frames"].items():
        w, h = fx["width"], fx["height"]
        img = np.array(fx["pixels"], np.uint8).reshape(h, w)
        canon = np.zeros(256, np.uint8)
        for s, ln in fx["canon"].items():
            canon[int(s)] = ln
        ef = EncodedFrame(w, h, canon, np.frombuffer(bytes.fromhex(fx["codes_hex"]), np.uint8),
                          np.array(fx["block_offsets"], np.uint32))
        got = ef.with_mid_marks().mid_marks
        assert np.array_equal(got, M.expected_marks(img, canon, False, False)), name
        n += 1
    ref = np.load(H.REF_HISTOGRAMS)
    for trial, sym in H.random_histogram_streams():
        if f"canon_{trial}" not in ref:
            continue
        canon, offs = ref[f"canon_{trial}"].astype(np.uint8), ref[f"offsets_{trial}"].astype(np.uint32)
        nb = sym.size // 64
        # a stream of whole blocks is a frame 8 pixels wide without deltas
        ef = EncodedFrame(8, 8 * nb, canon, ref[f"codes_{trial}"].astype(np.uint8), offs[:nb], None, NO_DELTA)
        got = ef.with_mid_marks().mid_marks
        assert np.array_equal(got, canon.astype(np.uint32)[sym.reshape(nb, 64)[:, :32]].sum(axis=1)), trial
        n += 1
    assert n > 20


def test_marks_of_an_edited_frame_are_dropped(mh, bigbridge):
    """Marks belong to the buffers they were made for: a frame given other codes, offsets or init
    bytes since has no valid marks, and with_mid_marks() makes them again."""
    ef = mh.encode_frame(np.ascontiguousarray(bigbridge[:40, :72]), init_zero_delta=True)
    assert ef.valid_mid_marks() is ef.mid_marks
    for field in ("codes", "block_offsets", "block_init"):
        other = getattr(ef, field).copy()
        other[1] ^= 1
        edited = dataclasses.replace(ef, **{field: other})
        assert edited.valid_mid_marks() is None
        again = edited.with_mid_marks()
        assert again.valid_mid_marks() is again.mid_marks
        assigned = dataclasses.replace(ef)
        assert assigned.valid_mid_marks() is not None
        setattr(assigned, field, other)
        assert assigned.valid_mid_marks() is None
    assert dataclasses.replace(ef, mid_marks=ef.mid_marks ^ 1).valid_mid_marks() is not None  # the marks themselves are free


def test_marked_entry_checks_its_arguments(mh):
    """mh_decode_marked refuses as mh_decode does, before any HIP call; marks off the 4-byte grid
    are MH_ERR_ALIGN with the other alignments (behind the NULL checks)."""
    import ctypes
    from metalhuffman_amd import _native as N
    fr = N.mh_frame(0x10000, 0x20000, 64, None, 0x30000, 0x40000, 256, None, None, N.mh_dims(8, 8, 1, 1), 1, 0)
    call = lambda marks, out, pitch=8: N.lib().mh_decode_marked(ctypes.byref(fr), marks, out, pitch, 64, None)
    assert call(0x50002, 0x60000) == -6                     # MH_ERR_ALIGN
    assert call(0x50002, None) == -1                        # MH_ERR_INVALID_ARG first
    assert call(0x50002, 0x60000, pitch=4) == -6            # with the other alignments
    fr.dims = N.mh_dims(8, 8, 2, 1)
    assert call(0x50002, 0x60000) == -2                     # MH_ERR_DIMS ahead of the alignments, as in mh_decode
    assert N.lib().mh_decode(ctypes.byref(fr), 0x60000, 8, 64, None) == -2


def test_band_and_set_layout_keep_marks_aligned(mh, bigbridge):
    """A band carries its blocks' marks; the set layout has none to misalign."""
    from metalhuffman_amd.codec import frame_set_layout
    ef = mh.encode_frame(np.ascontiguousarray(bigbridge[:64, :136]))
    band = ef.band(2, 5)
    assert np.array_equal(band.mid_marks, band.with_mid_marks().mid_marks)
    assert np.array_equal(band.mid_marks, ef.mid_marks[2 * ef.block_width: 5 * ef.block_width])
    assert "mid_marks" not in frame_set_layout([ef, band])._fields
