"""codec.frame_set_layout: the host packing of a frame SET (frames of different sizes) for
decoder.DeviceFrameSet and the mh_decode_set_* entries. CPU only."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

SIZES = ((8, 8), (9, 17), (64, 40), (520, 24))


def _image(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(100 + 2 * xx + yy + rng.normal(0, 5, (h, w)), 0, 255).astype(np.uint8)


def _frames(mh, **kw):
    imgs = [_image(w, h, 50 + i) for i, (w, h) in enumerate(SIZES)]
    return [mh.encode_frame(im, limit_lengths=True, **kw) for im in imgs], imgs


@pytest.mark.parametrize("kw", [{}, {"init_zero_delta": True}, {"flags": 1}])
def test_layout_of_four_sizes(mh, kw):
    efs, imgs = _frames(mh, **kw)
    lay = mh.frame_set_layout(efs)
    nbs = [-(-w // 8) * -(-h // 8) for w, h in SIZES]
    assert nbs == [1, 6, 40, 195]
    # first_block: the running sums of NB; the records are (first_block, width, height, 0)
    assert lay.geoms.dtype == np.uint32 and lay.geoms.shape == (4, 4)
    assert lay.geoms[:, 0].tolist() == [0, 1, 7, 47] == np.concatenate([[0], np.cumsum(nbs)[:-1]]).tolist()
    assert [tuple(g[1:3]) for g in lay.geoms.tolist()] == list(SIZES)
    assert not lay.geoms[:, 3].any()
    assert lay.total_blocks == sum(nbs) == lay.block_offsets.size
    assert lay.block_offsets.dtype == np.uint32
    # the maxima, taken separately
    assert (lay.width, lay.height) == (520, 40)
    assert lay.flags == kw.get("flags", 0)
    # code slots: n + 1 offsets, 16-byte aligned, each holding its frame's bytes and then zeros
    assert lay.code_offsets.dtype == np.int64 and lay.code_offsets.shape == (5,)
    assert lay.code_offsets[0] == 0 and not (lay.code_offsets % 16).any()
    assert lay.code_offsets[-1] == lay.codes.size
    for f, ef in enumerate(efs):
        a, b = int(lay.code_offsets[f]), int(lay.code_offsets[f + 1])
        assert ef.codes.size <= b - a < ef.codes.size + 16
        assert np.array_equal(lay.codes[a: a + ef.codes.size], ef.codes) and not lay.codes[a + ef.codes.size: b].any()
    assert (lay.block_init is not None) == bool(kw.get("init_zero_delta"))
    if lay.block_init is not None:
        assert lay.block_init.dtype == np.uint8 and lay.block_init.size == lay.total_blocks
    # every frame round-trips from its slices of the layout
    for f, (ef, img) in enumerate(zip(efs, imgs)):
        first, w, h, _ = (int(v) for v in lay.geoms[f])
        nb = nbs[f]
        back = dataclasses.replace(
            ef, width=w, height=h, block_offsets=lay.block_offsets[first: first + nb].copy(),
            codes=lay.codes[int(lay.code_offsets[f]): int(lay.code_offsets[f + 1])].copy(),
            block_init=None if lay.block_init is None else lay.block_init[first: first + nb].copy(), flags=lay.flags)
        assert np.array_equal(mh.decode_frame_cpu(back), img), f


def test_layout_of_one_frame_and_any_order(mh):
    efs, _ = _frames(mh)
    one = mh.frame_set_layout(efs[2:3])
    assert one.geoms.tolist() == [[0, 64, 40, 0]] and one.total_blocks == 40 and (one.width, one.height) == (64, 40)
    rev = mh.frame_set_layout(efs[::-1])
    assert rev.geoms[:, 0].tolist() == [0, 195, 235, 241] and (rev.width, rev.height) == (520, 40)
    assert mh.frame_set_layout(iter(efs)).total_blocks == 242      # any iterable


def test_layout_value_errors(mh):
    efs, imgs = _frames(mh)
    with pytest.raises(ValueError, match="no frames"):
        mh.frame_set_layout([])
    raw = mh.encode_frame(imgs[1], flags=mh.MH_FLAG_NO_DELTA, limit_lengths=True)
    with pytest.raises(ValueError, match="flags"):
        mh.frame_set_layout([efs[0], raw])
    init = mh.encode_frame(imgs[1], init_zero_delta=True, limit_lengths=True)
    with pytest.raises(ValueError, match="block_init"):
        mh.frame_set_layout([efs[0], init])
    with pytest.raises(ValueError, match="block_init"):
        mh.frame_set_layout([init, efs[0], init])
    with pytest.raises(ValueError, match="block offsets"):
        mh.frame_set_layout([dataclasses.replace(efs[1], width=17)])
    with pytest.raises(ValueError, match="outside"):
        mh.frame_set_layout([dataclasses.replace(efs[0], width=0)])


def test_device_frame_set_refuses_other_arguments():
    """The set entries take a DeviceFrameSet and nothing else (TypeError before any buffer is touched)."""
    import torch
    from metalhuffman_amd import decoder as D
    fr = D.DeviceFrames(64, 40, 1, torch.zeros(40, dtype=torch.int32), torch.zeros(16, dtype=torch.uint8), None)
    with pytest.raises(TypeError, match="DeviceFrameSet"):
        D.decode_set_crops(fr, None, [(0, 0, 0)], (8, 8))
    with pytest.raises(TypeError, match="DeviceFrameSet"):
        D.decode_set_crops_normalized_planes(fr, None, [(0, 0, 0)], (8, 8), torch.float16, [1.0], [0.0])


def _host_set():
    """A DeviceFrameSet description with host tensors: the size and a host list are validated before
    a buffer is looked at (as tests/test_crops_abi.py does for DeviceFrames)."""
    import torch
    from metalhuffman_amd import decoder as D
    z = torch.zeros(16, dtype=torch.uint8)
    return D.DeviceFrameSet(520, 40, 4, SIZES, 242, torch.zeros(242, dtype=torch.int32), z, None,
                            torch.zeros((4, 4), dtype=torch.int32))


@pytest.mark.parametrize("crops,size", [
    ([(4, 0, 0)], (8, 8)),                      # frame >= n_frames
    ([(0, 1, 0)], (8, 8)),                      # leaves its OWN 8 x 8 frame ...
    ([(3, 0, 0), (1, 2, 0)], (8, 8)),           # ... 9 x 17
    ([(2, 0, 33)], (8, 8)),
    ([(2, 0, 0)], (65, 8)),                     # wider than its frame, not than the set's widest
    ([(3, 0, 0)], (8, 25)),
    ([(0, -1, 0)], (8, 8)),
])
def test_host_lists_are_checked_against_each_crops_own_frame(crops, size):
    from metalhuffman_amd import decoder as D
    with pytest.raises(ValueError, match="crop"):
        D.decode_set_crops(_host_set(), None, crops, size)


@pytest.mark.parametrize("size", [(0, 8), (8, 0), (521, 8), (8, 41)])
def test_sizes_are_checked_against_the_sets_maxima(size):
    from metalhuffman_amd import decoder as D
    with pytest.raises(ValueError, match="does not fit"):
        D.decode_set_crops(_host_set(), None, [(3, 0, 0)], size)


def test_good_host_lists_pass_and_plane_rules_hold():
    import torch
    from metalhuffman_amd import decoder as D
    fs = _host_set()
    good = [(0, 0, 0), (1, 1, 9), (2, 56, 32), (3, 512, 16)]
    assert D._host_crops(fs, good, 8, 8).tolist() == [list(g) + [0] for g in good]
    with pytest.raises(ValueError, match="HIP device"):
        D.decode_set_crops(fs, None, good, (8, 8))
    f16 = torch.float16
    with pytest.raises(ValueError, match="n_planes"):
        D.decode_set_crops_normalized_planes(fs, None, good, (8, 8), f16, [1.0], [0.0], n_planes=2)
    with pytest.raises(ValueError, match="plane 1"):        # frames 0 and 1 differ in size
        D.decode_set_crops_normalized_planes(fs, None, [(0, 0, 0)], (8, 8), f16, [1.0, 1.0], [0.0, 0.0])
    with pytest.raises(ValueError, match="plane 1 would be frame 4"):
        D.decode_set_crops_normalized_planes(fs, None, [(3, 0, 0)], (8, 8), f16, [1.0, 1.0], [0.0, 0.0])
    with pytest.raises(ValueError, match="MH_CROP_MIRROR"):
        D.decode_set_crops_normalized_planes(fs, None, [(3, 0, 0, 1)], (9, 8), f16, [1.0], [0.0])
    with pytest.raises(ValueError, match="HIP device"):     # stride 0: one frame under two maps
        D.decode_set_crops_normalized_planes(fs, None, good, (8, 8), f16, [1.0, 2.0], [0.0, 0.5], plane_stride=0)
