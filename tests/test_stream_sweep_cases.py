"""The seeded stream sweep's cases (stream_helpers.sweep_case), checked on the CPU: over the default
range of both modes -- the cases test_gpu_stream_sweep.py runs -- every value of every axis occurs,
the two geometries and lengths the sweep is there for are hit, and every case builds with no frame
left out. A value the default range misses is mended in the generator's lists, never here."""
from __future__ import annotations

import pytest

import stream_helpers as SH

N = SH.SWEEP_DEFAULT_CASES
CASES = {m: [SH.sweep_case(m, i) for i in range(N)] for m in SH.MODES}

_BUILT = {}


def _built(mh, mode):
    """[(case, FrameSet, order)] of a mode's default range, built once."""
    if mode not in _BUILT:
        _BUILT[mode] = [(c,) + SH.sweep_frames(mh, c) for c in CASES[mode]]
    return _BUILT[mode]


def test_the_default_sweep_has_32_cases_a_mode():
    assert N == 32


def test_a_case_follows_from_its_name_alone():
    for m in SH.MODES:
        assert [SH.sweep_case(m, i) for i in range(N)] == CASES[m]
        assert len({c.describe() for c in CASES[m]}) == N
    assert SH.sweep_case("table", 3) != SH.sweep_case("headers", 3)


@pytest.mark.parametrize("mode", SH.MODES)
def test_every_value_of_every_axis_occurs(mode):
    cs = CASES[mode]
    for c in cs:
        assert 1 <= c.W <= 264 and 1 <= c.H <= 264 and c.mode == mode, c.describe()
    assert set(SH.EDGES) <= {c.W for c in cs} and set(SH.EDGES) <= {c.H for c in cs}
    assert {c.W for c in cs} == set(SH.SIZES) == {c.H for c in cs}
    assert {c.slots for c in cs} == {1, 2, 3, 4}
    assert {c.frames for c in cs} == set(range(2, 10))
    assert {c.fmt for c in cs} == set(SH.FORMATS)
    for axis in ("packed", "pinned", "owned", "graphs", "wait") + (("prepared",) if mode == "table" else ()):
        assert {getattr(c, axis) for c in cs} == {False, True}, axis


@pytest.mark.parametrize("mode", SH.MODES)
def test_the_axes_are_not_tied_to_each_other(mode):
    """Every pair of values of the host layout, the memory kind and the raster ownership occurs, and
    both launch kinds meet both host layouts and back-to-back submits."""
    cs = CASES[mode]
    assert len({(c.packed, c.pinned, c.owned) for c in cs}) == 8
    assert len({(c.graphs, c.packed) for c in cs}) == 4
    assert len({(c.graphs, c.wait) for c in cs}) == 4
    assert len({(c.fmt, c.packed) for c in cs}) == 6
    if mode == "table":
        assert len({(c.graphs, c.prepared) for c in cs}) == 4


@pytest.mark.parametrize("mode", SH.MODES)
def test_block_offsets_off_the_16_byte_grid(mode):
    """4 * NB % 16 != 0: the slot's offsets are padded, and the one-buffer layout has a gap."""
    hits = [c.i for c in CASES[mode] if 4 * c.nb % 16 != 0]
    assert len(hits) >= 1, hits


@pytest.mark.parametrize("mode", SH.MODES)
def test_every_case_builds_and_none_is_left_out(mh, mode):
    built = _built(mh, mode)
    assert len(built) == N                                   # the share of cases left out is zero
    for c, fs, order in built:
        assert len(fs.efs) == c.frames == len(fs.imgs) and sorted(order) == list(range(c.frames)), c.describe()
        for ef, im in zip(fs.efs, fs.imgs):
            assert (ef.width, ef.height) == (c.W, c.H) == im.shape[::-1]
            assert ef.canon.max() <= 16 and ef.codes.size >= SH.CODES_PAD
            assert (ef.block_init is not None) == (c.fmt == "init")
        if mode == "table":
            assert all((ef.canon == fs.efs[0].canon).all() for ef in fs.efs)


@pytest.mark.parametrize("mode", SH.MODES)
def test_a_slot_takes_a_short_frame_behind_a_long_one(mh, mode):
    """A slot whose second frame is under half its first frame's length: stale bytes behind the pad."""
    hits = [c.i for c, fs, order in _built(mh, mode) if SH.second_under_half(fs.sizes, order, c.slots)]
    assert len(hits) >= 1, hits
    for c, fs, order in _built(mh, mode):                    # and the order is the one the issue names
        s = c.slots
        assert fs.sizes[order[0]] == max(fs.sizes)
        if c.frames > s:
            assert fs.sizes[order[s]] == min(fs.sizes[i] for i in order[s:])


def test_frames_decode_to_their_images(mh, oracle):
    """The host's own check of a few built cases: the oracle's shader decode of every frame."""
    from metalhuffman_amd.codec import Huffman
    for mode in SH.MODES:
        for c, fs, _ in _built(mh, mode)[:6]:
            for ef, im in zip(fs.efs, fs.imgs):
                t1, t2 = Huffman.generateSplitLookupTables(ef.canon)
                got = oracle.decode_frame_shader(ef.block_offsets, ef.codes, t1, t2, c.W, c.H, block_init=ef.block_init,
                                                 delta=c.fmt != "no_delta")
                assert (got == im).all(), c.describe()
