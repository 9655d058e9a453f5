"""mh_encode_set_device_async through the raw ABI into guard-filled outputs (set_encode_helpers.py),
against mh.encode_frame frame by frame: header, codes, pad bytes, nothing behind them, lengths, block
offsets, init bytes, d_frame_code_offsets, status words and every guard byte. The sets sit on the tile
(256 blocks) and pack-unit (4 tiles) edges, in the order large, small, large."""
from __future__ import annotations

import numpy as np
import pytest

import limit_helpers as LH
import set_encode_helpers as SH
from encode_helpers import CAPACITY, LIMIT, NO_DELTA, OK, TOO_LONG

pytestmark = pytest.mark.gpu

FORMATS = {"delta": (0, False), "raw": (NO_DELTA, False), "delta_init": (0, True), "raw_init": (NO_DELTA, True)}
SETS = {"edges": SH.EDGE_SET, "one": [(264, 256)]}


@pytest.fixture(scope="module")
def edge_images(bigbridge):
    return {name: SH.images(bigbridge, sizes) for name, sizes in SETS.items()}


@pytest.mark.parametrize("aligned", [False, True], ids=["bytes", "dwords"])
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("which", list(SETS))
def test_set_matches_the_host_codec(mh, device, edge_images, which, fmt, aligned):
    from metalhuffman_amd import _native as N
    flags, init_zero = FORMATS[fmt]
    imgs = edge_images[which]
    srcs = SH.planar_sources(device, imgs, aligned)
    r, _ = SH.run(mh, device, imgs, srcs, flags=flags, init_zero=init_zero)
    assert r.plan.totals.fetch_mode == (1 if aligned else N.MH_SET_FETCH_BYTES)
    exp = SH.expect(mh, imgs, r.caps, flags, init_zero)
    assert all(s == OK for s, _ in exp), [s for s, _ in exp]
    SH.check(r, exp)


def test_a_full_slot_in_the_middle_is_rejected_alone(mh, device, edge_images):
    """codes_cap 16 for a middle frame: status -4, its outputs untouched, its neighbours -- of other
    sizes -- exact; and a slot of exactly round_up(codes_len, 4) rounded up to 16 is accepted."""
    imgs = edge_images["edges"]
    roomy = SH.expect(mh, imgs, [1 << 30] * len(imgs))
    caps = [SH.r16(SH.r4(ef.codes.size)) for _, ef in roomy]    # flush slots
    caps[2] = 16
    caps[4] = SH.roomy_cap(264, 256)
    for aligned in (False, True):
        r, _ = SH.run(mh, device, imgs, SH.planar_sources(device, imgs, aligned), caps=caps, init_zero=True)
        exp = SH.expect(mh, imgs, caps, 0, True)
        assert [s for s, _ in exp] == [OK, OK, CAPACITY, OK, OK, OK, OK]
        SH.check(r, exp)


def test_a_tree_deeper_than_16(mh, device, edge_images):
    """One frame of a Fibonacci histogram between natural neighbours: -3 without
    MH_ENCODE_LIMIT_LENGTHS, and with it the length-limited code (code_lengths_limited)."""
    deep = LH.image_from_histogram(LH.fib_histogram(20, 128 * 128, seed=4), 128, 128, seed=4)   # 256 blocks x 64 symbols
    imgs = [edge_images["edges"][1], deep, edge_images["edges"][3]]
    hist = LH.frame_histogram(deep)
    assert LH.huffman_depth(sorted(int(c) for c in hist if c)) > 16
    srcs = SH.planar_sources(device, imgs, True)
    r, ws = SH.run(mh, device, imgs, srcs)
    exp = SH.expect(mh, imgs, r.caps)
    assert [s for s, _ in exp] == [OK, TOO_LONG, OK]
    SH.check(r, exp)
    r, _ = SH.run(mh, device, imgs, srcs, flags=LIMIT, workspace=ws)
    exp = SH.expect(mh, imgs, r.caps, LIMIT)
    assert [s for s, _ in exp] == [OK, OK, OK]
    assert np.array_equal(exp[1][1].canon, mh.code_lengths_limited(hist, 16)) and int(exp[1][1].canon.max()) == 16
    SH.check(r, exp)


def test_two_calls_over_one_workspace(mh, device, edge_images):
    """A second, different set over the workspace the first one left behind."""
    imgs = edge_images["edges"]
    r, ws = SH.run(mh, device, imgs, SH.planar_sources(device, imgs, False), flags=NO_DELTA)
    SH.check(r, SH.expect(mh, imgs, r.caps, NO_DELTA))
    back = imgs[::-1][:5]
    r, _ = SH.run(mh, device, back, SH.planar_sources(device, back, True), init_zero=True, workspace=ws)
    SH.check(r, SH.expect(mh, back, r.caps, 0, True))


@pytest.mark.parametrize("pitch_extra", [0, 1], ids=["dwords", "bytes"])
@pytest.mark.parametrize("K", [3, 4])
def test_planes_of_interleaved_images(mh, device, bigbridge, K, pitch_extra):
    """Planes of K-channel HWC images of two sizes, each against the host codec on the de-interleaved
    plane: a 4-byte aligned pitch (dword loads), and a pitch of W * K + 1 (byte loads)."""
    from metalhuffman_amd import _native as N
    sizes = [(264, 120), (37, 50)]
    planes_of = [SH.images(bigbridge, [s] * K, seed=11 + 5 * i) for i, s in enumerate(sizes)]
    srcs = SH.interleaved_sources(device, planes_of, K, pitch_extra)
    imgs = [p for planes in planes_of for p in planes]
    r, _ = SH.run(mh, device, imgs, srcs, init_zero=True)
    assert r.plan.totals.fetch_mode == (K if pitch_extra == 0 else N.MH_SET_FETCH_BYTES)
    exp = SH.expect(mh, imgs, r.caps, 0, True)
    assert all(s == OK for s, _ in exp)
    SH.check(r, exp)
