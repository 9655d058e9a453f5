"""The GPU encoders through their C ABI (encode_helpers.run) where the Python wrappers never take
them: pixels at any byte offset and frame stride inside garbage (the byte-load instances at widths
that are multiples of 8, the 16-byte pair loads at addresses that are only 8-byte aligned), the
stride rules, output pointers at their weakest legal alignment, the capacity rule at its edge for
every residue of the byte count, widths and block counts on the kernels' thresholds, and the
dimension limits. Every output sits inside guards of which every byte is checked, every call is
made twice over one workspace, the standard is the host codec byte for byte, and every accepted
case is decoded back on the device (encode_helpers.check, round_trip)."""
from __future__ import annotations

import numpy as np
import pytest

import encode_helpers as EH
from encode_helpers import Layout

pytestmark = pytest.mark.gpu

H = 40
# W = 48: an even width in blocks (enc_pack_wave_kernel<true, true>, the 16-byte pair loads, where
# the frame address allows 8-byte loads); 24: odd (<true, false>); 43: W % 8 != 0 (<false, false>)
WIDTHS = (48, 24, 43)


def _layouts(w):
    """name -> Layout; "dense" is the control. delta 8 / stride + 8: 8-byte loads at addresses that
    are 8 mod 16; delta 1, 4, 7 and stride + 3: byte loads whatever the width; stride + 4112: a
    page of garbage between frames."""
    px = w * H
    return {"dense": Layout(), "delta 8": Layout(delta=8), "delta 1": Layout(delta=1), "delta 4": Layout(delta=4),
            "delta 7": Layout(delta=7), "stride + 8": Layout(stride=px + 8), "stride + 3": Layout(stride=px + 3),
            "stride + 4112": Layout(stride=px + 4112), "delta 8, stride + 8": Layout(delta=8, stride=px + 8)}


def _header(entry, imgs, flags=0, init_zero=False):
    return EH.supplied_header(imgs, flags, init_zero) if entry == "shared_supplied" else None


def _same_outputs(r, control, name):
    for k in control.host:
        assert np.array_equal(r.host[k], control.host[k]), f"{name}: {k} differs from the dense layout's"


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("entry", EH.ENTRIES)
def test_pixel_layouts(mh, device, bigbridge, entry, w):
    """Three frames at every layout: the host codec's bytes, and the dense layout's outputs byte for
    byte (the single-frame entry takes the strides too: its three calls read frames at them)."""
    imgs = EH.natural_frames(bigbridge, w, H, 3, seed=w)
    header = _header(entry, imgs)
    control = None
    for name, lay in _layouts(w).items():
        r, exp = EH.run_checked(mh, device, entry, imgs, layout=lay, header=header)
        assert all(s == EH.OK for s, _ in exp.frames)
        control = control or r
        _same_outputs(r, control, name)


@pytest.mark.parametrize("delta", [0, 8, 3])
def test_four_kernel_path_below_32_blocks_wide(mh, device, bigbridge, delta):
    """248 x 16,928: 31 x 2,116 = 65,596 blocks, 513 tiles of kCodeTile -- one past kFusedMaxTiles,
    so split, tree, scan and pack run as four kernels, on a frame narrower than group_row's 32."""
    w, h = 248, 16928
    assert -(-(31 * 2116) // EH.K_CODE_TILE) == EH.K_FUSED_MAX_TILES + 1 and EH.blocks(w, h) == (31, 2116)
    imgs = EH.natural_frames(bigbridge, w, h, 1, seed=5)
    _, exp = EH.run_checked(mh, device, "single", imgs, layout=Layout(delta=delta))
    assert exp.frames[0][0] == EH.OK


@pytest.mark.parametrize("entry", EH.BATCHED)
def test_stride_rules(mh, device, bigbridge, entry):
    """gray_frame_stride < W * H with two frames: MH_ERR_CAPACITY before any launch, whatever the
    workspace (four times the need, so only the stride rule can answer); one frame: any stride."""
    w = 48
    imgs = EH.natural_frames(bigbridge, w, H, 2, seed=9)
    need = EH.workspace_bytes(mh, entry, w, H, 2)
    runs = EH.run(mh, device, entry, imgs, header=_header(entry, imgs), told_stride=w * H - 1, ws_bytes=4 * need,
                  launches=False)
    EH.check_untouched(runs, EH.CAPACITY)
    one = imgs[:1]
    for stride in (0, 1, w * H - 1):
        _, exp = EH.run_checked(mh, device, entry, one, layout=Layout(stride=stride), header=_header(entry, one))
        assert exp.frames[0][0] == EH.OK


@pytest.mark.parametrize("init_zero", [False, True])
@pytest.mark.parametrize("no_delta", [False, True])
@pytest.mark.parametrize("entry", EH.ENTRIES)
def test_outputs_at_their_weakest_alignment(mh, device, bigbridge, entry, no_delta, init_zero):
    """d_codes at 4, 8 and 12 mod 16 (the single-frame entry; its slots then sit at every word
    residue), d_block_init and the header(s) at odd addresses, d_block_offsets at 4 mod 16, the
    status words at 4 mod 8 -- the same bytes as at offset 0."""
    flags = EH.NO_DELTA if no_delta else 0
    for w in (48, 43):
        imgs = EH.natural_frames(bigbridge, w, H, 3, seed=20 + w)
        header = _header(entry, imgs, flags, init_zero)
        control, _ = EH.run_checked(mh, device, entry, imgs, flags=flags, init_zero=init_zero, header=header)
        for codes_off in ((4, 8, 12) if entry == "single" else (16,)):
            lay = Layout(codes_off=codes_off, offs_off=4, init_off=1, canon_off=3, len_off=8, status_off=4)
            r, exp = EH.run_checked(mh, device, entry, imgs, flags=flags, init_zero=init_zero, layout=lay,
                                    header=header)
            assert all(s == EH.OK for s, _ in exp.frames)
            _same_outputs(r, control, f"W {w}, d_codes at {codes_off} mod 16")


# ---- the capacity rule at its edge ----------------------------------------------------------------------

def _crops(bigbridge):
    """64 seeded 72 x 40 crops of the picture."""
    return [np.ascontiguousarray(bigbridge[53 * i % 1400: 53 * i % 1400 + 40, 37 * i % 1900: 37 * i % 1900 + 72])
            for i in range(64)]


def _residue_classes(mh, bigbridge):
    """-> ({codes_len % 4: crop}, {round_up(codes_len, 4) % 16: crop}); all eight classes are there."""
    mod4, mod16 = {}, {}
    for im in _crops(bigbridge):
        k = mh.encode_frame(im).codes.size
        mod4.setdefault(k % 4, im)
        mod16.setdefault(EH.r4(k) % 16, im)
    assert sorted(mod4) == [0, 1, 2, 3] and sorted(mod16) == [0, 4, 8, 12], (sorted(mod4), sorted(mod16))
    return mod4, mod16


def test_single_frame_capacity_edge(mh, device, bigbridge):
    """codes_cap = round_up(codes_len, 4): every byte, and the guard that starts at d_codes +
    codes_cap intact; four bytes less: MH_ERR_CAPACITY and nothing written. For every residue of
    codes_len mod 4 and of the rounded count mod 16 (the packer stores quads). A codes_cap that is no
    multiple of 4 counts as it stands: codes_len itself, where that is below its rounded value, is
    MH_ERR_CAPACITY too."""
    mod4, mod16 = _residue_classes(mh, bigbridge)
    for im in list(mod4.values()) + list(mod16.values()):
        fit = EH.r4(mh.encode_frame(im).codes.size)
        for codes_off in (0, 4):
            _, exp = EH.run_checked(mh, device, "single", [im], slot=fit, layout=Layout(codes_off=codes_off))
            assert exp.frames[0][0] == EH.OK
            _, exp = EH.run_checked(mh, device, "single", [im], slot=fit - 4, layout=Layout(codes_off=codes_off))
            assert exp.frames[0][0] == EH.CAPACITY
        k = mh.encode_frame(im).codes.size
        if k % 4:
            _, exp = EH.run_checked(mh, device, "single", [im], slot=fit, cap=k)
            assert exp.frames[0][0] == EH.CAPACITY


def _trio(mh, entry, bigbridge):
    """Three crops, the middle one with round_up(codes_len, 4) % 16 == 0 under the entry's table and
    both neighbours at least 16 bytes shorter -> (images, header or None, the middle frame's count)."""
    crops = _crops(bigbridge)
    own = [mh.encode_frame(im).codes.size for im in crops]
    a, b = (crops[i] for i in np.argsort(own)[:2])          # the two shortest
    for mid in crops:
        imgs = [a, mid, b]
        if mid is a or mid is b:
            continue
        header = _header(entry, imgs)
        exp = EH.expect(mh, entry, imgs, header=header)
        k = [EH.r4(ef.codes.size) for _, ef in exp.frames]
        if k[1] % 16 == 0 and k[0] <= k[1] - 16 and k[2] <= k[1] - 16:
            return imgs, header, k[1]
    raise AssertionError("no crop of the 64 gives the middle frame a count that is a multiple of 16")


@pytest.mark.parametrize("entry", EH.BATCHED)
def test_batched_capacity_edge(mh, device, bigbridge, entry):
    """codes_frame_stride = the middle frame's rounded count: it fits exactly, the slots flush
    against each other; 16 less: the middle frame alone is MH_ERR_CAPACITY, its slot and offsets
    untouched, its neighbours exact (and d_header_status stays MH_OK)."""
    imgs, header, fit = _trio(mh, entry, bigbridge)
    _, exp = EH.run_checked(mh, device, entry, imgs, slot=fit, header=header)
    assert [s for s, _ in exp.frames] == [EH.OK] * 3 and exp.header_status == EH.OK
    _, exp = EH.run_checked(mh, device, entry, imgs, slot=fit - 16, header=header)
    assert [s for s, _ in exp.frames] == [EH.OK, EH.CAPACITY, EH.OK] and exp.header_status == EH.OK


# ---- widths and block counts on the thresholds (encode_helpers.threshold_shapes) ------------------------

@pytest.mark.parametrize("bw", EH.THRESHOLD_WIDTHS)
@pytest.mark.parametrize("entry", EH.ENTRIES)
def test_width_and_tile_thresholds(mh, device, bigbridge, entry, bw):
    """Widths in blocks around kStepBlocks = 16, group_row's 32 and kCodeTile = 128 / kBatchTile =
    256, each ending on the block and one pixel into the last one, at heights that put the block
    count on, just below and just above one packer step (16), one tile (128 fused, 256 batched) and
    one packer workgroup (kPackWaves = 4 tiles). The pixels sit 8 bytes off a 16-byte boundary."""
    for w, h in EH.threshold_shapes(entry, bw):
        imgs = EH.accepted_frames(mh, entry, bigbridge, w, h, 1 if entry == "single" else 2, seed=bw)
        _, exp = EH.run_checked(mh, device, entry, imgs, layout=Layout(delta=8), header=_header(entry, imgs))
        assert all(s == EH.OK for s, _ in exp.frames), (w, h)


@pytest.mark.parametrize("h", [1536, 1537])
def test_shared_reduction_at_96_and_97_tiles(mh, device, bigbridge, h):
    """1024 x 1536 is 96 tiles a frame, one reduction workgroup of kReduceTiles; 1537 rows, 97."""
    bw, bh = EH.blocks(1024, h)
    assert -(-(bw * bh) // EH.K_BATCH_TILE) == (EH.K_REDUCE_TILES if h == 1536 else EH.K_REDUCE_TILES + 1)
    imgs = EH.accepted_frames(mh, "shared_built", bigbridge, 1024, h, 2, seed=h)
    _, exp = EH.run_checked(mh, device, "shared_built", imgs)
    assert all(s == EH.OK for s, _ in exp.frames)


@pytest.mark.parametrize("wh", [(65535, 11), (11, 65535), (65535, 8), (1, 65535), (65535, 1)])
@pytest.mark.parametrize("entry", EH.ENTRIES)
def test_dimension_limits(mh, device, bigbridge, entry, wh):
    """The u16 limits: 8,192 blocks of one row with W % 8 == 7 (byte loads), 8,192 block rows."""
    w, h = wh
    imgs = EH.accepted_frames(mh, entry, bigbridge, w, h, 1 if entry == "single" else 2, seed=w + h)
    _, exp = EH.run_checked(mh, device, entry, imgs, header=_header(entry, imgs))
    assert all(s == EH.OK for s, _ in exp.frames)
