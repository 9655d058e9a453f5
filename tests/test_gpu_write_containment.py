"""GPU write containment: every decode kernel stores only inside its frames' rasters.

include/metalhuffman.h: frame f, row y starts at d_out + f*out_frame_stride + y*out_pitch;
round_up(W, 8) bytes of every row y < H are written; "the rest of the pitch and rows >= H
are not touched". The kernels keep that promise without a bounds branch: every lane issues
eight unconditional 8-byte row stores per block, and dead lanes and rows >= H are dropped
only because their offset falls outside the tile's buffer descriptor (out_tile in
csrc/mh_decode.hip; the lane-pair diagnostic kernel has its own copy). An error of one block
row there changes no pixel -- it overwrites the caller's memory -- so each case here decodes
through the C-ABI into a raster laid out inside one pattern-filled buffer
(helpers.containment_plan) and then checks EVERY byte of it (helpers.check_containment,
itself tested in test_write_containment_cpu.py): the lead guard in front of d_out, the row
padding beyond round_up(W, 8), rows >= H, the gap between frames, the tail guard, and every
pixel against the oracle's decode_frame_shader.

Two geometries per case: `tight` (pitch = round_up(W, 8), stride = H*pitch, d_out 256-byte
aligned: a row >= H of frame f that is not dropped lands in rows 0..7 of frame f+1) and
`loose` (a pitch that is a multiple of 8 but not of 16, stride = H*pitch + 40, d_out 8- but
not 16-byte aligned).

Shapes: the smallest at which the addressing can go wrong. Every frame is encoded on its
full block grid and declared smaller (both edges cropped, same grid and table):
  A  grid 96x56 declared 93x50: 12x7 = 84 blocks = tile 0 (ends inside block row 5) + a tile
     of 20 live lanes; rows 50..55 must be dropped
  B  grid 24x40 declared 17x33: 3x5 = 15 blocks, one tile over five block rows, 49 dead
     lanes; rows 33..39 must be dropped. (960 symbols cannot carry a 14-bit Huffman code --
     the Fibonacci histogram that needs one has 1,596 -- so B's frames are the first five
     block rows, EncodedFrame.band(0, 5), of 24x320 frames: the same grid, a 14-bit table)
  C  grid 256x32 declared 250x27: 128 blocks = 2 tiles; kind X has every rare delta in
     tile 0 (its span, 4,591 B, exceeds the 4,352-B LDS stage: decode_halves), kind Y in
     tile 1; one histogram, one table; batches alternate X, Y

Each case's id names the kernel, the shape, the table flavour and the frame count; the
test asserts the tile count that routes the launch (launch() in mh_decode.hip: a prepared
table and tiles <= 4 x CUs -> the small kernels, else mh_decode_kernel) and the flavour's
precondition on the canonical lengths, so the coverage can be read without a profiler.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import pytest

from helpers import (check_containment, containment_plan, fibonacci_deltas, image_from_block_deltas,
                     shift_stream)

pytestmark = pytest.mark.gpu

# shape: (grid W, grid H, declared W, declared H)
SHAPES = {"A": (96, 56, 93, 50), "B": (24, 40, 17, 33), "C": (256, 32, 250, 27)}
N_DISTINCT = 7       # distinct frames per set; larger batches cycle through them
STAGE_BYTES = 4352   # kStageBytes (mh_decode.hip)


def _oracle_decode(O, ef):
    t1, t2 = ef.tables()
    return O.decode_frame_shader(ef.block_offsets, ef.codes, t1, t2, ef.width, ef.height,
                                 block_init=ef.block_init, delta=not (ef.flags & 1))


def _lens(ef):
    L = ef.canon[ef.canon > 0]
    return int(L.min()), int(L.max()), int(L.size)


def _flat_symbols(n_values, nb, seed):
    """Every value 0..n_values-1 exactly nb*64/n_values times, shuffled: one code length."""
    assert (nb * 64) % n_values == 0
    d = np.repeat(np.arange(n_values, dtype=np.uint8), nb * 64 // n_values)
    np.random.default_rng(seed).shuffle(d)
    return d


def _build_set(mh, shape, flavour):
    """-> list of (EncodedFrame declared W x H, the image's H x W crop): frames of one table."""
    from metalhuffman_amd import frames as F
    gw, gh, W, H = SHAPES[shape]
    nb = (gw // 8) * (gh // 8)
    kw = {}
    if shape == "C":
        assert flavour == "oversize"
        rare = np.random.default_rng(0).integers(1, 256, size=64 * 64, dtype=np.uint8)
        imgs = []
        for kind in range(2):  # X: the rare deltas in blocks 0..63, Y: in blocks 64..127
            d = np.zeros(nb * 64, np.uint8)
            d[kind * 4096: kind * 4096 + 4096] = rare
            imgs.append(image_from_block_deltas(d, gw, gh))
        efs = [mh.encode_frame(im) for im in imgs]
        o = efs[0].block_offsets.astype(np.int64)
        assert (o[64] - o[0]) // 8 > STAGE_BYTES                               # X: tile 0 oversize
        o = efs[1].block_offsets.astype(np.int64)
        assert (8 * efs[1].payload_bytes - o[64]) // 8 > STAGE_BYTES and (o[64] - o[0]) // 8 < STAGE_BYTES
        assert _lens(efs[0])[1] <= 13                                           # escape-free step
    elif shape == "B":
        # a 24 x 320 frame carries the 14-bit table; its first five block rows are the 24 x 40 grid
        assert flavour == "general14"
        base = image_from_block_deltas(fibonacci_deltas(15, 3 * 40 * 64, seed=1), gw, 8 * gh)
        imgs = [F.block_shuffle(base, 40 + s) for s in range(N_DISTINCT)]
        efs = [mh.encode_frame(im).band(0, gh // 8) for im in imgs]
        imgs = [im[:gh] for im in imgs]
        assert _lens(efs[0])[1] == 14
    else:
        if flavour in ("general", "general_nodelta"):
            d, want = fibonacci_deltas(17, nb * 64, seed=1), (1, 16, 17)
        elif flavour in ("general14", "general14_init"):
            d, want = fibonacci_deltas(15, nb * 64, seed=1), (1, 14, 15)
        elif flavour == "noesc":
            d, want = fibonacci_deltas(14, nb * 64, seed=1), (1, 13, 14)
        elif flavour in ("flat8", "off_grid"):
            d, want = _flat_symbols(256, nb, 2), (8, 8, 256)
        elif flavour == "flat4":
            d, want = _flat_symbols(16, nb, 3), (4, 4, 16)
        else:
            raise KeyError(flavour)
        if flavour == "general_nodelta":  # the symbols are the pixels
            base = np.ascontiguousarray(d.reshape(gh, gw))
            kw = {"flags": mh.MH_FLAG_NO_DELTA}
        else:
            base = image_from_block_deltas(d, gw, gh)
        if flavour == "general14_init":
            kw = {"init_zero_delta": True}
        imgs = [F.block_shuffle(base, 40 + s) for s in range(N_DISTINCT)]
        efs = [mh.encode_frame(im, **kw) for im in imgs]
        assert _lens(efs[0]) == want, (flavour, _lens(efs[0]))
        if flavour == "general14_init":
            assert all(ef.block_init is not None for ef in efs)
        if flavour == "flat8":
            assert all((ef.block_offsets % 8 == 0).all() for ef in efs)
        if flavour == "off_grid":  # every block off the byte grid, another shift per frame
            efs = [shift_stream(ef, 1 + i) for i, ef in enumerate(efs)]
            assert all((ef.block_offsets % 8 != 0).all() for ef in efs)
    for ef in efs:
        assert (ef.width, ef.height) == (gw, gh) and np.array_equal(ef.canon, efs[0].canon)
    efs = [dataclasses.replace(ef, width=W, height=H) for ef in efs]
    assert len({ef.codes.tobytes() for ef in efs}) == len(efs), "the frames of a set differ"
    return [(ef, np.ascontiguousarray(im[:H, :W])) for ef, im in zip(efs, imgs)]


_SETS: dict = {}


def _frame_set(mh, oracle, shape, flavour):
    """Encoded once per module: [(frame, expected raster)], expected = the oracle's decode,
    which must also be the image the frame was made from."""
    key = (shape, flavour)
    if key not in _SETS:
        out = []
        for ef, img in _build_set(mh, shape, flavour):
            want = _oracle_decode(oracle, ef)
            assert np.array_equal(want, img), key
            want.setflags(write=False)
            out.append((ef, want))
        _SETS[key] = out
    return _SETS[key]


def _geometry(geom, W, H):
    """-> (pitch, stride, lead)"""
    w8 = (W + 7) // 8 * 8
    if geom == "tight":
        return w8, H * w8, 4096
    pitch = 136 if W == 93 else (w8 + 8 if (w8 + 8) % 16 else w8 + 16)
    assert pitch % 8 == 0 and pitch % 16 == 8 and pitch > w8
    return pitch, H * pitch + 40, 4096 + 8


def _decode_and_check(mh, device, geom, frames, *, prepared=True, lane_pairs=False, force_offsets=False,
                      kernel, cus):
    """One launch of `frames` = [(EncodedFrame, expected)] into a guarded buffer; asserts the
    routing to `kernel`, then checks every byte of the buffer."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    efs = [f[0] for f in frames]
    n, W, H = len(efs), efs[0].width, efs[0].height
    t1, t2 = efs[0].tables()
    tabs = D.DeviceTables.upload(t1, t2, device, prepare_lut=prepared)
    assert (tabs.lut is not None) == prepared
    fr = D.DeviceFrames.pack(efs, device)
    if force_offsets:  # one frame WITH a frame-offset array: not the single-frame entry
        assert n == 1 and fr.frame_code_offsets is None
        fr.frame_code_offsets = torch.tensor([0, fr.codes.numel()], dtype=torch.int64, device=device)
    assert fr.n_frames == n and (fr.frame_code_offsets is None) == (n == 1 and not force_offsets)

    # launch() in mh_decode.hip
    tiles = -(-fr.n_blocks // 64) * n
    if kernel == "frame":
        assert prepared and n == 1 and fr.frame_code_offsets is None and tiles <= 4 * cus
    elif kernel == "small":
        assert prepared and fr.frame_code_offsets is not None and tiles <= 4 * cus
    elif kernel == "batch":
        assert tiles > 4 * cus
    elif kernel == "batch_inkernel_table":
        assert not prepared and -(-tiles // cus) == 1   # one wave per workgroup: build_lut on 64 threads
    elif kernel == "lanepair":
        assert prepared and lane_pairs and tiles <= 4 * cus
    else:
        raise KeyError(kernel)

    pitch, stride, lead = _geometry(geom, W, H)
    w8 = (W + 7) // 8 * 8
    plan = containment_plan(n, W, H, pitch, stride, lead, 8 * pitch + 4096, written_cols=w8)
    buf = torch.from_numpy(plan.pattern.copy()).to(device)
    d_out = buf.data_ptr() + plan.d_out
    if geom == "tight":
        assert d_out % 256 == 0
    else:
        # (40 bytes are no whole row, except at shape B's pitch of 40: there the gap is row H)
        assert d_out % 16 == 8 and stride % 8 == 0 and stride - H * pitch == 40
        assert (stride % pitch != 0) == (pitch != 40)
    st = D._frame_struct(fr, tabs, N.MH_FLAG_LANE_PAIRS if lane_pairs else 0)
    entry = N.diag_lanepairs().mh_diag_decode_lanepairs if lane_pairs else N.lib().mh_decode
    N.check(entry(ctypes.byref(st), d_out, pitch, stride, torch.cuda.current_stream(device).cuda_stream),
            "mh_decode")
    torch.cuda.synchronize(device)
    check_containment(buf.cpu().numpy(), plan, [f[1] for f in frames])


def _cycle(frames, n):
    return [frames[i % len(frames)] for i in range(n)]


@pytest.fixture(scope="module")
def cus(device):
    import torch
    return torch.cuda.get_device_properties(device).multi_processor_count


GEOMS = pytest.mark.parametrize("geom", ["tight", "loose"])


def _ids(cases):
    return ["-".join(c) for c in cases]


SMALL3 = [("A", "general"), ("A", "general_nodelta"), ("A", "general14_init"), ("A", "flat8"),
          ("A", "off_grid"), ("B", "general14"), ("C", "oversize")]


@GEOMS
@pytest.mark.parametrize("case", SMALL3, ids=_ids(SMALL3))
def test_small_kernel_3_frames(mh, oracle, device, cus, case, geom):
    """1. mh_decode_small_kernel, 3 frames (frame code offsets), prepared table; tiles: A 3 x 2,
    B 3 x 1, C 3 x 2 (<= 4 x CUs). Steps (small_decode): general, general_nodelta -> Small13
    (16-bit codes: the 13-bit table with escapes); general14* -> Small14; flat8 and off_grid
    -> SmallFlat8 (funnel-shift bytes from the staged span); C -> decode_halves<Small14> for
    the oversize tile of each frame."""
    frames = _frame_set(mh, oracle, *case)
    _decode_and_check(mh, device, geom, _cycle(frames, 3), kernel="small", cus=cus)


@GEOMS
def test_small_kernel_one_frame_with_offset_array(mh, oracle, device, cus, geom):
    """2. mh_decode_small_kernel, ONE frame of shape A (2 tiles, general14: Small14) with a
    two-entry frame_code_offsets array: launch() keeps such a call away from the
    single-frame entry, whose arguments have no room for the array."""
    frames = _frame_set(mh, oracle, "A", "general14")
    _decode_and_check(mh, device, geom, frames[:1], force_offsets=True, kernel="small", cus=cus)


@GEOMS
@pytest.mark.parametrize("flavour", ["flat8", "off_grid"])
def test_frame_kernel_flat8(mh, oracle, device, cus, flavour, geom):
    """3. mh_decode_frame_kernel, one frame of shape A (2 tiles, no offset array): the SmallFlat8
    step, on and off the byte grid (test_gpu_frame_entry.py has the lookup tables)."""
    frames = _frame_set(mh, oracle, "A", flavour)
    _decode_and_check(mh, device, geom, frames[1:2], kernel="frame", cus=cus)


BATCH = [("A", "general"), ("A", "noesc"), ("A", "flat4"), ("A", "flat8"), ("A", "off_grid"),
         ("A", "general14_init"), ("B", "general14"), ("C", "oversize")]


@GEOMS
@pytest.mark.parametrize("case", BATCH, ids=_ids(BATCH))
def test_batch_kernel(mh, oracle, device, cus, case, geom):
    """4. mh_decode_kernel, prepared table, 4*CUs // tiles_per_frame + 1 frames (> 4 x CUs tiles:
    513 frames of A or C, 1,025 of B on 256 CUs; 5-wave workgroups), cycling through the
    set's distinct frames so that neighbouring frames differ. Loops: general ->
    batch_loop<Lut13>; noesc -> <Lut13NoEsc>; flat4 -> <Lut13Flat>; flat8 -> flat8_loop's
    per-lane path (flat8_block); off_grid -> flat8_loop's slow loop (decode_halves<Batch8>);
    general14_init -> <Lut13> with block_init; C -> <Lut13NoEsc>, whose waves leave the
    pipelined loop at an oversize tile for the slow loop's decode_halves."""
    frames = _frame_set(mh, oracle, *case)
    gw, gh = SHAPES[case[0]][:2]
    tiles_per_frame = -(-(gw // 8) * (gh // 8) // 64)
    n_batch = 4 * cus // tiles_per_frame + 1
    _decode_and_check(mh, device, geom, _cycle(frames, n_batch), kernel="batch", cus=cus)


INKERNEL = [("A", "general"), ("B", "general14")]


@GEOMS
@pytest.mark.parametrize("case", INKERNEL, ids=_ids(INKERNEL))
def test_batch_kernel_in_kernel_table(mh, oracle, device, cus, case, geom):
    """5. mh_decode_kernel without a prepared table (prepare_lut=False), 3 frames (6 / 3 tiles):
    one-wave workgroups, build_lut on 64 threads, batch_loop<Lut13>."""
    frames = _frame_set(mh, oracle, *case)
    _decode_and_check(mh, device, geom, _cycle(frames, 3), prepared=False, kernel="batch_inkernel_table", cus=cus)


LANEPAIR = [("A", "general14"), ("B", "general14")]


@GEOMS
@pytest.mark.parametrize("case", LANEPAIR, ids=_ids(LANEPAIR))
def test_lane_pair_kernel(mh, oracle, device, cus, case, geom):
    """6. mh_decode_lanepair_kernel (the diagnostic library), 3 frames: 32-block tiles (A: 3 per
    frame, the last with 20 blocks; B: one of 15), its own copy of the output addressing."""
    frames = _frame_set(mh, oracle, *case)
    _decode_and_check(mh, device, geom, _cycle(frames, 3), lane_pairs=True, kernel="lanepair", cus=cus)
