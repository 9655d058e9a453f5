"""Helpers of the set-frames tests (test_gpu_decode_set_frames*.py): frames of the zoo headers at the
smallest sizes at which each path of the entry can go wrong, their upload as a DeviceFrameSet (block
arrays in any order, frames sharing entries), and ONE launch of mh_decode_set_frames through the C ABI
into a GUARDED buffer -- FILL bytes in front of the first raster, behind the last, between the rasters
and in every row's pitch padding. check() compares EVERY byte of that buffer: a decoded frame's pixels
against codec.decode_frame_cpu of the same frame, everything else against FILL. The only bytes not
compared are the contract's unspecified ones, columns W .. round_up(W, 8) - 1 of a written row."""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np

import slice_helpers as SH

FILL = 0xA5
PRESET = 0x5A5A5A5A                      # what a status word holds before the launch
MH_ERR_DIMS, MH_ERR_CAPACITY = -2, -4
GUARD, ROW_GAP, FRAME_GAP = 256, 24, 72  # bytes; multiples of 8, the rasters' alignment rule

# (W, H): one lane; one full block; a partial block; exactly one full tile; a second tile of one lane;
# one block per row (a tile spanning 64 block rows); a tile that straddles block rows; 128 tiles
SIZES = ((1, 1), (8, 8), (9, 7), (512, 8), (520, 8), (8, 520), (264, 40), (1024, 512))
# the four table flavours slice_decode dispatches on: the flat 8-bit identity, flat <= 13 bits,
# longest <= 13, a code longer than 13 bits
HEADERS = ("8x256", "flat", "noesc", "escapes")
FORMATS = {"delta": "delta", "raw": "no_delta", "init": "init_zero_delta"}

_CPU: dict = {}


def up8(v):
    return (v + 7) // 8 * 8


def frame(mh, oracle, size, header, fmt="delta", j=0):
    """-> (EncodedFrame, expected raster): slice_helpers.one_frame at the size's own grid, the expected
    raster codec.decode_frame_cpu of that frame (computed once, read-only; equal to the oracle's)."""
    w, h = size
    key = (w, h, header, fmt, j)
    if key not in _CPU:
        ef, want = SH.one_frame(mh, oracle, (up8(w), up8(h), w, h), header, FORMATS[fmt], j)
        cpu = mh.decode_frame_cpu(ef)
        assert cpu.shape == (h, w) and np.array_equal(cpu, want), key
        cpu.setflags(write=False)
        _CPU[key] = (ef, cpu)
    return _CPU[key]


def frames(mh, oracle, sizes=SIZES, headers=HEADERS, fmt="delta"):
    """One frame per size, the headers dealt in turn (a table per frame), or all under headers[0]."""
    return [frame(mh, oracle, s, headers[i % len(headers)], fmt, i) for i, s in enumerate(sizes)]


def pack(device, efs, block_order=None, alias=None):
    """A DeviceFrameSet of `efs` whose block arrays are concatenated in `block_order` (default: frame
    order), so first_block need not rise with the frame number. alias = {g: f}: frame g stores no block
    entries of its own and names frame f's (the two must be the same frame encoded the same way)."""
    import torch
    import metalhuffman_amd as mh
    from metalhuffman_amd import decoder as D
    lay = mh.frame_set_layout(efs)   # the codes' slots (frame order) and the format
    n = len(efs)
    alias = alias or {}
    order = [f for f in (block_order or range(n)) if f not in alias]
    assert sorted(order + list(alias)) == list(range(n))
    first, offs, init, at = {}, [], [], 0
    for f in order:
        first[f] = at
        offs.append(np.asarray(efs[f].block_offsets, np.uint32))
        if efs[f].block_init is not None:
            init.append(np.asarray(efs[f].block_init, np.uint8))
        at += efs[f].n_blocks
    for g, f in alias.items():
        assert np.array_equal(efs[g].block_offsets, efs[f].block_offsets) and efs[g].width == efs[f].width
        first[g] = first[f]
    geoms = np.array([(first[f], efs[f].width, efs[f].height, 0) for f in range(n)], np.uint32)
    fco = torch.from_numpy(lay.code_offsets).to(device) if n > 1 else None
    return D.DeviceFrameSet(lay.width, lay.height, n, tuple((e.width, e.height) for e in efs), at,
                            torch.from_numpy(np.concatenate(offs).view(np.int32)).to(device),
                            torch.from_numpy(lay.codes).to(device), fco,
                            torch.from_numpy(geoms.view(np.int32)).to(device),
                            torch.from_numpy(np.concatenate(init)).to(device) if init else None, lay.flags, 0)


def tables(device, efs, shared=False):
    from metalhuffman_amd import decoder as D
    if shared:
        assert all(np.array_equal(ef.canon, efs[0].canon) for ef in efs)
        t1, t2 = efs[0].tables()
        return D.DeviceTables.upload(t1, t2, device)
    return D.DeviceTableSet.from_canonical_headers(np.stack([ef.canon for ef in efs]), device)


@dataclasses.dataclass
class Records:
    """The host copy of what one launch reads: u32 arrays in the device's formats."""
    geoms: np.ndarray        # [n, 4]
    rasters: np.ndarray      # [n, 4]: offset low, offset high, pitch, 0
    shares: np.ndarray       # [n, 4]
    group_frame: np.ndarray  # [n_groups]
    out_bytes: int

    def copy(self):
        return Records(self.geoms.copy(), self.rasters.copy(), self.shares.copy(), self.group_frame.copy(),
                       self.out_bytes)


def records(mh, fs, budget=64, pitch_align=0, guarded=True):
    """The planner's shares and map for the set, and rasters: the planner's own (guarded=False: dense,
    so only the pitch padding the alignment leaves is guarded) or a layout with ROW_GAP bytes of padding
    in every row -- a caller pitch larger than the planner's -- and FRAME_GAP bytes between rasters."""
    geoms = fs.geoms.cpu().numpy().view(np.uint32).reshape(-1, 4)
    p = mh.decode_set_plan(geoms, budget, pitch_align)
    rasters, out_bytes = p.rasters.copy(), p.out_bytes
    if guarded:
        A, at = max(8, pitch_align), 0
        for f, (w, h) in enumerate(fs.sizes):
            pitch = int(p.pitches[f]) + -(-ROW_GAP // A) * A
            rasters[f] = (at & 0xFFFFFFFF, at >> 32, pitch, 0)
            at = -(-(at + h * pitch + FRAME_GAP) // A) * A
        out_bytes = at
    return Records(geoms.copy(), rasters, p.shares.copy(), p.group_frame.copy(), out_bytes)


@dataclasses.dataclass
class Launch:
    rc: int
    buf: np.ndarray          # GUARD + out_bytes + GUARD bytes
    status: list             # the set status words, or None
    rec: Records


def run(device, fs, tabs, rec, frame_status="tables", set_status=True, out_bytes=None, extra_flags=0):
    """One launch of mh_decode_set_frames with the records `rec` into a guarded buffer."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    n = fs.n_frames
    buf = torch.full((2 * GUARD + rec.out_bytes,), FILL, dtype=torch.uint8, device=device)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(device)
    d_geoms, d_rasters, d_shares, d_map = dev(rec.geoms), dev(rec.rasters), dev(rec.shares), dev(rec.group_frame)
    st = torch.full((n,), PRESET, dtype=torch.int32, device=device) if set_status is True else set_status
    if isinstance(tabs, D.DeviceTables):
        luts, stride, fst = tabs.lut, 0, None
    else:
        luts, stride, fst = tabs.luts, tabs.stride, tabs.status
    if not isinstance(frame_status, str):
        fst = frame_status
    fr = fs.frame_struct(extra_flags)
    out = buf.data_ptr() + GUARD
    assert out % 8 == 0 and all(t.data_ptr() % 16 == 0 for t in (d_geoms, d_rasters, d_shares))
    rc = N.lib().mh_decode_set_frames(ctypes.byref(fr), d_geoms.data_ptr(), fs.total_blocks, d_rasters.data_ptr(),
                                      d_shares.data_ptr(), d_map.data_ptr(), int(rec.group_frame.size),
                                      luts.data_ptr(), stride, fst.data_ptr() if fst is not None else None,
                                      st.data_ptr() if st is not None else None, out,
                                      rec.out_bytes if out_bytes is None else out_bytes,
                                      torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize(device)
    return Launch(rc, buf.cpu().numpy(), st.cpu().tolist() if st is not None else None, rec)


def check(lay, rasters, sizes, expected, care=None, partial=()):
    """Every byte of the guarded buffer. rasters: the u32[n, 4] records the EXPECTED layout follows
    (the launch's own, or the uncorrupted ones); expected[f]: None for a frame that must have written
    nothing, else its [H, W] picture. care: None or a bool[H, W] mask per frame (compare where True).
    partial: frames that may have lost tiles -- each of their pixels is the picture's or still FILL."""
    exp = np.full(lay.buf.size, FILL, np.uint8)
    cmp = np.ones(lay.buf.size, bool)
    either = np.zeros(lay.buf.size, bool)
    assert len(expected) == len(sizes)
    for f, px in enumerate(expected):
        if px is None:
            continue
        w, h = sizes[f]
        assert px.shape == (h, w), (f, px.shape, sizes[f])
        off = GUARD + (int(rasters[f, 0]) | int(rasters[f, 1]) << 32)
        pitch = int(rasters[f, 2])
        for y in range(h):
            o = off + y * pitch
            exp[o: o + w] = px[y]
            cmp[o + w: o + up8(w)] = False
            if care is not None and care[f] is not None:
                cmp[o: o + w] = care[f][y]
            if f in partial:
                either[o: o + w] = True
    bad = np.flatnonzero((lay.buf != exp) & cmp & ~(either & (lay.buf == FILL)))
    if bad.size:
        o = int(bad[0])
        where = "a guard byte"
        for f, (w, h) in enumerate(sizes):
            off, pitch = GUARD + (int(rasters[f, 0]) | int(rasters[f, 1]) << 32), int(rasters[f, 2])
            if off <= o < off + h * pitch:
                where = f"frame {f} ({w} x {h}), row {(o - off) // pitch}, byte {(o - off) % pitch}"
        raise AssertionError(f"{bad.size} wrong byte(s) of {lay.buf.size}; first at offset {o} ({where}): "
                             f"{int(lay.buf[o]):#x}, expected {int(exp[o]):#x}")
