"""GPU decode path: torch device tensors in, W x H uint8 raster out, via mh_decode().

This is the host-side mirror of the reference renderer's decode contract
(Shared/AAPLRenderer.m:1192-1678): the same five buffers (block offsets, huffBuff,
T1, T2, dims) are uploaded once (the renderer's MTLBuffers, :576-667) and every
decode is one launch of the HIP kernel in csrc/mh_decode.hip. PyTorch is only the
device-memory / stream plumbing; nothing here computes on the CPU.
"""
from __future__ import annotations

import contextlib
import ctypes
import dataclasses
import zlib
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .codec import DecodeSetPlan, EncodedFrame, Huffman, block_grid, decode_set_plan, finite_f32, frame_set_layout
from .codec import norm_format as _norm_format

ALIGN = 16  # frame code starts inside a packed batch (16-byte buffer loads)


def _dev(device) -> torch.device:
    d = torch.device(device)
    if d.type != "cuda":
        raise RuntimeError("the MI355X decoder needs a HIP device (torch 'cuda' on ROCm)")
    if d.index is None:  # 'cuda' -> the current device, so device checks compare equal
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def _stream_ptr(stream: Optional[torch.cuda.Stream], device: torch.device) -> int:
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return int(s.cuda_stream)


def _header_tensor(canon, dev: torch.device, convert: bool = True) -> torch.Tensor:
    """Canonical headers -> a u8 tensor on `dev`: a host array is uploaded; a tensor is moved, cast
    and made contiguous, or (convert=False) left as it is for the caller to judge."""
    if isinstance(canon, torch.Tensor):
        return canon.to(dev, torch.uint8).contiguous() if convert else canon
    return torch.from_numpy(np.ascontiguousarray(canon, np.uint8)).to(dev)


def _tables_key(t1, t2) -> int:
    """A checksum of host T1/T2 (generateSplitLookupTables' arrays): which code a table pair is.
    Mid-block marks hold a running symbol sum, so they are good under their frame's own tables only."""
    return zlib.crc32(np.ascontiguousarray(t2, np.uint8), zlib.crc32(np.ascontiguousarray(t1, np.uint8)))


@dataclasses.dataclass
class DeviceTables:
    """T1/T2 (+ the derived LDS table) resident on one device."""
    table1: torch.Tensor     # u8[512]
    table2: torch.Tensor     # u8[2 * entries]
    lut: Optional[torch.Tensor]  # u8[mh_lut_bytes()] from mh_prepare_lut, or None
    # _tables_key of the host tables these were uploaded or built from (None: unknown, e.g. built
    # from a header that is already a device tensor): decode() uses a frame's mid-block marks only
    # under the tables of the frame's own code
    key: Optional[int] = None

    @property
    def table2_entries(self) -> int:
        return self.table2.numel() // 2

    @classmethod
    def upload(cls, t1: np.ndarray, t2: np.ndarray, device="cuda", prepare_lut: bool = True,
               stream: Optional[torch.cuda.Stream] = None) -> "DeviceTables":
        dev = _dev(device)
        d1 = torch.from_numpy(np.ascontiguousarray(t1, np.uint8)).to(dev)
        d2 = torch.from_numpy(np.ascontiguousarray(t2, np.uint8)).to(dev)
        tabs = cls(d1, d2, None, _tables_key(t1, t2))
        if prepare_lut:
            tabs.prepare_lut(stream)
        return tabs

    @classmethod
    def from_canonical_header(cls, canon, device="cuda", prepare_lut: bool = True,
                              stream: Optional[torch.cuda.Stream] = None) -> "DeviceTables":
        """Build T1/T2 (and the prepared table) ON the device from the 256-byte
        canonical header (mh_build_tables_device), e.g. after a 256-byte broadcast.
        T2 keeps its full MH_TABLE2_MAX_ENTRIES capacity (zero past the used
        subtables). Asynchronous; check_status() syncs and raises on a bad header."""
        dev = _dev(device)
        hdr = _header_tensor(canon, dev)
        if hdr.numel() != 256:
            raise ValueError("the canonical header has 256 entries")
        d1 = torch.empty(512, dtype=torch.uint8, device=dev)
        d2 = torch.empty(2 * N.MH_TABLE2_MAX_ENTRIES, dtype=torch.uint8, device=dev)
        meta = torch.zeros(2, dtype=torch.int32, device=dev)  # [used T2 entries, status]
        lut = torch.empty(int(N.lib().mh_lut_bytes()), dtype=torch.uint8, device=dev) if prepare_lut else None
        N.check(N.lib().mh_build_tables_device(hdr.data_ptr(), d1.data_ptr(), d2.data_ptr(),
                                               meta.data_ptr(), lut.data_ptr() if lut is not None else None,
                                               meta.data_ptr() + 4, _stream_ptr(stream, dev)),
                "mh_build_tables_device")
        tabs = cls(d1, d2, lut)
        tabs._meta = meta
        if not isinstance(canon, torch.Tensor):
            try:
                tabs.key = _tables_key(*Huffman.generateSplitLookupTables(np.ascontiguousarray(canon, np.uint8)))
            except (N.MHError, ValueError):  # a header the device will reject too (check_status)
                pass
        return tabs

    def check_status(self) -> int:
        """Used T2 entries of a device-built table (synchronises); raises MHError
        when the header was rejected."""
        meta = getattr(self, "_meta", None)
        if meta is None:
            return self.table2_entries
        entries, status = (int(v) for v in meta.cpu().tolist())
        N.check(status, "mh_build_tables_device")
        return entries

    def prepare_lut(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        dev = self.table1.device
        lut = torch.empty(int(N.lib().mh_lut_bytes()), dtype=torch.uint8, device=dev)
        N.check(N.lib().mh_prepare_lut(self.table1.data_ptr(), self.table2.data_ptr(),
                                       self.table2_entries, lut.data_ptr(),
                                       _stream_ptr(stream, dev)), "mh_prepare_lut")
        self.lut = lut


@dataclasses.dataclass
class DeviceTableSet:
    """n prepared tables, one per frame of a batch, for decode_frames (mh_decode_frames):
    table i at luts[i], status[i] its build status (non-zero: header rejected, the table
    is all zero and decode_frames skips the frame)."""
    luts: torch.Tensor       # u8[n, stride], stride a multiple of 16 >= mh_lut_bytes()
    status: torch.Tensor     # int32[n]

    @property
    def n_tables(self) -> int:
        return int(self.luts.shape[0])

    @property
    def stride(self) -> int:
        return int(self.luts.shape[1])

    @classmethod
    def from_canonical_headers(cls, canon, device="cuda",
                               stream: Optional[torch.cuda.Stream] = None) -> "DeviceTableSet":
        """Build the n prepared tables ON the device from n 256-byte canonical headers
        (u8[n, 256], tensor or array) in one launch (mh_build_luts_device). Asynchronous;
        check_status() syncs and raises when a header was rejected."""
        dev = _dev(device)
        hdr = _header_tensor(canon, dev)
        if hdr.dim() != 2 or hdr.shape[1] != 256 or hdr.shape[0] < 1:
            raise ValueError("canonical headers are u8[n, 256]")
        n = int(hdr.shape[0])
        stride = (int(N.lib().mh_lut_bytes()) + 15) // 16 * 16
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            luts = torch.empty((n, stride), dtype=torch.uint8, device=dev)
            status = torch.empty(n, dtype=torch.int32, device=dev)
        N.check(N.lib().mh_build_luts_device(hdr.data_ptr(), n, luts.data_ptr(), stride, status.data_ptr(),
                                             _stream_ptr(stream, dev)), "mh_build_luts_device")
        ts = cls(luts, status)
        ts._headers = hdr  # read by the launch in flight
        return ts

    def check_status(self) -> None:
        """Synchronises; raises MHError naming the frames whose header was rejected."""
        st = self.status.cpu().tolist()
        bad = [i for i, s in enumerate(st) if s]
        if bad:
            raise N.MHError(int(st[bad[0]]), f"mh_build_luts_device: frame(s) {bad[:8]} rejected")


@dataclasses.dataclass
class DeviceFrames:
    """n frames of one size packed for mh_decode (one shared table pair) or, packed with
    shared_table=False, for mh_decode_frames (a table per frame)."""
    width: int
    height: int
    n_frames: int
    block_offsets: torch.Tensor          # u32 as int32[n * NB]
    codes: torch.Tensor                  # u8[total]
    frame_code_offsets: Optional[torch.Tensor]  # int64[n + 1] (None for one frame)
    block_init: Optional[torch.Tensor] = None   # u8[n * NB]
    flags: int = 0
    code_bytes: int = 0                  # payload bytes (sum over frames, pad excluded)
    # u32 as int32[n * NB] mid-block marks, or None: used by decode() of a single frame
    # (mh_decode_marked); every other entry ignores them. One rule, EncodedFrame's: marks belong to
    # the buffers they were made for, named by marks_for = (block_offsets, codes, block_init,
    # tables key). decode() passes the marks only while the object still holds those very tensors
    # and is given tables of that key (DeviceTables.key, the frames' own code); in every other case
    # -- re-seated buffers, dataclasses.replace with other buffers, foreign or unkeyed tables, a
    # batch -- the launch is mh_decode's. The tables are part of the rule because a mark holds a
    # running symbol sum: decode() accepts any tables for any frames, and under another code the
    # result is defined by the walk from the block's offset (the oracle's), which marks of the
    # frame's own code would not reproduce.
    mid_marks: Optional[torch.Tensor] = None
    marks_for: Optional[tuple] = dataclasses.field(default=None, repr=False, compare=False)

    def bind_mid_marks(self, marks: Optional[torch.Tensor], tables_key: Optional[int]) -> None:
        """Attach marks made from this object's present buffers, valid under the tables of `tables_key`."""
        self.mid_marks = marks
        self.marks_for = (self.block_offsets, self.codes, self.block_init, tables_key)

    @property
    def n_blocks(self) -> int:
        bw, bh = block_grid(self.width, self.height)
        return bw * bh

    @classmethod
    def pack(cls, frames: Sequence[EncodedFrame], device="cuda", shared_table: bool = True) -> "DeviceFrames":
        """Upload frames (host arrays) into one packed device batch. shared_table=True
        (default): the frames must share one canonical table (decode()); False: any
        headers, for decode_frames() with a DeviceTableSet. When every frame has valid mid-block
        marks (EncodedFrame.valid_mid_marks: made from the frame's present bytes) they are
        uploaded too, in one buffer with the block offsets and right behind them."""
        dev = _dev(device)
        if not frames:
            raise ValueError("no frames")
        w, h, fl = frames[0].width, frames[0].height, frames[0].flags
        for f in frames:
            if (f.width, f.height, f.flags) != (w, h, fl):
                raise ValueError("a batch holds frames of one size and one format")
            if shared_table and not np.array_equal(f.canon, frames[0].canon):
                raise ValueError("a batch shares one canonical table")
        starts = [0]
        for f in frames:
            starts.append(starts[-1] + ((f.codes.size + ALIGN - 1) // ALIGN) * ALIGN)
        packed = np.zeros(starts[-1], np.uint8)
        for f, s in zip(frames, starts):
            packed[s: s + f.codes.size] = f.codes
        offs = np.concatenate([f.block_offsets for f in frames]).astype(np.uint32)
        init = None
        if frames[0].block_init is not None:
            init = torch.from_numpy(np.concatenate([f.block_init for f in frames])).to(dev)
        fco = None
        if len(frames) > 1:
            fco = torch.tensor(starts, dtype=torch.int64, device=dev)
        d_offs, d_marks = None, None
        host_marks = [f.valid_mid_marks() for f in frames]
        if all(m is not None for m in host_marks):
            marks = np.concatenate(host_marks).astype(np.uint32)
            both = torch.from_numpy(np.concatenate([offs, marks]).view(np.int32)).to(dev)
            d_offs, d_marks = both[: offs.size], both[offs.size:]
        else:
            d_offs = torch.from_numpy(offs.view(np.int32)).to(dev)
        out = cls(w, h, len(frames), d_offs, torch.from_numpy(packed).to(dev), fco, init, fl,
                  sum(f.payload_bytes for f in frames))
        if d_marks is not None:
            out.bind_mid_marks(d_marks, _tables_key(*frames[0].tables()) if shared_table else None)
        return out


@dataclasses.dataclass
class DeviceFrameSet:
    """n frames of DIFFERENT sizes packed for the set entries (decode_set_crops,
    decode_set_crops_normalized_planes; include/metalhuffman.h, mh_frame_geom): one offsets array
    over all the frames' blocks, one code slot and one geometry record (first block, width, height)
    per frame. width and height are the LARGEST in the set -- what the C entries take as dims."""
    width: int
    height: int
    n_frames: int
    sizes: tuple                         # ((width, height), ...) per frame
    total_blocks: int
    block_offsets: torch.Tensor          # u32 as int32[total_blocks]
    codes: torch.Tensor                  # u8[total]
    frame_code_offsets: Optional[torch.Tensor]  # int64[n + 1] (None for one frame)
    geoms: torch.Tensor                  # u32 as int32[n, 4]: mh_frame_geom records
    block_init: Optional[torch.Tensor] = None   # u8[total_blocks]
    flags: int = 0
    code_bytes: int = 0                  # payload bytes (sum over frames, pad excluded)

    @classmethod
    def pack(cls, frames: Sequence[EncodedFrame], device="cuda") -> "DeviceFrameSet":
        """Upload codec.frame_set_layout(frames): frames of any sizes and any headers (a table per
        frame from a DeviceTableSet, or one DeviceTables when they share a header) of one format."""
        dev = _dev(device)
        lay = frame_set_layout(frames)
        n = len(lay.geoms)
        init = torch.from_numpy(lay.block_init).to(dev) if lay.block_init is not None else None
        fco = torch.from_numpy(lay.code_offsets).to(dev) if n > 1 else None
        return cls(lay.width, lay.height, n, tuple((int(g[1]), int(g[2])) for g in lay.geoms), lay.total_blocks,
                   torch.from_numpy(lay.block_offsets.view(np.int32)).to(dev), torch.from_numpy(lay.codes).to(dev),
                   fco, torch.from_numpy(lay.geoms.view(np.int32)).to(dev), init, lay.flags,
                   sum(f.payload_bytes for f in frames))

    def size_limits(self) -> tuple:
        """(widths, heights) as int64 arrays, one entry per frame (the host check of a crop list)."""
        lim = self.__dict__.get("_limits")
        if lim is None:
            a = np.asarray(self.sizes, np.int64).reshape(-1, 2)
            lim = self.__dict__["_limits"] = (a[:, 0].copy(), a[:, 1].copy())
        return lim

    def frame_struct(self, extra_flags: int = 0) -> N.mh_frame:
        """The mh_frame of the set: dims carry the largest width and height, the table fields are NULL
        (the set entries take prepared tables). Cached as DeviceFrames' structs are; never modified."""
        return _frame_entry(self, None, extra_flags)[0]

    def _head(self, dev_index: int) -> tuple:
        """(d_geoms, total_blocks) for the C entries, the records checked as `out` tensors are."""
        g = self.geoms
        if (g.dtype is not torch.int32 or g.shape != (self.n_frames, 4) or g.get_device() != dev_index
                or not g.is_contiguous() or g.data_ptr() % 16):
            raise ValueError(f"geoms must be a contiguous, 16-byte aligned int32 [{self.n_frames}, 4] tensor on "
                             f"cuda:{dev_index}")
        return g.data_ptr(), self.total_blocks


def _marks_ptr(frames: DeviceFrames, tables: Optional[DeviceTables]) -> Optional[int]:
    """The marks' address if decode(frames, tables) may use them (DeviceFrames.marks_for), else None."""
    m, bound = frames.mid_marks, frames.marks_for
    if m is None or bound is None or tables is None:
        return None
    if (bound[0] is not frames.block_offsets or bound[1] is not frames.codes or bound[2] is not frames.block_init
            or bound[3] is None or tables.key != bound[3]):
        return None
    if m.device != frames.codes.device or m.numel() != frames.block_offsets.numel() or not m.is_contiguous():
        return None
    return m.data_ptr()


def _frame_entry(frames: DeviceFrames, tables: Optional[DeviceTables], extra_flags: int = 0):
    """(mh_frame, device index) for (frames, tables): _frame_cache's struct and its device."""
    fr, cache = _frame_cache(frames, tables, extra_flags)
    return fr, cache[3]


def _frame_cache(frames: DeviceFrames, tables: Optional[DeviceTables], extra_flags: int = 0):
    """(mh_frame, cache entry) for (frames, tables), extra_flags ORed into the frames'
    flags. Filling a ctypes struct field by field costs ~5.5 us of Python -- more than
    the 5.3 us decode of a 2048x1536 frame -- so the structs are kept on `frames` and
    reused while the buffers and sizes they were built from are the same objects (the
    buffer tensors are the renderer's MTLBuffers: allocated once, never re-seated in
    place; the cache holds references to them, so their ids cannot be reused). The
    device check runs when an entry is built. Callers never modify the struct.
    tables None: the struct of the frame-slice entries (mh_decode_frames, ...), whose table
    fields stay NULL; those structs have a cache of their own beside the first."""
    if tables is not None:
        slot, t1, t2, lut = "_fr_cache", tables.table1, tables.table2, tables.lut
    else:
        slot, t1, t2, lut = "_frs_cache", None, None, None
    refs = (frames.block_offsets, frames.codes, frames.frame_code_offsets, frames.block_init, t1, t2, lut)
    marks = getattr(frames, "mid_marks", None)  # (a DeviceFrameSet has none)
    key = (id(refs[0]), id(refs[1]), id(refs[2]), id(refs[3]), id(t1), id(t2), id(lut),
           frames.width, frames.height, frames.n_frames, frames.flags, id(marks))
    cache = frames.__dict__.get(slot)
    if cache is None or cache[0] != key:
        dev = frames.codes.device
        if dev.type != "cuda" or any(t is not None and t.device != dev for t in refs):
            raise ValueError("tables and frames must live on the same HIP device" if tables is not None
                             else "the frames' buffers must live on one HIP device")
        # [4], [5]: the marks decode() passes for this pair (and a reference that keeps them alive)
        cache = (key, refs, {}, dev.index, _marks_ptr(frames, tables) if marks is not None else None, marks)
        frames.__dict__[slot] = cache
    fr = cache[2].get(extra_flags)
    if fr is None:
        bw, bh = block_grid(frames.width, frames.height)
        ptr = [t.data_ptr() if t is not None else None for t in refs]
        fr = N.mh_frame(ptr[0], ptr[1], frames.codes.numel(), ptr[2], ptr[4], ptr[5],
                        tables.table2_entries if tables is not None else 0, ptr[6], ptr[3],
                        N.mh_dims(frames.width, frames.height, bw, bh), frames.n_frames,
                        frames.flags | extra_flags)
        cache[2][extra_flags] = fr
    return fr, cache


def _frame_struct(frames: DeviceFrames, tables: DeviceTables, extra_flags: int = 0) -> N.mh_frame:
    return _frame_entry(frames, tables, extra_flags)[0]


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def decode(frames: DeviceFrames, tables: DeviceTables, out: Optional[torch.Tensor] = None,
           stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0) -> torch.Tensor:
    """Decode every frame into out[n, H, pitch] (pitch = W rounded up to 8).
    extra_flags: decode-only flags ORed into the frame's (MH_FLAG_ANY_ORDER; MH_FLAG_LANE_PAIRS
    routes the call to the lane-pair diagnostic library, _native.diag_lanepairs()).
    The per-call host path is kept lean (a cached struct, the raw current stream): one
    frame decodes in ~5.3 us, so every microsecond of Python shows in eager loops."""
    fr, cache = _frame_cache(frames, tables, extra_flags)
    dev_index, marks = cache[3], cache[4]
    pitch = (frames.width + 7) // 8 * 8
    h = frames.height
    # _out_raster and _raw_stream_ptr inlined on purpose: two calls show on the 5.3 us single-frame path
    if out is None:
        out = torch.empty((frames.n_frames, h, pitch), dtype=torch.uint8, device=frames.codes.device)
    else:
        sh = out.shape
        if (out.dtype is not torch.uint8 or len(sh) < 2 or sh[-1] != pitch or sh[-2] != h
                or out.get_device() != dev_index or not out.is_contiguous()
                or out.numel() < frames.n_frames * h * pitch):
            raise ValueError(f"out must be a contiguous uint8 [{frames.n_frames}, {h}, {pitch}] "
                             f"tensor on cuda:{dev_index}")
    if stream is not None:
        sp = stream.cuda_stream
    elif _raw_stream is not None:
        sp = _raw_stream(dev_index)
    else:
        sp = torch.cuda.current_stream(dev_index).cuda_stream
    if fr.flags & N.MH_FLAG_LANE_PAIRS:  # the diagnostic library's kernel (A/B only)
        rc = N.diag_lanepairs().mh_diag_decode_lanepairs(ctypes.byref(fr), out.data_ptr(), pitch, h * pitch, sp)
    elif marks is not None:
        rc = N.lib().mh_decode_marked(ctypes.byref(fr), marks, out.data_ptr(), pitch, h * pitch, sp)
    else:
        rc = N.lib().mh_decode(ctypes.byref(fr), out.data_ptr(), pitch, h * pitch, sp)
    if rc:
        N.check(rc, "mh_decode")
    return out


CHECK_FIELDS = ("zero_width_lookups", "bad_escapes", "length_mismatches", "first_bad_block")


def check(frames: DeviceFrames, tables: DeviceTables,
          stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Debug mode of the decode contract (mh_check): per frame u32[4] =
    (zero-width lookups, T1 escapes past T2, blocks whose codes miss the next
    block's offset, first offending block or 0xFFFFFFFF), as an int64 tensor
    [n_frames, 4] on the device. Never touches a raster."""
    dev = frames.codes.device
    rep = torch.empty((frames.n_frames, 4), dtype=torch.int32, device=dev)
    fr = _frame_struct(frames, tables)
    N.check(N.lib().mh_check(ctypes.byref(fr), rep.data_ptr(), _stream_ptr(stream, dev)), "mh_check")
    return rep.to(torch.int64) & 0xFFFFFFFF


def _frames_entry(frames: DeviceFrames, extra_flags: int = 0):
    return _frame_entry(frames, None, extra_flags)


def _slice_entry(who: str, frames: DeviceFrames, extra_flags: int):
    """_frames_entry for the decode entries of the product library, none of which has the lane-pair
    kernel: (mh_frame, device index), or ValueError naming `who` under MH_FLAG_LANE_PAIRS."""
    fr, dev_index = _frame_entry(frames, None, extra_flags)
    if fr.flags & N.MH_FLAG_LANE_PAIRS:
        raise ValueError(f"MH_FLAG_LANE_PAIRS does not apply to {who}")
    return fr, dev_index


def _out_raster(frames: DeviceFrames, out: Optional[torch.Tensor], h: int, pitch: int, dev_index: int,
                stream: Optional[torch.cuda.Stream]) -> torch.Tensor:
    """decode()'s `out` contract for a raster of h rows: allocated (on `stream`) when None,
    validated otherwise."""
    if out is None:
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            return torch.empty((frames.n_frames, h, pitch), dtype=torch.uint8, device=frames.codes.device)
    sh = out.shape
    if (out.dtype is not torch.uint8 or len(sh) < 2 or sh[-1] != pitch or sh[-2] != h
            or out.get_device() != dev_index or not out.is_contiguous()
            or out.numel() < frames.n_frames * h * pitch):
        raise ValueError(f"out must be a contiguous uint8 [{frames.n_frames}, {h}, {pitch}] "
                         f"tensor on cuda:{dev_index}")
    return out


def _raw_stream_ptr(stream: Optional[torch.cuda.Stream], dev_index: int) -> int:
    if stream is not None:
        return stream.cuda_stream
    if _raw_stream is not None:
        return _raw_stream(dev_index)
    return torch.cuda.current_stream(dev_index).cuda_stream


def _check_table_set(ts: DeviceTableSet, frames: DeviceFrames, dev_index: int) -> None:
    if (ts.n_tables != frames.n_frames or ts.luts.get_device() != dev_index
            or ts.luts.dtype is not torch.uint8 or not ts.luts.is_contiguous()
            or ts.status.get_device() != dev_index or ts.status.dtype is not torch.int32
            or ts.status.numel() != frames.n_frames or not ts.status.is_contiguous()):
        raise ValueError(f"the table set must hold {frames.n_frames} tables on cuda:{dev_index}")


def _slice_shape(entry: str, frames: DeviceFrames, stream: Optional[torch.cuda.Stream], extra_flags: int,
                 region=None, windows=None, log2_scale=None, crops=None) -> tuple:
    """(workgroups per frame, window or crop, waves per workgroup) from the C entry `entry`
    (mh_decode_*_shape). Between the frame and the stream the entry takes `region`, or
    windows = (n_windows, (bw, bh)) and then `log2_scale`, or crops = (n_crops, (w, h)[, dtype
    [, n_planes]]), the pixel size followed by the format and the plane count -- each when given."""
    scale = () if log2_scale is None else (_log2_scale(log2_scale),)
    what = ()
    if windows is not None:
        size = _window_size(frames, windows[1])
    elif crops is not None:
        what = _crop_size(frames, crops[1])
        if len(crops) > 2:
            what += (_norm_format(crops[2]),)
        if int(crops[0]) < 1:
            raise ValueError("no crops")
        if len(crops) > 3:
            if not 1 <= int(crops[3]) <= N.MH_MAX_PLANES:
                raise ValueError(f"1..{N.MH_MAX_PLANES} planes, not {crops[3]}")
            what += (int(crops[3]),)
        what = (int(crops[0]), *what)
    fr, dev_index = _frame_entry(frames, None, extra_flags)
    if windows is not None:  # (the windows' count is checked behind the frame entry, the crops' ahead of it)
        if int(windows[0]) < 1:
            raise ValueError("no windows")
        what = (int(windows[0]), *size)
    elif region is not None:
        what = (ctypes.byref(_region_struct(frames, region)),)
    g, w = ctypes.c_uint32(0), ctypes.c_uint32(0)
    N.check(getattr(N.lib(), entry)(ctypes.byref(fr), *what, *scale, _raw_stream_ptr(stream, dev_index),
                                    ctypes.byref(g), ctypes.byref(w)), entry)
    return int(g.value), int(w.value)


def decode_frames_shape(frames: DeviceFrames, stream: Optional[torch.cuda.Stream] = None,
                        extra_flags: int = 0) -> tuple:
    """(workgroups per frame, waves per workgroup) decode_frames would launch with
    (mh_decode_frames_shape)."""
    return _slice_shape("mh_decode_frames_shape", frames, stream, extra_flags)


def decode_frames(frames, table_set="cuda", out: Optional[torch.Tensor] = None,
                  stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0, skip_rejected: bool = True):
    """Two uses, told apart by the first argument:

    decode_frames(frames: DeviceFrames, table_set: DeviceTableSet, out=None, stream=None,
    extra_flags=0, skip_rejected=True) -> the device raster out[n, H, pitch] (decode()'s `out`
    contract), frame f decoded with its own table table_set.luts[f] in one launch
    (mh_decode_frames). skip_rejected: table_set.status goes in as the per-frame status, so
    a frame whose word is non-zero is skipped and its raster left untouched.

    decode_frames(encoded: Sequence[EncodedFrame], device="cuda") -> [n, H, W] uint8 on the
    host: the convenience for frames that share one table (upload, decode, copy back);
    decode_frames_mixed is its twin for lists with different headers."""
    if not isinstance(frames, DeviceFrames):
        return _decode_frames_host(frames, table_set)
    if not isinstance(table_set, DeviceTableSet):
        raise TypeError("decode_frames(DeviceFrames, ...) takes a DeviceTableSet")
    fr, dev_index = _slice_entry("decode_frames", frames, extra_flags)
    _check_table_set(table_set, frames, dev_index)
    pitch = (frames.width + 7) // 8 * 8
    h = frames.height
    out = _out_raster(frames, out, h, pitch, dev_index, stream)
    sp = _raw_stream_ptr(stream, dev_index)
    rc = N.lib().mh_decode_frames(ctypes.byref(fr), table_set.luts.data_ptr(), table_set.stride,
                                  table_set.status.data_ptr() if skip_rejected else None, out.data_ptr(), pitch,
                                  h * pitch, sp)
    if rc:
        N.check(rc, "mh_decode_frames")
    return out


class Region(NamedTuple):
    """Blocks [bx0, bx0 + bw) x [by0, by0 + bh) of a frame's 8x8 block grid (mh_region)."""
    bx0: int
    by0: int
    bw: int
    bh: int

    def pixel_size(self, width: int, height: int) -> tuple:
        """(RW, RH): the region's pixels inside a width x height frame (the frame's right and
        bottom edge blocks are partial)."""
        return (min(width, 8 * (self.bx0 + self.bw)) - 8 * self.bx0,
                min(height, 8 * (self.by0 + self.bh)) - 8 * self.by0)

    def scaled_size(self, width: int, height: int, log2_scale: int) -> tuple:
        """(SW, SH): the region's size at scale 2^log2_scale, ceil(RW / s) x ceil(RH / s)."""
        s = 1 << _log2_scale(log2_scale)
        rw, rh = self.pixel_size(width, height)
        return (rw + s - 1) // s, (rh + s - 1) // s


def region_of_rect(width: int, height: int, x0: int, y0: int, w: int, h: int) -> tuple:
    """The pixel rectangle [x0, x0 + w) x [y0, y0 + h) of a width x height frame rounded out to
    whole blocks -> (Region, dx, dy), (dx, dy) the rectangle's offset inside the region. Pure.
    ValueError when the rectangle is empty or leaves the frame."""
    width, height, x0, y0, w, h = (int(v) for v in (width, height, x0, y0, w, h))
    if width < 1 or height < 1:
        raise ValueError("an empty frame")
    if w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > width or y0 + h > height:
        raise ValueError(f"the rectangle {w}x{h} at ({x0}, {y0}) lies outside the {width}x{height} frame")
    bx0, by0 = x0 // 8, y0 // 8
    return (Region(bx0, by0, (x0 + w + 7) // 8 - bx0, (y0 + h + 7) // 8 - by0), x0 - 8 * bx0, y0 - 8 * by0)


def _region_struct(frames: DeviceFrames, region) -> "N.mh_region":
    bx0, by0, bw, bh = (int(v) for v in region)
    gw, gh = block_grid(frames.width, frames.height)
    if bw < 1 or bh < 1 or bx0 < 0 or by0 < 0 or bx0 + bw > gw or by0 + bh > gh:
        raise ValueError(f"region {(bx0, by0, bw, bh)} lies outside the {gw}x{gh} block grid")
    return N.mh_region(bx0, by0, bw, bh)


def decode_region_shape(frames: DeviceFrames, region, stream: Optional[torch.cuda.Stream] = None,
                        extra_flags: int = 0) -> tuple:
    """(workgroups per frame, waves per workgroup) decode_region would launch with
    (mh_decode_region_shape)."""
    return _slice_shape("mh_decode_region_shape", frames, stream, extra_flags, region)


def _region_tables(who: str, frames: DeviceFrames, tables, dev_index: int, skip_rejected: bool) -> tuple:
    """decode_region's table argument -> (luts, stride, status or None)."""
    if isinstance(tables, DeviceTables):
        if tables.lut is None:
            raise ValueError(f"{who} needs the prepared table (DeviceTables.prepare_lut())")
        if tables.lut.get_device() != dev_index:
            raise ValueError(f"the table must live on cuda:{dev_index}")
        return tables.lut, 0, None
    if isinstance(tables, DeviceTableSet):
        _check_table_set(tables, frames, dev_index)
        return tables.luts, tables.stride, tables.status if skip_rejected else None
    raise TypeError(f"{who} takes a DeviceTables or a DeviceTableSet")


def _decode_region(who: str, k: Optional[int], frames: DeviceFrames, tables, region, out, stream,
                   extra_flags: int, skip_rejected: bool) -> torch.Tensor:
    """decode_region (k None: the C entry takes no scale) and decode_region_scaled: the arguments
    checked, the default raster made, one launch."""
    fr, dev_index = _slice_entry(who, frames, extra_flags)
    rg = _region_struct(frames, region)
    luts, stride, status = _region_tables(who, frames, tables, dev_index, skip_rejected)
    k0 = k or 0
    pitch = (8 >> k0) * rg.bw
    h = (min(frames.height, 8 * (rg.by0 + rg.bh)) - 8 * rg.by0 + (1 << k0) - 1) >> k0  # RH, or SH = ceil(RH / s)
    out = _out_raster(frames, out, h, pitch, dev_index, stream)
    sp = _raw_stream_ptr(stream, dev_index)
    tail = (luts.data_ptr(), stride, status.data_ptr() if status is not None else None, out.data_ptr(), pitch,
            h * pitch, sp)
    if k is None:
        rc = N.lib().mh_decode_region(ctypes.byref(fr), ctypes.byref(rg), *tail)
    else:
        rc = N.lib().mh_decode_region_scaled(ctypes.byref(fr), ctypes.byref(rg), k, *tail)
    if rc:
        N.check(rc, "mh_" + who)
    return out


def decode_region(frames: DeviceFrames, tables, region, out: Optional[torch.Tensor] = None,
                  stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0,
                  skip_rejected: bool = True) -> torch.Tensor:
    """Decode the blocks `region` = (bx0, by0, bw, bh) of every frame into out[n, RH, 8 * bw] in
    one launch (mh_decode_region); the full W x H raster is neither written nor needed. tables: a
    DeviceTables (its prepared table shared by all frames) or a DeviceTableSet (a table per
    frame; with skip_rejected its status goes in as the per-frame status and a frame whose word
    is non-zero is left untouched). out: decode()'s contract with the region's shape."""
    return _decode_region("decode_region", None, frames, tables, region, out, stream, extra_flags, skip_rejected)


def _log2_scale(log2_scale) -> int:
    k = int(log2_scale)
    if k != log2_scale or not 0 <= k <= 3:
        raise ValueError(f"log2_scale must be 0, 1, 2 or 3 (scale 1, 1/2, 1/4, 1/8), not {log2_scale!r}")
    return k


def decode_region_scaled_shape(frames: DeviceFrames, region, log2_scale: int,
                               stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0) -> tuple:
    """(workgroups per frame, waves per workgroup) decode_region_scaled would launch with
    (mh_decode_region_scaled_shape)."""
    return _slice_shape("mh_decode_region_scaled_shape", frames, stream, extra_flags, region, log2_scale=log2_scale)


def decode_region_scaled(frames: DeviceFrames, tables, region, log2_scale: int, out: Optional[torch.Tensor] = None,
                         stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0,
                         skip_rejected: bool = True) -> torch.Tensor:
    """decode_region at scale s = 2^log2_scale (0..3) in one launch (mh_decode_region_scaled): every
    s x s cell of the region becomes the mean of its pixels inside the frame, halves rounded up,
    and no full-size raster exists. -> out[n, SH, bw * c], c = 8 >> log2_scale, whose first SW
    columns are the picture ((SW, SH) = Region.scaled_size; the columns beyond, cells of a
    right-edge block outside the frame, are 0). tables, out and skip_rejected: decode_region's.
    log2_scale 0 is decode_region."""
    return _decode_region("decode_region_scaled", _log2_scale(log2_scale), frames, tables, region, out, stream,
                          extra_flags, skip_rejected)


def decode_scaled(frames: DeviceFrames, tables, log2_scale: int, out: Optional[torch.Tensor] = None,
                  stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0,
                  skip_rejected: bool = True) -> torch.Tensor:
    """The whole frame at scale 2^log2_scale: decode_region_scaled of the full block grid, returned
    as its [n, ceil(H / s), ceil(W / s)] view (`out`, when given, has the region's shape)."""
    gw, gh = block_grid(frames.width, frames.height)
    region = Region(0, 0, gw, gh)
    full = decode_region_scaled(frames, tables, region, log2_scale, out, stream, extra_flags, skip_rejected)
    sw, sh = region.scaled_size(frames.width, frames.height, log2_scale)
    return full.reshape(frames.n_frames, full.shape[-2], full.shape[-1])[:, :sh, :sw]


def decode_rect(frames: DeviceFrames, tables, x0: int, y0: int, w: int, h: int,
                out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                extra_flags: int = 0, skip_rejected: bool = True) -> torch.Tensor:
    """The pixel rectangle [x0, x0 + w) x [y0, y0 + h) of every frame: decode_region of the
    blocks that cover it (region_of_rect), returned as the [n, h, w] view of that raster (`out`,
    when given, has the region's shape)."""
    region, dx, dy = region_of_rect(frames.width, frames.height, x0, y0, w, h)
    full = decode_region(frames, tables, region, out, stream, extra_flags, skip_rejected)
    return full.reshape(frames.n_frames, full.shape[-2], full.shape[-1])[:, dy: dy + h, dx: dx + w]


def windows_of_rects(width: int, height: int, frame_idx, x0, y0, w: int, h: int) -> tuple:
    """n pixel rectangles of ONE size w x h, rectangle i at (x0[i], y0[i]) of frame frame_idx[i]
    (arrays of one length) of width x height frames -> (windows int64[n, 3] of (frame, bx0, by0),
    (bw, bh), dx[n], dy[n]) for decode_windows: rectangle i is out[i, dy[i]: dy[i] + h, dx[i]: dx[i] + w].
    Every window starts at its rectangle's block (region_of_rect's rounding), and (bw, bh) is the
    smallest block size that holds every rectangle at its own sub-block offset (dx, dy). Pure.
    ValueError when a rectangle is empty or leaves the frame, or when a window grown to (bw, bh)
    leaves the block grid."""
    width, height, w, h = (int(v) for v in (width, height, w, h))
    if width < 1 or height < 1:
        raise ValueError("an empty frame")
    f, x0, y0 = (np.atleast_1d(np.asarray(v)).astype(np.int64) for v in (frame_idx, x0, y0))
    if not (f.ndim == x0.ndim == y0.ndim == 1 and f.size == x0.size == y0.size and f.size >= 1):
        raise ValueError("frame_idx, x0 and y0 are arrays of one length >= 1")
    bad = (x0 < 0) | (y0 < 0) | (x0 + w > width) | (y0 + h > height) | (f < 0)
    if w < 1 or h < 1 or bad.any():
        i = int(np.flatnonzero(bad)[0]) if bad.any() else 0
        raise ValueError(f"rectangle {i}: {w}x{h} at ({int(x0[i])}, {int(y0[i])}) of frame {int(f[i])} lies outside "
                         f"the {width}x{height} frame")
    bx0, by0 = x0 // 8, y0 // 8
    bw = int(((x0 + w + 7) // 8 - bx0).max())
    bh = int(((y0 + h + 7) // 8 - by0).max())
    gw, gh = block_grid(width, height)
    out = (bx0 + bw > gw) | (by0 + bh > gh)
    if out.any():
        i = int(np.flatnonzero(out)[0])
        raise ValueError(f"rectangle {i}: its window of {bw}x{bh} blocks at block ({int(bx0[i])}, {int(by0[i])}) "
                         f"leaves the {gw}x{gh} block grid")
    return np.stack([f, bx0, by0], axis=1), (bw, bh), x0 - 8 * bx0, y0 - 8 * by0


def _window_size(frames: DeviceFrames, size) -> tuple:
    bw, bh = (int(v) for v in size)
    gw, gh = block_grid(frames.width, frames.height)
    if bw < 1 or bh < 1 or bw > gw or bh > gh:
        raise ValueError(f"a window of {bw}x{bh} blocks does not fit the {gw}x{gh} block grid")
    return bw, bh


def _host_list(frames: DeviceFrames, items, noun: str, origin: str, w: int, h: int, unit: str, limits: tuple,
               of: str):
    """A descriptor list checked on the host: a device tensor's type and shape only (it is not read: no
    host sync, the kernel validates it) -> None; a host sequence of (frame, `origin`) -> its int32 [n, 4]
    descriptor array, or ValueError when a `noun` of w x h `unit` names no frame or leaves `limits`."""
    if isinstance(items, torch.Tensor) and items.is_cuda:
        dev = frames.codes.device
        if (items.device != dev or items.dtype is not torch.int32 or items.dim() != 2
                or items.shape[1] not in (3, 4) or items.shape[0] < 1):
            raise ValueError(f"a device {noun}s tensor is int32 [n, 3] or [n, 4] on {dev}")
        return None
    a = np.asarray(items.numpy() if isinstance(items, torch.Tensor) else items)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1 or a.dtype.kind not in "iu":
        raise ValueError(f"{noun}s is a sequence of (frame, {origin}) integers")
    a = a.astype(np.int64)
    lw, lh = limits
    if isinstance(lw, np.ndarray):  # a frame set: one size per frame, every item against its own frame's
        f = np.clip(a[:, 0], 0, frames.n_frames - 1)
        lw, lh = lw[f], lh[f]
    bad = ((a < 0).any(axis=1) | (a[:, 0] >= frames.n_frames) | (a[:, 1] + w > lw) | (a[:, 2] + h > lh))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        if isinstance(lw, np.ndarray):
            lw, lh = int(lw[i]), int(lh[i])
        raise ValueError(f"{noun} {i} = {tuple(int(v) for v in a[i])} of {w}x{h} {unit} lies outside the "
                         f"{frames.n_frames} frames of {lw}x{lh}{of}")
    full = np.zeros((a.shape[0], 4), np.int32)
    full[:, :3] = a
    return full


def _host_windows(frames: DeviceFrames, windows, bw: int, bh: int):
    """decode_windows' `windows` checked on the host (_host_list) against the frames and the block grid."""
    return _host_list(frames, windows, "window", "bx0, by0", bw, bh, "blocks",
                      block_grid(frames.width, frames.height), " blocks")


def _windows_tensor(frames: DeviceFrames, windows, host) -> torch.Tensor:
    """The int32 [n, 4] descriptor array on the frames' device, 16-byte aligned: the upload of a
    checked host list (_host_windows), or the caller's device tensor -- as it is when it is [n, 4],
    contiguous and aligned."""
    if host is not None:
        return torch.from_numpy(host).to(frames.codes.device)
    if windows.shape[1] == 3:
        windows = torch.nn.functional.pad(windows, (0, 1))
    if not windows.is_contiguous() or windows.data_ptr() % 16:
        windows = windows.clone(memory_format=torch.contiguous_format)
    return windows


def decode_windows_shape(frames: DeviceFrames, n_windows: int, size,
                         stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0) -> tuple:
    """(workgroups per window, waves per workgroup) decode_windows would launch n_windows windows
    of size = (bw, bh) blocks with (mh_decode_windows_shape)."""
    return _slice_shape("mh_decode_windows_shape", frames, stream, extra_flags, windows=(n_windows, size))


_NO_STREAM = contextlib.nullcontext()  # (reusable: one per call costs what two function calls do)


def _decode_list(who: str, entry: str, frames: DeviceFrames, tables, items, host, mid: tuple, slot: tuple, dtype,
                 strides: tuple, out, status, stream, extra_flags: int, skip_rejected: bool, head: tuple = ()):
    """What the window and crop entries share behind their own checks: the frame entry, the tables, the
    descriptor array, the default ZERO-FILLED raster [n, *slot] of `dtype` and the status tensor (all made
    under `stream`), `out` and `status` checked, and one launch of the C entry `entry`, which takes `mid`
    between the descriptor count and the tables and, behind the rasters, their byte `strides` (row, [plane,]
    slot), and `head` (a frame set's geometry records and block count) right behind the frame.
    `host`: _host_list's result for `items`. Called once per batch: no loop, no list, no closure."""
    fr, dev_index = _slice_entry(who, frames, extra_flags)
    luts, stride, fstatus = _region_tables(who, frames, tables, dev_index, skip_rejected)
    dev = frames.codes.device
    with torch.cuda.stream(stream) if stream is not None else _NO_STREAM:
        desc = _windows_tensor(frames, items, host)  # (an upload or a padded copy belongs to `stream`)
        n = int(desc.shape[0])
        shape = (n, *slot)
        if out is None:
            out = torch.zeros(shape, dtype=dtype, device=dev)
        lstatus = torch.empty(n, dtype=torch.int32, device=dev) if status is True else status
    if (out.dtype is not dtype or out.shape != shape or out.get_device() != dev_index
            or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {'uint8' if dtype is torch.uint8 else dtype} {list(shape)} "
                         f"tensor on cuda:{dev_index}")
    if lstatus is not None and (not isinstance(lstatus, torch.Tensor) or lstatus.dtype is not torch.int32
                                or lstatus.numel() != n or lstatus.get_device() != dev_index
                                or not lstatus.is_contiguous()):
        raise ValueError(f"status must be True or a contiguous int32 [{n}] tensor on cuda:{dev_index}")
    rc = getattr(N.lib(), entry)(ctypes.byref(fr), *head, desc.data_ptr(), n, *mid, luts.data_ptr(), stride,
                                 fstatus.data_ptr() if fstatus is not None else None,
                                 lstatus.data_ptr() if lstatus is not None else None, out.data_ptr(), *strides,
                                 _raw_stream_ptr(stream, dev_index))
    if rc:
        N.check(rc, entry)
    return (out, lstatus) if status is True else out


def _decode_windows(who: str, k: int, frames: DeviceFrames, tables, windows, size, out, status, stream,
                    extra_flags: int, skip_rejected: bool):
    """decode_windows (k = 0: the C entry takes no scale) and decode_windows_scaled."""
    bw, bh = _window_size(frames, size)
    c = 8 >> k
    host = _host_windows(frames, windows, bw, bh)
    return _decode_list(who, "mh_decode_windows_scaled" if k else "mh_decode_windows", frames, tables, windows, host,
                        (bw, bh, k) if k else (bw, bh), (c * bh, c * bw), torch.uint8, (c * bw, c * bh * c * bw),
                        out, status, stream, extra_flags, skip_rejected)


def decode_windows(frames: DeviceFrames, tables, windows, size, out: Optional[torch.Tensor] = None,
                   status=None, stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0,
                   skip_rejected: bool = True):
    """Decode a list of windows of one size = (bw, bh) in blocks, window p the blocks
    [bx0, bx0 + bw) x [by0, by0 + bh) of frame `frame`, into out[n_windows, 8 * bh, 8 * bw] in one
    launch (mh_decode_windows). Windows may overlap, repeat and name frames in any order.
    windows: an int32 tensor [n, 3] or [n, 4] of (frame, bx0, by0[, 0]) on the frames' device -- used as
    it is when [n, 4], contiguous and 16-byte aligned, never read on the host (no sync): the kernel
    validates every window and rejects, with status MH_ERR_DIMS and an untouched slot, one that
    names no frame or leaves the block grid -- or a host sequence / array of (frame, bx0, by0),
    validated here (ValueError) and uploaded.
    out: a contiguous uint8 [n, 8 * bh, 8 * bw] tensor on the frames' device; None allocates a
    ZERO-FILLED one, because the rows >= RH_p of a window at the frame's bottom edge (and a rejected
    or skipped window's whole slot) are never written. The first RW_p columns of a row are the picture.
    status: None; True to get (out, int32[n] per-window status); or an int32[n] device tensor that
    receives it (out is returned): MH_ERR_DIMS for a rejected window, the frame's non-zero status
    word for a window of a skipped frame, else 0.
    tables, extra_flags, skip_rejected: decode_region's (the table set's status is per frame)."""
    return _decode_windows("decode_windows", 0, frames, tables, windows, size, out, status, stream, extra_flags,
                           skip_rejected)


def decode_windows_scaled_shape(frames: DeviceFrames, n_windows: int, size, log2_scale: int,
                                stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0) -> tuple:
    """(workgroups per window, waves per workgroup) decode_windows_scaled would launch n_windows
    windows of size = (bw, bh) blocks with, at scale 2^log2_scale (mh_decode_windows_scaled_shape)."""
    return _slice_shape("mh_decode_windows_scaled_shape", frames, stream, extra_flags, windows=(n_windows, size),
                        log2_scale=log2_scale)


def decode_windows_scaled(frames: DeviceFrames, tables, windows, size, log2_scale: int,
                          out: Optional[torch.Tensor] = None, status=None,
                          stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0,
                          skip_rejected: bool = True):
    """decode_windows at scale s = 2^log2_scale (0..3) in one launch (mh_decode_windows_scaled): every
    s x s cell of a window becomes the mean of its pixels inside the frame, halves rounded up, as in
    decode_region_scaled, and no full-size raster exists. -> out[n_windows, bh * c, bw * c],
    c = 8 >> log2_scale. Window p's picture is its first SH_p rows and SW_p columns, (SW_p, SH_p) =
    Region(bx0, by0, bw, bh).scaled_size; the columns beyond SW_p in those rows are 0, and rows
    >= SH_p (and a rejected or skipped window's whole slot) are never written, so out = None
    allocates a ZERO-FILLED raster as decode_windows does.
    Rectangle i of windows_of_rects lies at out[i, dy[i] // s: (dy[i] + h) // s, dx[i] // s:
    (dx[i] + w) // s] -- exactly only when dx[i], dy[i], w and h are multiples of s: the cells are
    those of the frame's grid, and a cell the rectangle covers in part averages pixels outside it.
    windows, size, status, tables, extra_flags, skip_rejected: decode_windows'. log2_scale 0 is
    decode_windows."""
    k = _log2_scale(log2_scale)
    return _decode_windows("decode_windows_scaled", k, frames, tables, windows, size, out, status, stream,
                           extra_flags, skip_rejected)


def _crop_size(frames: DeviceFrames, size) -> tuple:
    w, h = (int(v) for v in size)
    if w < 1 or h < 1 or w > frames.width or h > frames.height:
        raise ValueError(f"a crop of {w}x{h} pixels does not fit the {frames.width}x{frames.height} frame")
    return w, h


def _host_crops(frames: DeviceFrames, crops, w: int, h: int):
    """decode_crops' `crops` checked on the host (_host_list) against the frames and their pixel size
    (a frame set: every crop against its own frame's)."""
    limits = frames.size_limits() if isinstance(frames, DeviceFrameSet) else (frames.width, frames.height)
    return _host_list(frames, crops, "crop", "x0, y0", w, h, "pixels", limits, "")


def decode_crops_shape(frames: DeviceFrames, n_crops: int, size,
                       stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0) -> tuple:
    """(workgroups per crop, waves per workgroup) decode_crops would launch n_crops crops of
    size = (w, h) pixels with (mh_decode_crops_shape)."""
    return _slice_shape("mh_decode_crops_shape", frames, stream, extra_flags, crops=(n_crops, size))


def decode_crops(frames: DeviceFrames, tables, crops, size, out: Optional[torch.Tensor] = None,
                 status=None, stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0,
                 skip_rejected: bool = True):
    """Decode a list of crops of one size = (w, h) in PIXELS, crop p the pixels [x0, x0 + w) x
    [y0, y0 + h) of frame `frame`, into out[n_crops, h, round_up(w, 8)] in one launch
    (mh_decode_crops): every crop starts at byte 0 of its own slot, whatever its origin's offset in
    the 8x8 block grid, so out[:, :, :w] is the batch -- dense when w is a multiple of 8. The decoder
    shifts each row in registers as it stores it; no larger raster and no gather pass exist. A crop
    lies wholly inside the frame (no clipping); crops may overlap, repeat and name frames in any order.
    crops: an int32 tensor [n, 3] or [n, 4] of (frame, x0, y0[, 0]) on the frames' device -- used as it
    is when [n, 4], contiguous and 16-byte aligned, never read on the host (no sync): the kernel
    validates every crop and rejects, with status MH_ERR_DIMS and an untouched slot, one that names
    no frame or leaves the frame -- or a host sequence / array of (frame, x0, y0), validated here
    (ValueError) and uploaded.
    out: a contiguous uint8 [n, h, round_up(w, 8)] tensor on the frames' device; None allocates a
    ZERO-FILLED one (a rejected or skipped crop's slot is never written). Columns >= w of a written
    row are unspecified.
    status, tables, extra_flags, skip_rejected: decode_windows'."""
    w, h = _crop_size(frames, size)
    host = _host_crops(frames, crops, w, h)
    pitch = (w + 7) // 8 * 8
    return _decode_list("decode_crops", "mh_decode_crops", frames, tables, crops, host, (w, h), (h, pitch),
                        torch.uint8, (pitch, h * pitch), out, status, stream, extra_flags, skip_rejected)


_NORM_DTYPES = (torch.float16, torch.bfloat16, torch.float32)  # indexed by MH_NORM_*


def _norm_raster(w: int, h: int, fmt: int, planes: tuple = ()) -> tuple:
    """A normalised entry's slot [(C,) h, round_up(w, 8)], its dtype and its byte strides (row, [plane,] slot)."""
    cols = (w + 7) // 8 * 8
    pitch = cols * (2, 2, 4)[fmt]
    return (*planes, h, cols), _NORM_DTYPES[fmt], (pitch, h * pitch, *(C * h * pitch for C in planes))


def _host_norm_crops(frames: DeviceFrames, crops, w: int, h: int):
    """decode_crops_normalized's `crops` checked on the host: _host_crops' rules for (frame, x0, y0),
    plus a fourth column of flags -- MH_CROP_MIRROR only, and only on a width that is a multiple of 8."""
    if isinstance(crops, torch.Tensor) and crops.is_cuda:
        return _host_crops(frames, crops, w, h)
    c = np.asarray(crops.numpy() if isinstance(crops, torch.Tensor) else crops)
    if c.ndim != 2 or c.shape[1] not in (3, 4) or c.shape[0] < 1 or c.dtype.kind not in "iu":
        raise ValueError("crops is a sequence of (frame, x0, y0) or (frame, x0, y0, flags) integers")
    full = _host_crops(frames, c[:, :3], w, h)
    if c.shape[1] == 4:
        flags = c[:, 3].astype(np.int64)
        bad = (flags & ~N.MH_CROP_MIRROR) != 0
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError(f"crop {i}: flags {int(flags[i]):#x} has bits other than MH_CROP_MIRROR")
        if (w % 8) and flags.any():
            i = int(np.flatnonzero(flags)[0])
            raise ValueError(f"crop {i}: MH_CROP_MIRROR needs a width that is a multiple of 8, not {w}")
        full[:, 3] = flags
    return full


def decode_crops_normalized_shape(frames: DeviceFrames, n_crops: int, size, dtype,
                                  stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0) -> tuple:
    """(workgroups per crop, waves per workgroup) decode_crops_normalized would launch n_crops crops
    of size = (w, h) pixels with, for `dtype` (mh_decode_crops_norm_shape)."""
    return _slice_shape("mh_decode_crops_norm_shape", frames, stream, extra_flags, crops=(n_crops, size, dtype))


def decode_crops_normalized(frames: DeviceFrames, tables, crops, size, dtype, scale: float = 1.0, bias: float = 0.0,
                            out: Optional[torch.Tensor] = None, status=None,
                            stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0,
                            skip_rejected: bool = True):
    """decode_crops straight into a model's input (mh_decode_crops_norm): crop p, the pixels [x0, x0 + w)
    x [y0, y0 + h) of frame `frame`, becomes out[p, :, :w] of torch.float16, bfloat16 or float32
    (`dtype`), every byte v as cvt(fma(float32(v), scale, bias)) -- one fused multiply-add in float32,
    then round-to-nearest-even to dtype; codec.norm_table gives the 256 values. The conversion, the
    affine map and the mirror are done on the row the decoder holds in registers: one launch, and no
    uint8 batch exists. Normalising by a mean and a standard deviation of [0, 1] pixels is
        scale = 1 / (255 * std), bias = -mean / std.
    -> out[n, h, round_up(w, 8)]; columns >= w of a written row are unspecified.
    crops: an int32 tensor [n, 4] of (frame, x0, y0, flags) on the frames' device -- used in place when
    contiguous and 16-byte aligned, never read on the host (no sync): the kernel rejects, with status
    MH_ERR_DIMS and an untouched slot, a crop that names no frame, leaves the frame, has a flag bit
    other than MH_CROP_MIRROR, or is mirrored at a width that is no multiple of 8 ([n, 3] is padded
    with flags 0) -- or a host sequence / array of (frame, x0, y0) or (frame, x0, y0, flags), validated
    here by the same rules (ValueError) and uploaded. flags = MH_CROP_MIRROR reverses the crop's rows:
    out[p, y, X] comes from pixel x0 + w - 1 - X.
    scale, bias: finite in float32 (ValueError).
    out: a contiguous [n, h, round_up(w, 8)] tensor of `dtype` on the frames' device; None allocates a
    ZERO-FILLED one (a rejected or skipped crop's slot is never written).
    status, tables, extra_flags, skip_rejected: decode_crops'."""
    w, h = _crop_size(frames, size)
    fmt = _norm_format(dtype)
    scale, bias = float(scale), float(bias)
    if not (finite_f32(scale) and finite_f32(bias)):
        raise ValueError(f"scale and bias must be finite in float32, not {scale!r}, {bias!r}")
    host = _host_norm_crops(frames, crops, w, h)
    return _decode_list("decode_crops_normalized", "mh_decode_crops_norm", frames, tables, crops, host,
                        (w, h, fmt, scale, bias), *_norm_raster(w, h, fmt), out, status, stream, extra_flags,
                        skip_rejected)


def _plane_coefficients(scale, bias):
    """decode_crops_normalized_planes' (scale, bias): two sequences of one length C, 1..MH_MAX_PLANES,
    every value finite in float32 -> (C, float[C] scale, float[C] bias) as ctypes arrays."""
    try:
        s, b = [float(v) for v in scale], [float(v) for v in bias]
    except TypeError:
        raise ValueError("scale and bias are sequences of one value per plane") from None
    if len(s) != len(b) or not 1 <= len(s) <= N.MH_MAX_PLANES:
        raise ValueError(f"scale and bias are sequences of one length, 1..{N.MH_MAX_PLANES} planes, "
                         f"not {len(s)} and {len(b)}")
    if not all(finite_f32(v) for v in s + b):
        raise ValueError(f"scale and bias must be finite in float32, not {s!r}, {b!r}")
    arr = ctypes.c_float * len(s)
    return len(s), arr(*s), arr(*b)


def _plane_stride(frames: DeviceFrames, n_planes: int, plane_stride) -> int:
    ps = int(plane_stride)
    if ps < 0 or ps > 0xFFFFFFFF or (n_planes - 1) * ps >= frames.n_frames:
        raise ValueError(f"{n_planes} planes {ps} frames apart do not fit the {frames.n_frames} frames")
    return ps


def _decode_planes(who: str, entry: str, frames: DeviceFrames, tables, crops, size, dtype, scale, bias, n_planes,
                   plane_stride, out, status, stream, extra_flags: int, skip_rejected: bool):
    """decode_crops_normalized_planes and its twin over a frame set (`frames` a DeviceFrameSet, which adds
    `n_planes`, the planes' size check of a host list and the set's `head`)."""
    w, h = _crop_size(frames, size)
    fmt = _norm_format(dtype)
    C, c_scale, c_bias = _plane_coefficients(scale, bias)
    if n_planes is not None and int(n_planes) != C:
        raise ValueError(f"n_planes = {n_planes}, but scale and bias hold {C} values")
    ps = _plane_stride(frames, C, plane_stride)
    host = _host_norm_crops(frames, crops, w, h)
    over_set = isinstance(frames, DeviceFrameSet)
    if host is not None:
        f0 = host[:, 0].astype(np.int64)
        bad = f0 + (C - 1) * ps >= frames.n_frames
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError(f"crop {i} = {tuple(int(v) for v in host[i])}: plane {C - 1} would be frame "
                             f"{int(host[i, 0]) + (C - 1) * ps} of {frames.n_frames}")
        if over_set:
            lw, lh = frames.size_limits()
            for c in range(1, C):
                bad = (lw[f0 + c * ps] != lw[f0]) | (lh[f0 + c * ps] != lh[f0])
                if bad.any():
                    i = int(np.flatnonzero(bad)[0])
                    raise ValueError(f"crop {i} = {tuple(int(v) for v in host[i])}: plane {c} (frame "
                                     f"{int(f0[i]) + c * ps}) is not of plane 0's size")
    head = frames._head(frames.codes.get_device()) if over_set else ()
    return _decode_list(who, entry, frames, tables, crops, host, (w, h, fmt, C, ps, c_scale, c_bias),
                        *_norm_raster(w, h, fmt, (C,)), out, status, stream, extra_flags, skip_rejected, head)


def decode_crops_normalized_planes_shape(frames: DeviceFrames, n_crops: int, size, dtype, n_planes: int,
                                         stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0) -> tuple:
    """(workgroups per (sample, plane) unit, waves per workgroup) decode_crops_normalized_planes would
    launch n_crops samples of n_planes planes of size = (w, h) pixels with, for `dtype`
    (mh_decode_crops_norm_planes_shape)."""
    return _slice_shape("mh_decode_crops_norm_planes_shape", frames, stream, extra_flags,
                        crops=(n_crops, size, dtype, n_planes))


def decode_crops_normalized_planes(frames: DeviceFrames, tables, crops, size, dtype, scale, bias,
                                   plane_stride: int = 1, out: Optional[torch.Tensor] = None, status=None,
                                   stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0,
                                   skip_rejected: bool = True):
    """decode_crops_normalized for images stored as C planes, one frame each, into a model's
    [n, C, h, w] input in one launch (mh_decode_crops_norm_planes). A crop (frame, x0, y0[, flags]) is a
    SAMPLE: its plane c is the crop at that origin, mirrored or not with the others, of frame
    `frame + c * plane_stride`, every byte v as cvt(fma(float32(v), scale[c], bias[c])).
    plane_stride is 1 for images stored plane after plane, the number of images for plane-major
    storage, and 0 for one gray frame under C different maps.
    -> out[n, C, h, round_up(w, 8)]; columns >= w of a written row are unspecified.
    scale, bias: sequences of one length C, 1..MH_MAX_PLANES, each value finite in float32
    (ValueError); codec.norm_coefficients makes them from a mean and a deviation per channel.
    crops: decode_crops_normalized's -- a device int32 [n, 4] tensor is used in place and never read on
    the host (the kernel rejects a sample, MH_ERR_DIMS and every plane untouched, whose last plane's
    frame does not exist); a host list is validated here by the same rules, and also needs
    frame + (C - 1) * plane_stride < n_frames (ValueError naming the crop).
    A sample is written whole or not at all: with a DeviceTableSet and skip_rejected, a sample any of
    whose C frames has a non-zero status word keeps every plane untouched, and its status is the
    first such word in plane order.
    out: a contiguous [n, C, h, round_up(w, 8)] tensor of `dtype` on the frames' device; None
    allocates a ZERO-FILLED one.
    status, tables, extra_flags, skip_rejected: decode_crops'."""
    return _decode_planes("decode_crops_normalized_planes", "mh_decode_crops_norm_planes", frames, tables, crops, size,
                          dtype, scale, bias, None, plane_stride, out, status, stream, extra_flags, skip_rejected)


def _frame_set(who: str, fs) -> "DeviceFrameSet":
    if not isinstance(fs, DeviceFrameSet):
        raise TypeError(f"{who} takes a DeviceFrameSet")
    return fs


def decode_set_crops_shape(fs: DeviceFrameSet, n_crops: int, size, stream: Optional[torch.cuda.Stream] = None,
                           extra_flags: int = 0) -> tuple:
    """(workgroups per crop, waves per workgroup) decode_set_crops would launch n_crops crops of
    size = (w, h) pixels with (mh_decode_set_crops_shape): the crop size and the device decide, not
    the frames' sizes."""
    return _slice_shape("mh_decode_set_crops_shape", _frame_set("decode_set_crops_shape", fs), stream, extra_flags,
                        crops=(n_crops, size))


def decode_set_crops(fs: DeviceFrameSet, tables, crops, size, out: Optional[torch.Tensor] = None,
                     status=None, stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0,
                     skip_rejected: bool = True):
    """decode_crops over a frame SET (mh_decode_set_crops): crop p is the pixels [x0, x0 + w) x
    [y0, y0 + h) of frame `frame`, whatever that frame's size, and crops of frames of any mix of sizes
    are decoded into out[n_crops, h, round_up(w, 8)] in ONE launch -- no grouping of a sampled batch by
    image size, no launch per size.
    size: (w, h) in pixels, at most the set's largest width and height (ValueError). A crop that does
    not fit its OWN frame is rejected per crop: on the device for a device tensor (status MH_ERR_DIMS,
    the slot untouched), here (ValueError) for a host list.
    tables: a DeviceTableSet with one table per frame of the set, or one DeviceTables for all.
    crops, out, status, extra_flags, skip_rejected: decode_crops'."""
    fs = _frame_set("decode_set_crops", fs)
    w, h = _crop_size(fs, size)
    host = _host_crops(fs, crops, w, h)
    pitch = (w + 7) // 8 * 8
    head = fs._head(fs.codes.get_device())
    return _decode_list("decode_set_crops", "mh_decode_set_crops", fs, tables, crops, host, (w, h), (h, pitch),
                        torch.uint8, (pitch, h * pitch), out, status, stream, extra_flags, skip_rejected, head)


def decode_set_crops_normalized_planes_shape(fs: DeviceFrameSet, n_crops: int, size, dtype, n_planes: int,
                                             stream: Optional[torch.cuda.Stream] = None,
                                             extra_flags: int = 0) -> tuple:
    """(workgroups per (sample, plane) unit, waves per workgroup) decode_set_crops_normalized_planes
    would launch with (mh_decode_set_crops_norm_planes_shape)."""
    return _slice_shape("mh_decode_set_crops_norm_planes_shape",
                        _frame_set("decode_set_crops_normalized_planes_shape", fs), stream, extra_flags,
                        crops=(n_crops, size, dtype, n_planes))


def decode_set_crops_normalized_planes(fs: DeviceFrameSet, tables, crops, size, dtype, scale, bias,
                                       n_planes: Optional[int] = None, plane_stride: int = 1,
                                       out: Optional[torch.Tensor] = None, status=None,
                                       stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0,
                                       skip_rejected: bool = True):
    """decode_crops_normalized_planes over a frame SET (mh_decode_set_crops_norm_planes): samples of
    images of any mix of sizes, each stored as C planes of ONE size, into a normalised
    out[n, C, h, round_up(w, 8)] in one launch. With one plane (scale and bias of length 1) it is
    decode_crops_normalized over a set.
    n_planes: None, or C = len(scale) said again (ValueError when they differ).
    A sample whose C frames are not of one size, or that does not fit them, is rejected whole: on the
    device for a device tensor (MH_ERR_DIMS, no plane written), here (ValueError) for a host list.
    Everything else -- crops, flags, scale, bias, plane_stride, out, status, tables -- is
    decode_crops_normalized_planes', with `tables` as in decode_set_crops."""
    fs = _frame_set("decode_set_crops_normalized_planes", fs)
    return _decode_planes("decode_set_crops_normalized_planes", "mh_decode_set_crops_norm_planes", fs, tables, crops,
                          size, dtype, scale, bias, n_planes, plane_stride, out, status, stream, extra_flags,
                          skip_rejected)


def decode_set_frames_shape(fs: DeviceFrameSet, stream: Optional[torch.cuda.Stream] = None,
                            extra_flags: int = 0) -> tuple:
    """(workgroups resident on the device at once, waves per workgroup) of decode_set_frames' kernel
    (mh_decode_set_frames_shape): the group budget its planner is given."""
    fr, dev_index = _slice_entry("decode_set_frames_shape", _frame_set("decode_set_frames_shape", fs), extra_flags)
    r, w = ctypes.c_uint32(0), ctypes.c_uint32(0)
    N.check(N.lib().mh_decode_set_frames_shape(ctypes.byref(fr), _raw_stream_ptr(stream, dev_index), ctypes.byref(r),
                                               ctypes.byref(w)), "mh_decode_set_frames_shape")
    return int(r.value), int(w.value)


@dataclasses.dataclass
class DeviceSetPlan:
    """A codec.DecodeSetPlan uploaded for decode_set_frames: the two record arrays, the group map,
    and the host copy the frame views are cut by."""
    plan: DecodeSetPlan
    rasters: torch.Tensor      # u32 as int32[n, 4]
    shares: torch.Tensor       # u32 as int32[n, 4]
    group_frame: torch.Tensor  # u32 as int32[n_groups]

    @classmethod
    def upload(cls, plan: DecodeSetPlan, device="cuda") -> "DeviceSetPlan":
        dev = _dev(device)
        up = [torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev)
              for a in (plan.rasters, plan.shares, plan.group_frame)]
        return cls(plan, *up)


def _set_plan(fs: DeviceFrameSet, plan, dev_index: int, stream, extra_flags: int) -> DeviceSetPlan:
    """decode_set_frames' plan argument -> an uploaded plan: None plans from the set's host geometry
    with the kernel's resident workgroups as the budget, once per set and kernel (cached on `fs`)."""
    if isinstance(plan, DeviceSetPlan):
        return plan
    dev = fs.codes.device
    with torch.cuda.stream(stream) if stream is not None else _NO_STREAM:
        if plan is not None:
            return DeviceSetPlan.upload(plan, dev)
        key = (fs.sizes, extra_flags & N.MH_FLAG_NO_DELTA, dev_index)
        cached = fs.__dict__.get("_set_plan")
        if cached is None or cached[0] != key:
            budget = decode_set_frames_shape(fs, stream, extra_flags)[0]
            geoms = np.asarray([(0, w, h, 0) for w, h in fs.sizes], np.uint32)
            cached = fs.__dict__["_set_plan"] = (key, DeviceSetPlan.upload(decode_set_plan(geoms, budget), dev))
        return cached[1]


def decode_set_frames(fs: DeviceFrameSet, tables, plan=None, out: Optional[torch.Tensor] = None,
                      frame_status: Optional[torch.Tensor] = None, status=None,
                      stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0):
    """Every frame of a SET whole, each at its own size, in ONE launch (mh_decode_set_frames): the
    images themselves from the set encoder's output, without regrouping the frames by size.
    tables: a DeviceTableSet with one table per frame of the set, or one DeviceTables for all.
    plan: a codec.DecodeSetPlan (uploaded here) or a DeviceSetPlan -- where each frame is written and
    how the launch's workgroups are shared out; None plans from the set's sizes with one resident
    round of the device as the budget and keeps the uploaded plan on `fs`. The device validates every
    record: a frame whose raster record is rejected gets status MH_ERR_CAPACITY, one whose geometry is
    rejected MH_ERR_DIMS, and neither is written.
    out: a contiguous uint8 tensor of at least plan.out_bytes bytes on the set's device, 8-byte
    aligned; None allocates a ZERO-FILLED one.
    frame_status: int32[n] on the device, a non-zero word skips the frame (its raster untouched); None
    takes a DeviceTableSet's build status.
    status: True allocates, or an int32 [n] tensor receives, a word per frame (MH_OK, the two codes
    above, or the frame's non-zero status word).
    Returns a list of n uint8 tensors, frame f an [H_f, W_f] view into `out` (row stride the frame's
    pitch); with `status`, (frames, status). Asynchronous on `stream`; no host synchronisation."""
    fs = _frame_set("decode_set_frames", fs)
    fr, dev_index = _slice_entry("decode_set_frames", fs, extra_flags)
    luts, stride, fstatus = _region_tables("decode_set_frames", fs, tables, dev_index, frame_status is None)
    if frame_status is not None:
        _status_arg("frame_status", frame_status, fs, dev_index)
        fstatus = frame_status
    d_geoms, total_blocks = fs._head(dev_index)
    dp = _set_plan(fs, plan, dev_index, stream, extra_flags)
    p, n = dp.plan, fs.n_frames
    if (dp.rasters.shape != (n, 4) or dp.shares.shape != (n, 4) or dp.group_frame.numel() != p.n_groups
            or any(t.get_device() != dev_index or t.dtype is not torch.int32 or not t.is_contiguous()
                   for t in (dp.rasters, dp.shares, dp.group_frame))):
        raise ValueError(f"the plan must hold {n} raster and share records and its group map on cuda:{dev_index}")
    with torch.cuda.stream(stream) if stream is not None else _NO_STREAM:
        if out is None:
            out = torch.zeros(p.out_bytes, dtype=torch.uint8, device=fs.codes.device)
        sstatus = torch.empty(n, dtype=torch.int32, device=fs.codes.device) if status is True else status
    if (out.dtype is not torch.uint8 or out.get_device() != dev_index or not out.is_contiguous()
            or out.numel() < p.out_bytes):
        raise ValueError(f"out must be a contiguous uint8 tensor of at least {p.out_bytes} bytes on cuda:{dev_index}")
    if sstatus is not None:
        _status_arg("status", sstatus, fs, dev_index)
    rc = N.lib().mh_decode_set_frames(ctypes.byref(fr), d_geoms, total_blocks, dp.rasters.data_ptr(),
                                      dp.shares.data_ptr(), dp.group_frame.data_ptr(), p.n_groups, luts.data_ptr(),
                                      stride, fstatus.data_ptr() if fstatus is not None else None,
                                      sstatus.data_ptr() if sstatus is not None else None, out.data_ptr(),
                                      out.numel(), _raw_stream_ptr(stream, dev_index))
    if rc:
        N.check(rc, "mh_decode_set_frames")
    base = out.storage_offset()  # as_strided counts from the storage's start, not from the view's
    offs, pitches = p.offsets, p.pitches
    frames = [out.as_strided((h, w), (int(pitches[f]), 1), base + int(offs[f])) for f, (w, h) in enumerate(fs.sizes)]
    return (frames, sstatus) if status is not None else frames


def decode_headers_shape(frames: DeviceFrames, stream: Optional[torch.cuda.Stream] = None,
                         extra_flags: int = 0) -> tuple:
    """(workgroups per frame, waves per workgroup) decode_headers would launch with
    (mh_decode_headers_shape)."""
    return _slice_shape("mh_decode_headers_shape", frames, stream, extra_flags)


def decode_headers(frames: DeviceFrames, canons, out: Optional[torch.Tensor] = None,
                   frame_status: Optional[torch.Tensor] = None, header_status: Optional[torch.Tensor] = None,
                   stream: Optional[torch.cuda.Stream] = None, extra_flags: int = 0) -> torch.Tensor:
    """Decode a batch straight from its canonical headers (mh_decode_headers): frame f's table is
    built inside the decode kernel from canons[f] -- no DeviceTableSet. canons: device u8[n, 256]
    tensor, or a host array (uploaded here). frame_status (optional int32[n] on the device): a
    non-zero word skips the frame. header_status (optional int32[n] on the device, not the same
    tensor): receives each decoded frame's verdict, 0, -3 or -5; a rejected frame's raster is
    left untouched. Returns the device raster out[n, H, pitch] (decode()'s `out` contract)."""
    fr, dev_index = _slice_entry("decode_headers", frames, extra_flags)
    dev = frames.codes.device
    hdr = _header_tensor(canons, dev, convert=False)
    if (hdr.dtype is not torch.uint8 or hdr.dim() != 2 or tuple(hdr.shape) != (frames.n_frames, 256)
            or hdr.get_device() != dev_index or not hdr.is_contiguous()):
        raise ValueError(f"canons must be a contiguous uint8 [{frames.n_frames}, 256] tensor on cuda:{dev_index}")
    for name, st in (("frame_status", frame_status), ("header_status", header_status)):
        if st is not None and (st.dtype is not torch.int32 or st.numel() != frames.n_frames
                               or st.get_device() != dev_index or not st.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous int32 [{frames.n_frames}] tensor on cuda:{dev_index}")
    pitch = (frames.width + 7) // 8 * 8
    h = frames.height
    out = _out_raster(frames, out, h, pitch, dev_index, stream)
    sp = _raw_stream_ptr(stream, dev_index)
    rc = N.lib().mh_decode_headers(ctypes.byref(fr), hdr.data_ptr(),
                                   frame_status.data_ptr() if frame_status is not None else None,
                                   header_status.data_ptr() if header_status is not None else None,
                                   out.data_ptr(), pitch, h * pitch, sp)
    if rc:
        N.check(rc, "mh_decode_headers")
    frames.__dict__["_hdr_keep"] = hdr  # read by the launch in flight
    return out


def _status_arg(name: str, st: Optional[torch.Tensor], frames: DeviceFrames, dev_index: int) -> None:
    if st is not None and (st.dtype is not torch.int32 or st.numel() != frames.n_frames
                           or st.get_device() != dev_index or not st.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous int32 [{frames.n_frames}] tensor on cuda:{dev_index}")


def _check_outputs(frames: DeviceFrames, stream: Optional[torch.cuda.Stream]) -> tuple:
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        rep = torch.empty((frames.n_frames, 4), dtype=torch.int32, device=frames.codes.device)
        verdict = torch.empty(frames.n_frames, dtype=torch.int32, device=frames.codes.device)
    return rep, verdict


def check_frames(frames: DeviceFrames, tables, frame_status: Optional[torch.Tensor] = None,
                 stream: Optional[torch.cuda.Stream] = None) -> tuple:
    """check() for a batch with a table per frame (mh_check_frames): tables is a DeviceTableSet, or a
    DeviceTables with its prepared table (one table for all frames). Returns (report, verdict) on the
    device: the report as check() returns it, int64 [n, 4]; the verdict int32 [n], 0 for a frame whose
    report is clean and MH_ERR_STREAM otherwise, which the decode entries take as frame_status as it
    is, on the same stream without a sync. frame_status (int32 [n]; None: the table set's own status):
    a frame whose word is non-zero is not walked, its report is clean and its verdict that word."""
    fr, dev_index = _slice_entry("check_frames", frames, 0)
    luts, stride, own = _region_tables("check_frames", frames, tables, dev_index, True)
    status = own if frame_status is None else frame_status
    _status_arg("frame_status", status, frames, dev_index)
    rep, verdict = _check_outputs(frames, stream)
    rc = N.lib().mh_check_frames(ctypes.byref(fr), luts.data_ptr(), stride,
                                 status.data_ptr() if status is not None else None, rep.data_ptr(),
                                 verdict.data_ptr(), _raw_stream_ptr(stream, dev_index))
    if rc:
        N.check(rc, "mh_check_frames")
    return rep.to(torch.int64) & 0xFFFFFFFF, verdict


def check_headers(frames: DeviceFrames, canons, frame_status: Optional[torch.Tensor] = None,
                  stream: Optional[torch.cuda.Stream] = None) -> tuple:
    """check_frames straight from the canonical headers (mh_check_headers; canons as decode_headers
    takes them). Returns (report, verdict, header_status): a rejected header is not walked, its
    report is clean, and its verdict and header_status word are the header's code (-3 or -5)."""
    fr, dev_index = _slice_entry("check_headers", frames, 0)
    hdr = _header_tensor(canons, frames.codes.device, convert=False)
    if (hdr.dtype is not torch.uint8 or hdr.dim() != 2 or tuple(hdr.shape) != (frames.n_frames, 256)
            or hdr.get_device() != dev_index or not hdr.is_contiguous()):
        raise ValueError(f"canons must be a contiguous uint8 [{frames.n_frames}, 256] tensor on cuda:{dev_index}")
    _status_arg("frame_status", frame_status, frames, dev_index)
    rep, verdict = _check_outputs(frames, stream)
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        # a skipped frame's word is not written by the kernel: 0, as its header was not judged
        header_status = torch.zeros(frames.n_frames, dtype=torch.int32, device=frames.codes.device)
    rc = N.lib().mh_check_headers(ctypes.byref(fr), hdr.data_ptr(),
                                  frame_status.data_ptr() if frame_status is not None else None,
                                  header_status.data_ptr(), rep.data_ptr(), verdict.data_ptr(),
                                  _raw_stream_ptr(stream, dev_index))
    if rc:
        N.check(rc, "mh_check_headers")
    frames.__dict__["_hdr_keep"] = hdr  # read by the launch in flight
    return rep.to(torch.int64) & 0xFFFFFFFF, verdict, header_status


def _decode_frames_host(encoded: Sequence[EncodedFrame], device="cuda") -> np.ndarray:
    t1, t2 = encoded[0].tables()
    tabs = DeviceTables.upload(t1, t2, device)
    frames = DeviceFrames.pack(encoded, device)
    out = decode(frames, tabs)
    return out[..., : frames.width].cpu().numpy()


def decode_frames_mixed(encoded: Sequence[EncodedFrame], device="cuda") -> np.ndarray:
    """Convenience for frames with different headers: upload, build the tables on the
    device, decode in one launch, copy back; returns [n, H, W] uint8 on the host. Raises
    MHError when a header is rejected."""
    frames = DeviceFrames.pack(encoded, device, shared_table=False)
    tabs = DeviceTableSet.from_canonical_headers(np.stack([np.asarray(f.canon, np.uint8) for f in encoded]),
                                                 frames.codes.device)
    out = decode_frames(frames, tabs)
    tabs.check_status()
    return out[..., : frames.width].cpu().numpy()
