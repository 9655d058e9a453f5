"""GPU encoder: a device frame in, the reference's buffers out (mh_encode_frame_device).

Byte-identical to the host codec (codec.encode_frame), so frames encoded on the GPU
feed the decoder -- and the reference's own renderer contract -- unchanged.
Encoder.encode returns the header and byte count on the host (one synchronisation);
Encoder.encode_async (mh_encode_frame_device_async) leaves everything on the device,
so an encode -> table build -> decode chain never waits on the host.
"""
from __future__ import annotations

import contextlib
import ctypes
import dataclasses
from typing import Optional

import numpy as np
import torch

from . import _native as N
from .codec import block_grid
from .decoder import DeviceFrames, _dev, _header_tensor, _stream_ptr


def _limit(limit_lengths: bool) -> int:
    return N.MH_ENCODE_LIMIT_LENGTHS if limit_lengths else 0


@dataclasses.dataclass
class DeviceEncodedFrame:
    width: int
    height: int
    canon: np.ndarray                 # u8[256] canonical header (host)
    codes: torch.Tensor               # u8[codes_len] on the device (payload + 4 zero bytes)
    block_offsets: torch.Tensor       # int32 view of u32[NB] on the device
    block_init: Optional[torch.Tensor]
    flags: int

    @property
    def payload_bytes(self) -> int:
        return int(self.codes.numel()) - N.MH_CODES_PAD

    def frames(self) -> DeviceFrames:
        """The encoded frame as a one-frame DeviceFrames for decode()."""
        return DeviceFrames(self.width, self.height, 1, self.block_offsets, self.codes, None,
                            self.block_init, self.flags, self.payload_bytes)


def _workspace_ptr(workspace: torch.Tensor) -> tuple:
    """(the workspace's first 256-byte aligned address, the bytes from there to its end)."""
    base = workspace.data_ptr()
    aligned = (base + 255) // 256 * 256
    return aligned, workspace.numel() - (aligned - base)


class Encoder:
    """Reusable device workspace + output buffers for frames of one size. Calls on
    one stream queue up behind each other; frames in flight on several streams need
    one Encoder (one workspace) per stream."""

    def __init__(self, width: int, height: int, device="cuda"):
        self.device = _dev(device)
        self.width, self.height = width, height
        bw, bh = block_grid(width, height)
        self.nb = bw * bh
        ws = int(N.lib().mh_encode_workspace_bytes(width, height))
        # zero-filled once: every encode leaves the histogram zeroed for the next, so
        # the calls pass MH_ENCODE_WORKSPACE_ZEROED and skip the per-call clear
        self.workspace = torch.zeros(ws + 256, dtype=torch.uint8, device=self.device)
        self.cap = (self.nb * 64 * 2 + N.MH_CODES_PAD + 3) // 4 * 4 + 16

    def _check_gray(self, gray: torch.Tensor) -> None:
        if gray.dtype != torch.uint8 or gray.shape != (self.height, self.width) or not gray.is_contiguous():
            raise ValueError(f"gray must be contiguous uint8 [{self.height}, {self.width}]")

    def encode(self, gray: torch.Tensor, flags: int = 0, init_zero_delta: bool = False,
               stream: Optional[torch.cuda.Stream] = None, limit_lengths: bool = False) -> DeviceEncodedFrame:
        """limit_lengths (here and in encode_async): a tree deeper than 16 gets the
        length-limited code on the device (MH_ENCODE_LIMIT_LENGTHS) instead of status -3.
        The keyword goes to the encoder only, never into the frame's `flags`."""
        self._check_gray(gray)
        gray = gray.to(self.device)
        codes = torch.empty(self.cap, dtype=torch.uint8, device=self.device)
        offs = torch.empty(self.nb, dtype=torch.int32, device=self.device)
        init = torch.empty(self.nb, dtype=torch.uint8, device=self.device) if init_zero_delta else None
        canon = np.zeros(256, np.uint8)
        n = ctypes.c_uint64(0)
        N.check(N.lib().mh_encode_frame_device(
            gray.data_ptr(), self.width, self.height, flags | N.MH_ENCODE_WORKSPACE_ZEROED | _limit(limit_lengths),
            canon.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), codes.data_ptr(), self.cap,
            ctypes.byref(n), offs.data_ptr(), init.data_ptr() if init is not None else None,
            *_workspace_ptr(self.workspace), _stream_ptr(stream, self.device)),
            "mh_encode_frame_device")
        return DeviceEncodedFrame(self.width, self.height, canon, codes[: n.value], offs, init, flags)

    def encode_async(self, gray: torch.Tensor, flags: int = 0, init_zero_delta: bool = False,
                     stream: Optional[torch.cuda.Stream] = None,
                     codes: Optional[torch.Tensor] = None, limit_lengths: bool = False) -> AsyncEncodedFrame:
        """Enqueue the encode on `stream` (default: the current stream) and return
        at once. `gray` must be ready on that stream (make it wait on the stream
        that produced the frame). `codes` may be a reused u8 buffer of at least the
        encoder's capacity (the default allocates one)."""
        self._check_gray(gray)
        if gray.device != self.device:
            raise ValueError("gray must live on the encoder's device")
        # outputs belong to the stream the kernels run on (the caching allocator must
        # not hand their memory out again while that stream still writes it)
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            if codes is None:
                codes = torch.empty(self.cap, dtype=torch.uint8, device=self.device)
            offs = torch.empty(self.nb, dtype=torch.int32, device=self.device)
            init = torch.empty(self.nb, dtype=torch.uint8, device=self.device) if init_zero_delta else None
            canon = torch.empty(256, dtype=torch.uint8, device=self.device)
            meta = torch.empty(2, dtype=torch.int64, device=self.device)   # [codes_len, status]
        if codes.dtype != torch.uint8 or codes.device != self.device or codes.numel() < 4:
            raise ValueError("codes must be a uint8 buffer on the encoder's device")
        N.check(N.lib().mh_encode_frame_device_async(
            gray.data_ptr(), self.width, self.height, flags | N.MH_ENCODE_WORKSPACE_ZEROED | _limit(limit_lengths),
            canon.data_ptr(), codes.data_ptr(),
            codes.numel(), meta.data_ptr(), offs.data_ptr(), init.data_ptr() if init is not None else None,
            meta.data_ptr() + 8, *_workspace_ptr(self.workspace),
            _stream_ptr(stream, self.device)), "mh_encode_frame_device_async")
        return AsyncEncodedFrame(self.width, self.height, canon, codes, meta[0:1],
                                 meta[1:2].view(torch.int32)[0:1], offs, init, flags)


@dataclasses.dataclass
class AsyncEncodedFrame:
    """An encode still in flight on the device: header, byte count and status are
    device tensors. frames()/tables() chain the decode without a host sync;
    result() synchronises and returns the DeviceEncodedFrame (raising MHError on
    a rejected frame)."""
    width: int
    height: int
    canon: torch.Tensor               # u8[256] on the device
    codes: torch.Tensor               # u8[capacity] on the device (first codes_len bytes used)
    codes_len: torch.Tensor           # int64[1] on the device (0 on an error)
    status: torch.Tensor              # int32[1] on the device
    block_offsets: torch.Tensor
    block_init: Optional[torch.Tensor]
    flags: int

    def frames(self) -> DeviceFrames:
        """A one-frame DeviceFrames over the whole code buffer (the decoder bounds
        the last block by its offset, not by the buffer size)."""
        return DeviceFrames(self.width, self.height, 1, self.block_offsets, self.codes, None,
                            self.block_init, self.flags, int(self.codes.numel()) - N.MH_CODES_PAD)

    def tables(self, prepare_lut: bool = True, stream: Optional[torch.cuda.Stream] = None):
        """T1/T2 (+ prepared table) built on the device from the device header."""
        from .decoder import DeviceTables
        return DeviceTables.from_canonical_header(self.canon, self.canon.device, prepare_lut, stream)

    def result(self) -> DeviceEncodedFrame:
        st, n = int(self.status.item()), int(self.codes_len.item())
        N.check(st, "mh_encode_frame_device_async")
        return DeviceEncodedFrame(self.width, self.height, self.canon.cpu().numpy(), self.codes[:n],
                                  self.block_offsets, self.block_init, self.flags)


class BatchEncoder:
    """n_frames frames of one size per call (mh_encode_frames_device_async): each frame
    gets its own histogram, tree and codes (byte-identical to codec.encode_frame, frame
    by frame), in three launches whatever n_frames. Codes land in fixed 16-byte
    aligned slots of `slot` bytes (the capacity), so the result is one DeviceFrames
    batch: AsyncEncodedBatch.decode() decodes it with a table per frame, decode() when the
    frames share a table (e.g. block shuffles)."""

    def __init__(self, width: int, height: int, n_frames: int, device="cuda"):
        self.device = _dev(device)
        self.width, self.height, self.n = width, height, n_frames
        bw, bh = block_grid(width, height)
        self.nb = bw * bh
        # one workspace for both entry points: whichever needs more
        ws = max(int(N.lib().mh_encode_frames_workspace_bytes(width, height, n_frames)),
                 int(N.lib().mh_encode_frames_shared_workspace_bytes(width, height, n_frames)))
        # zero-filled once: every call leaves the histograms zeroed (MH_ENCODE_WORKSPACE_ZEROED)
        self.workspace = torch.zeros(ws + 256, dtype=torch.uint8, device=self.device)
        self.slot = (self.nb * 64 * 2 + N.MH_CODES_PAD + 15) // 16 * 16 + 16

    def _encode_batch(self, entry: str, source: tuple, *, shared: bool, header, flags: int, init_zero_delta: bool,
                      stream: Optional[torch.cuda.Stream], limit_lengths: bool,
                      plane_fields: tuple = (1, 1)) -> "AsyncEncodedBatch":
        """The four methods' body: the outputs (allocated on the stream the kernels run on), the
        call of library entry `entry`, whose first arguments are `source`, and the batch.
        shared: one table (`header`: None to build it, else 256 code lengths, a device tensor or
        a host array); plane_fields: the batch's (n_planes, plane_frame_stride)."""
        n, dev = self.n, self.device
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            codes = torch.empty(n * self.slot + 16, dtype=torch.uint8, device=dev)
            offs = torch.empty(n * self.nb, dtype=torch.int32, device=dev)
            init = torch.empty(n * self.nb, dtype=torch.uint8, device=dev) if init_zero_delta else None
            canon = torch.empty(256 if shared else (n, 256), dtype=torch.uint8, device=dev)
            lens = torch.empty(n, dtype=torch.int64, device=dev)
            fco = torch.empty(n + 1, dtype=torch.int64, device=dev)
            status = torch.empty(n + 1 if shared else n, dtype=torch.int32, device=dev)  # shared, [n]: the header's verdict
            canon_in = _header_tensor(header, dev) if header is not None else None
            if canon_in is not None and canon_in.numel() != 256:
                raise ValueError("header must hold 256 code lengths")
        cbase = (codes.data_ptr() + 15) // 16 * 16
        tables = (canon_in.data_ptr() if canon_in is not None else None, canon.data_ptr()) if shared else (canon.data_ptr(),)
        verdicts = (status.data_ptr(), status.data_ptr() + 4 * n) if shared else (status.data_ptr(),)
        N.check(getattr(N.lib(), entry)(
            *source, self.width, self.height, flags | N.MH_ENCODE_WORKSPACE_ZEROED | _limit(limit_lengths), *tables,
            cbase, self.slot, lens.data_ptr(), fco.data_ptr(), offs.data_ptr(),
            init.data_ptr() if init is not None else None, *verdicts, *_workspace_ptr(self.workspace),
            _stream_ptr(stream, dev)), entry)
        view = codes[cbase - codes.data_ptr(): cbase - codes.data_ptr() + n * self.slot]
        return AsyncEncodedBatch(self.width, self.height, n, self.slot, canon, view, lens, fco, status[:n], offs, init,
                                 flags, shared=shared, header_status=status[n:] if shared else None,
                                 n_planes=plane_fields[0], plane_frame_stride=plane_fields[1])

    def _check_grays(self, grays: torch.Tensor) -> tuple:
        """The frames methods' input check -> the entries' first arguments."""
        if (grays.dtype != torch.uint8 or tuple(grays.shape) != (self.n, self.height, self.width)
                or not grays.is_contiguous()):
            raise ValueError(f"grays must be contiguous uint8 [{self.n}, {self.height}, {self.width}]")
        if grays.device != self.device:
            raise ValueError("grays must live on the encoder's device")
        return grays.data_ptr(), self.height * self.width, self.n

    def encode_async(self, grays: torch.Tensor, flags: int = 0, init_zero_delta: bool = False,
                     stream: Optional[torch.cuda.Stream] = None, limit_lengths: bool = False) -> "AsyncEncodedBatch":
        """grays: contiguous uint8 [n, H, W] on the encoder's device, ready on `stream`.
        limit_lengths: frames whose tree is deeper than 16 get the length-limited code
        (MH_ENCODE_LIMIT_LENGTHS) instead of status -3; the batch's `flags` do not carry it."""
        return self._encode_batch("mh_encode_frames_device_async", self._check_grays(grays), shared=False, header=None,
                                  flags=flags, init_zero_delta=init_zero_delta, stream=stream,
                                  limit_lengths=limit_lengths)

    def encode_shared_async(self, grays: torch.Tensor, header=None, flags: int = 0, init_zero_delta: bool = False,
                            stream: Optional[torch.cuda.Stream] = None,
                            limit_lengths: bool = False) -> "AsyncEncodedBatch":
        """All frames under ONE Huffman table (mh_encode_frames_shared_device_async): what
        decoder.decode, the table-mode streams and the multi-GPU paths consume.
        header=None builds the table from the batch's summed histogram (codec.shared_header
        of the frames; limit_lengths as in encode_async); otherwise `header` -- 256 code
        lengths, a device tensor or a host array -- is validated and used as it is (a header
        fixed for a sequence, an earlier batch's, one broadcast before encoding). The result
        is marked `shared`: `canon` is the one header (u8[256] on the device),
        `header_status` its verdict (int32[1] on the device), `status` the per-frame words
        (-5 for a frame that holds a symbol the header has no code for)."""
        return self._encode_batch("mh_encode_frames_shared_device_async", self._check_grays(grays), shared=True,
                                  header=header, flags=flags, init_zero_delta=init_zero_delta, stream=stream,
                                  limit_lengths=limit_lengths)

    def _image_layout(self, images: torch.Tensor, plane_major: bool, first_channel: int, n_planes):
        """The images methods' input check -> the entries' first arguments -- the address, the
        mh_image_layout of a uint8 [n, H, W, K] tensor with channel stride 1 and any other strides (a
        window of a larger batch, RGB of RGBA, padded rows) and the image count -- and the batch's
        (n_planes, plane_frame_stride)."""
        if images.dtype != torch.uint8 or images.dim() != 4:
            raise ValueError("images must be a uint8 tensor [n, H, W, K]")
        n, h, w, k = images.shape
        c = k - first_channel if n_planes is None else int(n_planes)
        if first_channel < 0 or c < 1 or first_channel + c > k:
            raise ValueError(f"planes {first_channel}..{first_channel + c - 1} of {k}-channel pixels")
        if (h, w) != (self.height, self.width) or n * c != self.n:
            raise ValueError(f"images must be [n, {self.height}, {self.width}, K] with n * n_planes == {self.n}")
        if k > 1 and images.stride(3) != 1:
            raise ValueError("the channels of a pixel must be adjacent bytes (stride 1)")
        if images.device != self.device:
            raise ValueError("images must live on the encoder's device")
        # a dimension of size 1 may carry any stride: the library ignores the image stride and the
        # row pitch there, and a one-pixel row needs a pixel stride that holds its channels
        ps = images.stride(2) if w > 1 else max(images.stride(2), k)
        lay = N.mh_image_layout(images.stride(0), images.stride(1), ps, first_channel, c, 1 if plane_major else 0)
        return (images.data_ptr(), ctypes.byref(lay), n), (c, n if plane_major else 1)

    def encode_images_async(self, images: torch.Tensor, plane_major: bool = False, first_channel: int = 0,
                            n_planes=None, flags: int = 0, init_zero_delta: bool = False,
                            stream: Optional[torch.cuda.Stream] = None,
                            limit_lengths: bool = False) -> "AsyncEncodedBatch":
        """encode_async reading interleaved pixels in place (mh_encode_images_device_async): `images`
        is uint8 [n, H, W, K] with adjacent channels and ANY other strides -- imgs[:, y0:y1, x0:x1, :3]
        of an RGBA batch goes in without a copy -- and the encoder was built for n_frames = n * C
        frames, C = n_planes (default: the channels from first_channel on). Plane c of image i is
        frame i * C + c, or c * n + i with plane_major; each is byte-identical to codec.encode_frame
        of codec.image_planes(images, ...)[frame]. The batch carries n_planes and
        plane_frame_stride for decoder.decode_crops_normalized_planes."""
        source, plane_fields = self._image_layout(images, plane_major, first_channel, n_planes)
        return self._encode_batch("mh_encode_images_device_async", source, shared=False, header=None, flags=flags,
                                  init_zero_delta=init_zero_delta, stream=stream, limit_lengths=limit_lengths,
                                  plane_fields=plane_fields)

    def encode_images_shared_async(self, images: torch.Tensor, header=None, plane_major: bool = False,
                                   first_channel: int = 0, n_planes=None, flags: int = 0,
                                   init_zero_delta: bool = False, stream: Optional[torch.cuda.Stream] = None,
                                   limit_lengths: bool = False) -> "AsyncEncodedBatch":
        """encode_shared_async reading interleaved pixels in place
        (mh_encode_images_shared_device_async): ONE table for all n * C plane frames, built from
        their summed histogram (header=None: codec.shared_header of codec.image_planes(images, ...))
        or supplied. `images`, the frame order and the batch's plane fields as in
        encode_images_async; `header` and the result as in encode_shared_async."""
        source, plane_fields = self._image_layout(images, plane_major, first_channel, n_planes)
        return self._encode_batch("mh_encode_images_shared_device_async", source, shared=True, header=header,
                                  flags=flags, init_zero_delta=init_zero_delta, stream=stream,
                                  limit_lengths=limit_lengths, plane_fields=plane_fields)


@dataclasses.dataclass
class AsyncEncodedBatch:
    """A batched encode in flight: everything on the device (per-frame slots).

    Host synchronisation: frames() synchronises the stream once by default (check=True,
    since round 5: it reads `status` and `codes_len`); a pipeline that overlaps encode with
    decode must call frames(check=False), which stays asynchronous, and check `status`
    itself. frame(f) always synchronises."""
    width: int
    height: int
    n_frames: int
    slot: int
    canon: torch.Tensor               # u8[n, 256]
    codes: torch.Tensor               # u8[n * slot]
    codes_len: torch.Tensor           # int64[n] (payload + MH_CODES_PAD; 0 on an error)
    frame_code_offsets: torch.Tensor  # int64[n + 1] = f * slot
    status: torch.Tensor              # int32[n]
    block_offsets: torch.Tensor       # int32 view of u32[n * NB]
    block_init: Optional[torch.Tensor]
    flags: int
    shared: bool = False              # encode_shared_async: ONE table; canon is then u8[256]
    header_status: Optional[torch.Tensor] = None  # shared: int32[1] on the device, the header's verdict
    n_planes: int = 1            # encode_images_*: the planes taken per image (frames = images * n_planes)
    plane_frame_stride: int = 1  # ... and the frames from a plane of an image to its next plane

    def frames(self, check: bool = True) -> DeviceFrames:
        """All slots as one DeviceFrames batch: for decoder.decode_frames with table_set()
        (a table per frame), or for decoder.decode when the frames share a table.

        check=True (default) synchronises once: it raises MHError if any frame was
        rejected (that frame's slot and block offsets were never written, so decoding
        the batch would read garbage), and `code_bytes` is the batch's payload bytes
        (sum of codes_len minus the pads), as for DeviceFrames.pack. check=False stays
        asynchronous: the caller must check `status` before trusting a decode of the
        batch, and `code_bytes` is then the slots' capacity (n * slot minus the pads),
        an upper bound of the payload."""
        if check:
            st = self.status.cpu()
            bad = [i for i in range(self.n_frames) if int(st[i])]
            if bad:
                what = "mh_encode_frames_shared_device_async" if self.shared else "mh_encode_frames_device_async"
                raise N.MHError(int(st[bad[0]]), f"{what}: frame(s) {bad[:8]} rejected")
            payload = int(self.codes_len.sum().item()) - self.n_frames * N.MH_CODES_PAD
        else:
            payload = int(self.codes.numel()) - self.n_frames * N.MH_CODES_PAD
        return DeviceFrames(self.width, self.height, self.n_frames, self.block_offsets, self.codes,
                            self.frame_code_offsets, self.block_init, self.flags, payload)

    def tables(self, prepare_lut: bool = True, stream: Optional[torch.cuda.Stream] = None):
        """A shared batch's one table: T1/T2 (+ the prepared table) built on the device from
        the device header (DeviceTables.from_canonical_header); asynchronous."""
        if not self.shared:
            raise ValueError("a batch with a table per frame has no single table: use table_set()")
        from .decoder import DeviceTables
        return DeviceTables.from_canonical_header(self.canon, self.canon.device, prepare_lut, stream)

    def table_set(self, stream: Optional[torch.cuda.Stream] = None):
        """One prepared table per frame, built on the device from the device headers in one
        launch (mh_build_luts_device); asynchronous. Its status is the encoder's word where
        the encoder rejected the frame (the header of such a frame is unspecified), else the
        table build's -- combined on the device, so decode() skips exactly those frames.
        A shared batch has one table: ValueError, use tables()."""
        if self.shared:
            raise ValueError("a shared batch has one table: use tables(), not table_set()")
        from .decoder import DeviceTableSet
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            ts = DeviceTableSet.from_canonical_headers(self.canon, self.canon.device, stream)
            ts.status = torch.where(self.status != 0, self.status, ts.status)
        return ts

    def decode(self, out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None):
        """encode batch -> n tables -> decode batch on one stream, no host synchronisation:
        returns the raster [n, H, pitch] (decode()'s `out` contract). A rejected frame is skipped
        on the device (its raster keeps what `out` held); the tables stay in `self.tables`, whose
        check_status() synchronises and names such frames.

        A shared batch (encode_shared_async) decodes through decoder.decode (mh_decode) with
        its one table, built on the device on the same stream. mh_decode cannot skip single
        frames, so this path does NOT stay asynchronous: it calls frames(check=True), which
        synchronises once and raises MHError if any frame (or the header) was rejected; the
        table build and the decode follow. A pipeline that must not synchronise checks
        `status` itself and calls decoder.decode(frames(check=False), tables(stream=...))."""
        if self.shared:
            from .decoder import decode
            fr = self.frames(check=True)
            self.shared_tables = self.tables(stream=stream)
            return decode(fr, self.shared_tables, out=out, stream=stream)
        from .decoder import decode_frames
        self.tables = self.table_set(stream)
        return decode_frames(self.frames(check=False), self.tables, out=out, stream=stream)

    def check(self, stream: Optional[torch.cuda.Stream] = None) -> tuple:
        """(report, verdict) of decoder.check_frames for the batch on `stream`, no host
        synchronisation: under table_set() (kept in `self.checked_tables`), or a shared batch
        under its one table with the encoder's status. A frame the encoder or the table build
        rejected is not walked and keeps that word as its verdict; the verdict goes into the
        decode entries' frame_status as it is."""
        from .decoder import check_frames
        frames = self.frames(check=False)
        if self.shared:
            self.checked_tables = self.tables(stream=stream)
            return check_frames(frames, self.checked_tables, frame_status=self.status, stream=stream)
        self.checked_tables = self.table_set(stream)
        return check_frames(frames, self.checked_tables, stream=stream)

    def frame(self, f: int) -> DeviceEncodedFrame:
        """Frame f (synchronises; raises MHError on a rejected frame)."""
        st, n = int(self.status[f].item()), int(self.codes_len[f].item())
        N.check(st, "mh_encode_frames_device_async")
        nb = self.block_offsets.numel() // self.n_frames
        init = self.block_init[f * nb:(f + 1) * nb] if self.block_init is not None else None
        canon = self.canon if self.shared else self.canon[f]
        return DeviceEncodedFrame(self.width, self.height, canon.cpu().numpy(),
                                  self.codes[f * self.slot: f * self.slot + n],
                                  self.block_offsets[f * nb:(f + 1) * nb], init, self.flags)


def encode_frame_device(gray: torch.Tensor, flags: int = 0, init_zero_delta: bool = False,
                        limit_lengths: bool = False) -> DeviceEncodedFrame:
    """One-shot GPU encode of a [H, W] uint8 device tensor."""
    h, w = gray.shape
    return Encoder(w, h, gray.device).encode(gray, flags, init_zero_delta, limit_lengths=limit_lengths)


def default_slot_bytes(width: int, height: int) -> int:
    """BatchEncoder's slot rule for one frame size: the worst case of 16 bits per symbol plus the
    pad, rounded up to 16 bytes, and 16 more."""
    bw, bh = block_grid(width, height)
    return (bw * bh * 64 * 2 + N.MH_CODES_PAD + 15) // 16 * 16 + 16


def _plane_source(i: int, p: torch.Tensor, dev: torch.device) -> tuple:
    """(address, row pitch, pixel stride, width, height) of one 2-D uint8 device view."""
    if not isinstance(p, torch.Tensor) or p.dtype != torch.uint8 or p.dim() != 2:
        raise ValueError(f"plane {i}: a 2-D uint8 tensor is required")
    if p.device != dev:
        raise ValueError(f"plane {i}: all planes must live on one HIP device")
    h, w = p.shape
    if not (1 <= w <= N.MH_MAX_DIM and 1 <= h <= N.MH_MAX_DIM):
        raise ValueError(f"plane {i}: {w}x{h} is outside 1..{N.MH_MAX_DIM}")
    # a dimension of size 1 may carry any stride: it is never stepped over
    pitch = p.stride(0) if h > 1 else 0
    ps = p.stride(1) if w > 1 else 1
    if (h > 1 and pitch < 1) or not 1 <= ps <= 255:
        raise ValueError(f"plane {i}: strides {tuple(p.stride())} -- rows need a positive stride, pixels one of 1..255")
    return p.data_ptr(), pitch, ps, w, h


def encode_set_async(planes, flags: int = 0, init_zero_delta: bool = False,
                     stream: Optional[torch.cuda.Stream] = None, limit_lengths: bool = False,
                     slot_bytes=None, n_planes: int = 1) -> "AsyncEncodedSet":
    """Encode frames of DIFFERENT sizes, each under its own table, straight into the frame-set layout
    in three launches (mh_encode_set_device_async): `planes` is a sequence of 2-D uint8 device
    tensors or views with positive strides (img[..., c] of an HWC image, a window of a larger
    picture), ready on `stream`. Every accepted frame is byte-identical to codec.encode_frame of that
    plane. slot_bytes: one value or one per frame, multiples of 16 (default: BatchEncoder's rule for
    each frame's size). The plan is made on the host and uploaded; nothing waits for the device.
    n_planes: recorded on the result for the planes decode entries (frames i * n_planes + c)."""
    planes = list(planes)
    if not planes:
        raise ValueError("no planes")
    dev = planes[0].device if isinstance(planes[0], torch.Tensor) else None
    if dev is None or dev.type != "cuda":
        raise ValueError("the planes must be tensors on a HIP device")
    heads = [_plane_source(i, p, dev) for i, p in enumerate(planes)]
    n = len(heads)
    if slot_bytes is None:
        caps = [default_slot_bytes(s[3], s[4]) for s in heads]
    elif isinstance(slot_bytes, int):
        caps = [slot_bytes] * n
    else:
        caps = [int(c) for c in slot_bytes]
        if len(caps) != n:
            raise ValueError(f"{len(caps)} slot sizes for {n} planes")
    from .codec import encode_set_plan
    full_flags = flags | N.MH_ENCODE_WORKSPACE_ZEROED | _limit(limit_lengths)
    host = encode_set_plan([s + (c,) for s, c in zip(heads, caps)], full_flags)
    t = host.totals
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        plan = torch.from_numpy(host.plan).to(dev)
        codes = torch.empty(t.codes_bytes + 16, dtype=torch.uint8, device=dev)
        offs = torch.empty(t.total_blocks, dtype=torch.int32, device=dev)
        init = torch.empty(t.total_blocks, dtype=torch.uint8, device=dev) if init_zero_delta else None
        canon = torch.empty((n, 256), dtype=torch.uint8, device=dev)
        lens = torch.empty(n, dtype=torch.int64, device=dev)
        fco = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        workspace = torch.empty(t.workspace_bytes + 256, dtype=torch.uint8, device=dev)
    if plan.data_ptr() % 16:
        raise RuntimeError("the uploaded plan is not 16-byte aligned")
    cbase = (codes.data_ptr() + 15) // 16 * 16
    N.check(N.lib().mh_encode_set_device_async(
        plan.data_ptr(), ctypes.byref(t), full_flags, canon.data_ptr(), cbase, t.codes_bytes, lens.data_ptr(),
        fco.data_ptr(), offs.data_ptr(), init.data_ptr() if init is not None else None, status.data_ptr(),
        *_workspace_ptr(workspace), _stream_ptr(stream, dev)), "mh_encode_set_device_async")
    view = codes[cbase - codes.data_ptr(): cbase - codes.data_ptr() + t.codes_bytes]
    es = AsyncEncodedSet(tuple((s[3], s[4]) for s in heads), tuple(caps), plan, t, canon, view, lens, fco, status, offs,
                         init, flags, n_planes, 1)
    es._alive = (planes, workspace, codes)  # read and written by the launches in flight
    return es


def encode_image_set_async(images, n_planes=None, first_channel: int = 0, flags: int = 0,
                           init_zero_delta: bool = False, stream: Optional[torch.cuda.Stream] = None,
                           limit_lengths: bool = False, slot_bytes=None) -> "AsyncEncodedSet":
    """encode_set_async over interleaved images of different sizes: `images` is a sequence of uint8
    [H_i, W_i, K] device tensors (any strides encode_set_async takes), C = n_planes planes are taken
    from first_channel on (default: all behind it), and frame i * C + c is plane c of image i
    (plane_frame_stride 1), read in place."""
    images = list(images)
    if not images:
        raise ValueError("no images")
    k = None
    for i, im in enumerate(images):
        if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3:
            raise ValueError(f"image {i}: a uint8 tensor [H, W, K] is required")
        if k is not None and im.shape[2] != k:
            raise ValueError(f"image {i}: {im.shape[2]} channels, the others have {k}")
        k = int(im.shape[2])
    c = k - first_channel if n_planes is None else int(n_planes)
    if first_channel < 0 or c < 1 or first_channel + c > k:
        raise ValueError(f"planes {first_channel}..{first_channel + c - 1} of {k}-channel pixels")
    planes = [im[:, :, first_channel + j] for im in images for j in range(c)]
    if slot_bytes is not None and not isinstance(slot_bytes, int):
        slot_bytes = [int(s) for s in slot_bytes for _ in range(c)] if len(slot_bytes) == len(images) else slot_bytes
    return encode_set_async(planes, flags, init_zero_delta, stream, limit_lengths, slot_bytes, n_planes=c)


@dataclasses.dataclass
class AsyncEncodedSet:
    """A set encode in flight: everything on the device, in the frame-set layout. No method here
    synchronises; `status` (int32[n], 0 = accepted) goes in as frame_status of the set decode
    entries, and table_set() already carries it."""
    sizes: tuple                      # ((width, height), ...) per frame
    slots: tuple                      # each frame's code slot in bytes
    plan: torch.Tensor                # u8: the uploaded plan (records, geometry, maps)
    totals: "N.mh_set_totals"
    canon: torch.Tensor               # u8[n, 256]
    codes: torch.Tensor               # u8[codes_bytes]
    codes_len: torch.Tensor           # int64[n] (payload + MH_CODES_PAD; 0 on an error)
    frame_code_offsets: torch.Tensor  # int64[n + 1]: the slots' offsets, written by the device
    status: torch.Tensor              # int32[n]
    block_offsets: torch.Tensor       # int32 view of u32[total_blocks]
    block_init: Optional[torch.Tensor]
    flags: int
    n_planes: int = 1
    plane_frame_stride: int = 1

    @property
    def n_frames(self) -> int:
        return len(self.sizes)

    @property
    def geoms(self) -> torch.Tensor:
        """int32[n, 4]: the mh_frame_geom records, a view into the uploaded plan."""
        o, n = int(self.totals.geoms_offset), self.n_frames
        return self.plan[o: o + 16 * n].view(torch.int32).view(n, 4)

    def frame_set(self):
        """The outputs as a DeviceFrameSet for decode_set_crops and
        decode_set_crops_normalized_planes; `code_bytes` is the slots' capacity (an upper bound of
        the payload: the byte counts are on the device)."""
        from .decoder import DeviceFrameSet
        t = self.totals
        return DeviceFrameSet(int(t.max_width), int(t.max_height), self.n_frames, self.sizes, int(t.total_blocks),
                              self.block_offsets, self.codes, self.frame_code_offsets, self.geoms, self.block_init,
                              self.flags, int(self.codes.numel()) - self.n_frames * N.MH_CODES_PAD)

    def table_set(self, stream: Optional[torch.cuda.Stream] = None):
        """One prepared table per frame from the device headers in one launch
        (mh_build_luts_device); its status is the encoder's word where the encoder rejected the
        frame, else the table build's -- combined on the device."""
        from .decoder import DeviceTableSet
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            ts = DeviceTableSet.from_canonical_headers(self.canon, self.canon.device, stream)
            ts.status = torch.where(self.status != 0, self.status, ts.status)
        return ts

    def decode(self, out: Optional[torch.Tensor] = None, status=None,
               stream: Optional[torch.cuda.Stream] = None):
        """encode set -> n tables -> every frame decoded whole at its own size, on one stream with
        no host synchronisation (decoder.decode_set_frames, one launch): a list of n uint8 [H_f, W_f]
        views into `out` (with `status`, also the int32[n] status tensor). A frame the encoder or
        the table build rejected is skipped on the device and its raster keeps what `out` held (zeros
        when allocated here); the tables stay in `self.tables`, the frame set in `self.decoded_set`."""
        from .decoder import decode_set_frames
        self.tables = self.table_set(stream)
        self.decoded_set = self.__dict__.get("decoded_set") or self.frame_set()
        return decode_set_frames(self.decoded_set, self.tables, out=out, status=status, stream=stream)
