"""A raw-ABI driver for the two image encode entries (test_gpu_encode_images.py,
test_gpu_encode_images_sweep.py, test_encode_images_abi.py): mh_encode_images_device_async ("batch")
and mh_encode_images_shared_device_async ("shared_built", "shared_supplied"), called through ctypes with
the interleaved pixels at any byte offset, row pitch and image stride inside a garbage-filled buffer
and every output inside encode_helpers' guard-filled tensors.

The standard is the host codec on codec.image_planes of the pixels, frame by frame: the Run objects
made here carry n_images * C frames, so encode_helpers.expect / check / check_untouched / round_trip
apply as they stand."""
from __future__ import annotations

import ctypes
import dataclasses
from typing import Optional

import numpy as np

import encode_helpers as EH

ENTRIES = EH.BATCHED            # "batch", "shared_built", "shared_supplied"
SPAN_MAX = 0x7FFFFFF0           # MH_IMAGE_TILE_SPAN_MAX


@dataclasses.dataclass(frozen=True)
class Pixels:
    """How the images sit in memory. Image i starts at base + delta + i * image_stride (base 256-byte
    aligned); row_pitch None = W * ps, image_stride None = the image's span (H - 1) * pitch + W * ps
    plus `gap` bytes of garbage."""
    ps: int = 3                 # pixel stride
    fc: int = 0                 # first channel
    C: int = 3                  # planes taken
    plane_major: bool = False
    delta: int = 0
    pitch_pad: int = 0          # row_pitch = W * ps + pitch_pad
    gap: int = 0

    def pitch(self, w):
        return w * self.ps + self.pitch_pad

    def span(self, w, h):
        return (h - 1) * self.pitch(w) + w * self.ps

    def image_stride(self, w, h):
        return self.span(w, h) + self.gap

    def wide(self, w, h, n):
        """Whether the library takes the dword loads (image_mode of mh_encode.hip)."""
        a = self.delta | (self.image_stride(w, h) if n > 1 else 0) | (self.pitch(w) if h > 1 else 0)
        return self.ps <= 4 and a % 4 == 0


def tile_rows(w):
    """MH_IMAGE_TILE_ROWS(w)."""
    return 8 * (254 // ((w + 7) // 8) + 2)


def layout_struct(px, w, h, **over):
    from metalhuffman_amd import _native as N
    f = dict(image_stride=px.image_stride(w, h), row_pitch=px.pitch(w), pixel_stride=px.ps, first_channel=px.fc,
             n_planes=px.C, plane_major=1 if px.plane_major else 0)
    f.update(over)
    return N.mh_image_layout(**f)


def pixel_array(frames, px, seed=2):
    """[n, H, W, ps] pixels whose taken channels are the given plane frames (n * C of them, in image
    order i * C + c whatever px.plane_major) and whose other channels are seeded garbage."""
    h, w = frames[0].shape
    n = len(frames) // px.C
    assert n * px.C == len(frames) and px.fc + px.C <= px.ps
    pix = np.random.default_rng([seed, w, h, n, px.ps, px.fc]).integers(0, 256, (n, h, w, px.ps), dtype=np.uint8)
    for i in range(n):
        for c in range(px.C):
            pix[i, :, :, px.fc + c] = frames[i * px.C + c]
    return pix


def pixel_bytes(pix, px, seed=1):
    """The pixels laid out as px says inside seeded garbage -> (u8 host buffer whose byte 0 is to be
    256-byte aligned, offset of image 0, bool mask of the bytes that are selected samples). Garbage
    in front of image 0, in the row padding, in the other channels, between images and behind the
    last: every byte the contract lets the kernels load is inside the buffer."""
    n, h, w, ps = pix.shape
    assert ps == px.ps
    pitch, istride = px.pitch(w), px.image_stride(w, h)
    size = px.delta + (n - 1) * istride + px.span(w, h) + 256
    buf = np.random.default_rng([seed, w, h, n, px.delta, pitch, istride]).integers(0, 256, size, dtype=np.uint8)
    mask = np.zeros(size, bool)
    rows = px.delta + np.arange(n)[:, None, None, None] * istride + np.arange(h)[None, :, None, None] * pitch + \
        np.arange(w)[None, None, :, None] * ps + np.arange(ps)[None, None, None, :]
    buf[rows] = pix
    mask[rows[..., px.fc:px.fc + px.C]] = True
    return buf, px.delta, mask


def upload(device, buf):
    """The host buffer on the device with its byte 0 at a 256-byte boundary -> (tensor, address of byte 0)."""
    import torch
    t = torch.empty(buf.size + 256, dtype=torch.uint8, device=device)
    o = (t.data_ptr() + 255) // 256 * 256 - t.data_ptr()
    t[o: o + buf.size].copy_(torch.from_numpy(buf))
    return t, t.data_ptr() + o


def planes(mh, pix, px):
    """The plane frames in the call's frame order: the definition, codec.image_planes."""
    return list(mh.image_planes(pix, px.fc, px.C, px.plane_major))


def run(mh, device, entry, pix, px, *, flags=0, init_zero=False, layout=EH.Layout(), slot=None, header=None,
        ws_fill=None, buf=None, dev=None, lay_over=None, launches=True, rounds=2):
    """Two rounds of one call over one workspace into fresh guarded outputs -> [Run, Run] of
    n_images * C frames (encode_helpers.run's contract). buf: the host bytes to use instead of
    pixel_bytes(pix, px) (the padding-independence test). dev: (tensor, address of image 0) of pixels
    already on the device (layouts too large to build on the host). lay_over: layout fields the call is told
    instead of the truth (refusals: launches False)."""
    import torch
    L = mh.lib()
    assert entry in ENTRIES and (header is not None) == (entry == "shared_supplied")
    n_img, h, w, _ = pix.shape
    n = n_img * px.C
    bw, bh = EH.blocks(w, h)
    nb = bw * bh
    slot = EH.roomy_slot(w, h) if slot is None else slot
    assert slot % 16 == 0 and layout.codes_off % 16 == 0
    shared = entry in EH.SHARED
    wsb = int((L.mh_encode_images_shared_workspace_bytes if shared else L.mh_encode_images_workspace_bytes)(w, h, n_img, px.C))
    assert wsb == EH.workspace_bytes(mh, entry, w, h, n)
    ws = torch.zeros(wsb + 256, dtype=torch.uint8, device=device)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    fl = flags | (EH.ZEROED if ws_fill is None else 0)
    wsp = (ws.data_ptr() + 255) // 256 * 256
    if dev is not None:
        pix_t, p0 = dev[0], dev[1] - px.delta
    else:
        if buf is None:
            buf, _, _ = pixel_bytes(pix, px)
        pix_t, p0 = upload(device, buf)
    lay = layout_struct(px, w, h, **(lay_over or {}))
    cin = torch.from_numpy(np.ascontiguousarray(header, np.uint8)).to(device) if header is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    runs = []
    for _ in range(rounds if launches else 1):
        o = dict(codes=EH._Out(device, n * slot, layout.codes_off, EH.FILL_BYTES),
                 offs=EH._Out(device, n * nb * 4, layout.offs_off, EH.FILL_U32),
                 canon=EH._Out(device, 256 if shared else 256 * n, layout.canon_off, EH.FILL_BYTES),
                 lens=EH._Out(device, 8 * n, layout.len_off, EH.FILL_U64),
                 st=EH._Out(device, 4 * n, layout.status_off, EH.FILL_STATUS),
                 fco=EH._Out(device, 8 * (n + 1), layout.len_off, EH.FILL_U64))
        if init_zero:
            o["init"] = EH._Out(device, n * nb, layout.init_off, EH.FILL_BYTES)
        if shared:
            o["hst"] = EH._Out(device, 4, layout.status_off, EH.FILL_STATUS)
        initp = o["init"].ptr if init_zero else None
        if not shared:
            rc = L.mh_encode_images_device_async(
                p0 + px.delta, ctypes.byref(lay), n_img, w, h, fl, o["canon"].ptr, o["codes"].ptr, slot, o["lens"].ptr,
                o["fco"].ptr, o["offs"].ptr, initp, o["st"].ptr, wsp, wsb, stream)
        else:
            rc = L.mh_encode_images_shared_device_async(
                p0 + px.delta, ctypes.byref(lay), n_img, w, h, fl, cin.data_ptr() if cin is not None else None,
                o["canon"].ptr, o["codes"].ptr, slot, o["lens"].ptr, o["fco"].ptr, o["offs"].ptr, initp, o["st"].ptr,
                o["hst"].ptr, wsp, wsb, stream)
        torch.cuda.synchronize(device)
        host = {k: v.host(f"{entry}: {k}") for k, v in o.items()}
        runs.append(EH.Run(entry, n, w, h, nb, slot, flags, init_zero, int(rc), host, o))
    del pix_t
    return runs


def run_checked(mh, device, entry, pix, px, *, flags=0, init_zero=False, layout=EH.Layout(), slot=None, header=None,
                ws_fill=None, decode=True):
    """run + the host codec on codec.image_planes + check (+ the device round trip) -> (round 2, Expected)."""
    frames = planes(mh, pix, px)
    if entry == "shared_supplied" and header is None:
        header = EH.supplied_header(frames, flags, init_zero)
    runs = run(mh, device, entry, pix, px, flags=flags, init_zero=init_zero, layout=layout, slot=slot, header=header,
               ws_fill=ws_fill)
    exp = EH.expect(mh, entry, frames, flags=flags, init_zero=init_zero, slot=runs[0].slot, header=header)
    what = f"{entry}, {pix.shape[2]} x {pix.shape[1]}, n {pix.shape[0]}, {px}"
    try:
        EH.check(mh, runs, frames, exp)
        if decode:
            EH.round_trip(mh, device, runs[1], frames, exp)
    except AssertionError as err:
        raise AssertionError(f"{what}: {err}") from err
    return runs[1], exp


def natural_pixels(bigbridge, w, h, n_img, px, seed=0):
    """n_img images whose taken planes are distinct natural frames (encode_helpers.natural_frames)."""
    return pixel_array(EH.natural_frames(bigbridge, w, h, n_img * px.C, seed), px, seed + 2)


# ---- the seeded sweep -------------------------------------------------------------------------------------

SWEEP_SALT = 41
SWEEP_CASES = 14                # per entry: 42 in all
STRIDE_EXTRA = (0, 1, 2, 4)     # pixel stride = C + one of these, or 5, or 7


@dataclasses.dataclass(frozen=True)
class SweepCase:
    entry: str
    i: int
    W: int
    H: int
    n: int
    px: Pixels
    no_delta: bool
    init_zero: bool
    limit: bool
    ws_fill: Optional[int]

    @property
    def flags(self):
        return (EH.NO_DELTA if self.no_delta else 0) | (EH.LIMIT if self.limit else 0)

    @property
    def wide(self):
        return self.px.wide(self.W, self.H, self.n)


def sweep_case(entry, i):
    """Case i of `entry`: everything follows from (entry, i) alone. Small frames (1..40 x 1..6 blocks,
    W and H anywhere in the last block), 1..3 images, C in 1..4 in turn, every other case on an
    aligned layout of pixel stride 2, 3 or 4 in turn (the dword loads) and the rest anywhere."""
    e, i = ENTRIES.index(entry), int(i)
    r = np.random.default_rng([e, i, SWEEP_SALT])
    C = (i + e) % 4 + 1
    bw, bh = int(r.integers(1, 41)), int(r.integers(1, 7))
    W = 8 * bw - (0 if r.random() < 0.4 else int(r.integers(1, 8)))
    H = 8 * bh - int(r.integers(0, 8))
    n = int(r.integers(1, 4))
    aligned = i % 2 == 0
    if aligned:
        ps = max(C, (3, 4, 2, 4, 3, 2, 4)[i // 2 % 7])
        fc = int(r.integers(0, ps - C + 1))
        pitch_pad = (-W * ps) % 4 + 4 * int(r.integers(0, 4))
        delta = 4 * int(r.integers(0, 4))
        span = (H - 1) * (W * ps + pitch_pad) + W * ps
        gap = (-span) % 4 + 4 * int(r.integers(0, 9))
    else:
        ps = (C + STRIDE_EXTRA[int(r.integers(0, 4))], 5, 7)[int(r.integers(0, 3))]
        fc = int(r.integers(0, ps - C + 1))
        pitch_pad, delta, gap = int(r.integers(0, 12)), int(r.integers(0, 9)), int(r.integers(0, 40))
    px = Pixels(ps, fc, C, bool((i // 2 + e) % 2), delta, pitch_pad, gap)
    return SweepCase(entry, i, W, H, n, px, bool(r.random() < 0.25), bool(r.random() < 0.4), bool(r.random() < 0.3),
                     None if r.random() < 0.5 else int(r.integers(1, 256)))


def sweep_cases():
    return [sweep_case(entry, i) for entry in ENTRIES for i in range(SWEEP_CASES)]
