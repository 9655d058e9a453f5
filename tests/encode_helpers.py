"""A raw-ABI driver for the three GPU encode entries (test_gpu_encode_layouts.py,
test_gpu_encode_sweep.py, test_encode_sweep_cases.py): mh_encode_frame_device_async ("single"),
mh_encode_frames_device_async ("batch") and mh_encode_frames_shared_device_async ("shared_built",
"shared_supplied"), called through ctypes with the pixels at any byte offset and frame stride inside
a garbage-filled buffer and every output at a caller-chosen offset inside a guard-filled tensor.

The standard is the host codec (mh.encode_frame, pinned to the reference encoder by
test_codec_parity.py), frame by frame; never another GPU encode. Every call is made twice over one
workspace into fresh outputs, and every accepted case is decoded on the device back to its images.

The "single" entry encodes its n frames one call after the other over one workspace into the slots
of one set of outputs, so a neighbouring slot and a call after a rejected frame are checked too."""
from __future__ import annotations

import ctypes
import dataclasses
from typing import Optional

import numpy as np

from helpers import fibonacci_deltas, image_of_symbols

ENTRIES = ("single", "batch", "shared_built", "shared_supplied")
BATCHED = ENTRIES[1:]
SHARED = ENTRIES[2:]
OK, TOO_LONG, CAPACITY, TABLE = 0, -3, -4, -5
NO_DELTA, ZEROED, LIMIT = 0x1, 0x100, 0x200
GUARD = 256                     # guard bytes on both sides of every payload, at the least
# one fill per kind of output: code / init / header bytes, u32 offsets, u64 lengths and frame offsets, status words
FILL_BYTES, FILL_U32, FILL_U64, FILL_STATUS = 0xC3, 0x3C, 0xFF, 0x5A


def r4(v):
    return (int(v) + 3) // 4 * 4


def r16(v):
    return (int(v) + 15) // 16 * 16


def blocks(w, h):
    return -(-w // 8), -(-h // 8)


def roomy_slot(w, h):
    """test_gpu_encode_shared._run's slot: two bytes a symbol, the pad, a spare quad."""
    bw, bh = blocks(w, h)
    return r16(bw * bh * 64 * 2 + 4) + 16


@dataclasses.dataclass(frozen=True)
class Layout:
    """Where the pixels and the outputs sit. Frame f's pixels start at base + delta + f * stride
    (base 256-byte aligned; stride None = W * H); every output's payload starts `*_off` bytes past
    a 256-byte boundary, so the offset is the pointer's residue."""
    delta: int = 0
    stride: Optional[int] = None
    codes_off: int = 0          # a multiple of 4 (single) or 16 (batched)
    offs_off: int = 0           # a multiple of 4
    init_off: int = 0
    canon_off: int = 0
    len_off: int = 0            # a multiple of 8: d_codes_len, d_frame_code_offsets
    status_off: int = 0         # a multiple of 4: d_status, d_header_status


class _Out:
    """One output: `size` payload bytes at a chosen residue inside its own guard-filled tensor."""

    def __init__(self, device, size, off, fill):
        import torch
        self.t = torch.full((GUARD + 256 + off + size + GUARD,), fill, dtype=torch.uint8, device=device)
        p = self.t.data_ptr()
        self.start = (p + GUARD + 255) // 256 * 256 + off - p
        self.ptr, self.size, self.fill = p + self.start, size, fill
        assert self.start >= GUARD and self.t.numel() - self.start - size >= GUARD

    def view(self):
        return self.t[self.start: self.start + self.size]

    def host(self, what):
        a = self.t.cpu().numpy()
        lo, hi = a[:self.start], a[self.start + self.size:]
        assert (lo == self.fill).all(), f"{what}: {int((lo != self.fill).sum())} guard byte(s) in front written"
        assert (hi == self.fill).all(), (f"{what}: {int((hi != self.fill).sum())} guard byte(s) behind written, "
                                         f"first at payload end + {int(np.flatnonzero(hi != self.fill)[0])}")
        return a[self.start: self.start + self.size]


def gray_buffer(device, imgs, delta, stride, seed=1):
    """The frames inside one larger u8 tensor of seeded garbage -> (tensor, address of frame 0).
    Garbage in front of frame 0, between frames and for 8 W + 64 bytes and more behind the last;
    every read the kernels may make (the frames' own bytes) is inside the allocation."""
    import torch
    h, w = imgs[0].shape
    n = len(imgs)
    assert n == 1 or stride >= w * h
    size = 256 + delta + (n - 1) * stride + w * h + 8 * w + 64 + 256
    buf = np.random.default_rng([seed, w, h, n, delta, stride]).integers(0, 256, size, dtype=np.uint8)
    t = torch.empty(size, dtype=torch.uint8, device=device)
    base = (t.data_ptr() + 255) // 256 * 256 - t.data_ptr() + delta
    for f, im in enumerate(imgs):
        assert im.shape == (h, w) and im.dtype == np.uint8
        buf[base + f * stride: base + f * stride + w * h] = im.reshape(-1)
    t.copy_(torch.from_numpy(buf))
    return t, t.data_ptr() + base


@dataclasses.dataclass
class Run:
    entry: str
    n: int
    w: int
    h: int
    nb: int
    slot: int
    flags: int
    init_zero: bool
    rc: int
    host: dict                  # name -> the payload on the host (guards already checked)
    dev: dict                   # name -> _Out

    def codes(self, f):
        return self.host["codes"][f * self.slot: (f + 1) * self.slot]

    def offsets(self, f):
        return self.host["offs"].view(np.uint32)[f * self.nb: (f + 1) * self.nb]

    def init(self, f):
        return self.host["init"][f * self.nb: (f + 1) * self.nb]

    def header(self, f):
        return self.host["canon"][:256] if self.entry in SHARED else self.host["canon"][256 * f: 256 * f + 256]

    @property
    def codes_len(self):
        return self.host["lens"].view(np.uint64)

    @property
    def status(self):
        return self.host["st"].view(np.int32)


def workspace_bytes(mh, entry, w, h, n):
    L = mh.lib()
    if entry == "single":
        return int(L.mh_encode_workspace_bytes(w, h))
    if entry == "batch":
        return int(L.mh_encode_frames_workspace_bytes(w, h, n))
    return int(L.mh_encode_frames_shared_workspace_bytes(w, h, n))


def run(mh, device, entry, imgs, *, flags=0, init_zero=False, layout=Layout(), slot=None, header=None,
        ws_fill=None, cap=None, n_frames=None, told_stride=None, ws_bytes=None, launches=True):
    """Two rounds of calls over one workspace into fresh outputs -> [Run, Run].
    flags: MH_FLAG_NO_DELTA | MH_ENCODE_LIMIT_LENGTHS; MH_ENCODE_WORKSPACE_ZEROED is added when the
    workspace is zero-filled (ws_fill None), else the workspace is filled with the byte ws_fill.
    slot: codes_cap (single; a multiple of 4, also the distance of the frames' slots) or
    codes_frame_stride (batched; a multiple of 16). cap (single only): a codes_cap other than the
    slot's size, any byte count up to it. header: u8[256] for shared_supplied.
    n_frames / told_stride / ws_bytes: what the call is told, where that is not the truth (the
    refusals: the buffers are laid out for the truth, so a call that launched would stay inside them).
    launches False: the call must refuse before any launch; no second round."""
    import torch
    L = mh.lib()
    assert entry in ENTRIES and (header is not None) == (entry == "shared_supplied")
    n = len(imgs)
    h, w = imgs[0].shape
    bw, bh = blocks(w, h)
    nb = bw * bh
    told_n = n if n_frames is None else n_frames
    stride = w * h if layout.stride is None else layout.stride
    slot = roomy_slot(w, h) if slot is None else slot
    assert slot % (4 if entry == "single" else 16) == 0 and layout.codes_off % (4 if entry == "single" else 16) == 0
    assert layout.offs_off % 4 == 0 and layout.len_off % 8 == 0 and layout.status_off % 4 == 0
    wsb = workspace_bytes(mh, entry, w, h, max(n, told_n)) if ws_bytes is None else ws_bytes
    ws = torch.zeros(wsb + 256, dtype=torch.uint8, device=device)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    fl = flags | (ZEROED if ws_fill is None else 0)
    wsp = (ws.data_ptr() + 255) // 256 * 256
    gray_t, gray = gray_buffer(device, imgs, layout.delta, stride)
    cin = torch.from_numpy(np.ascontiguousarray(header, np.uint8)).to(device) if header is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    told = stride if told_stride is None else told_stride
    assert entry != "single" or (told == stride and told_n == n)
    assert cap is None or (entry == "single" and cap <= slot)
    runs = []
    for _ in range(2 if launches else 1):
        o = dict(codes=_Out(device, n * slot, layout.codes_off, FILL_BYTES),
                 offs=_Out(device, n * nb * 4, layout.offs_off, FILL_U32),
                 canon=_Out(device, 256 if entry in SHARED else 256 * n, layout.canon_off, FILL_BYTES),
                 lens=_Out(device, 8 * n, layout.len_off, FILL_U64),
                 st=_Out(device, 4 * n, layout.status_off, FILL_STATUS))
        if init_zero:
            o["init"] = _Out(device, n * nb, layout.init_off, FILL_BYTES)
        if entry in BATCHED:
            o["fco"] = _Out(device, 8 * (n + 1), layout.len_off, FILL_U64)
        if entry in SHARED:
            o["hst"] = _Out(device, 4, layout.status_off, FILL_STATUS)
        initp = o["init"].ptr if init_zero else None
        if entry == "single":
            rc = OK
            for f in range(n):
                rc = rc or L.mh_encode_frame_device_async(
                    gray + f * stride, w, h, fl, o["canon"].ptr + 256 * f, o["codes"].ptr + f * slot, slot if cap is None else cap,
                    o["lens"].ptr + 8 * f, o["offs"].ptr + 4 * nb * f, initp + nb * f if init_zero else None,
                    o["st"].ptr + 4 * f, wsp, wsb, stream)
        elif entry == "batch":
            rc = L.mh_encode_frames_device_async(
                gray, told, told_n, w, h, fl, o["canon"].ptr, o["codes"].ptr, slot, o["lens"].ptr, o["fco"].ptr,
                o["offs"].ptr, initp, o["st"].ptr, wsp, wsb, stream)
        else:
            rc = L.mh_encode_frames_shared_device_async(
                gray, told, told_n, w, h, fl, cin.data_ptr() if cin is not None else None, o["canon"].ptr,
                o["codes"].ptr, slot, o["lens"].ptr, o["fco"].ptr, o["offs"].ptr, initp, o["st"].ptr, o["hst"].ptr,
                wsp, wsb, stream)
        torch.cuda.synchronize(device)
        host = {k: v.host(f"{entry}: {k}") for k, v in o.items()}
        runs.append(Run(entry, n, w, h, nb, slot, flags, init_zero, int(rc), host, o))
    del gray_t
    return runs


@dataclasses.dataclass
class Expected:
    header: Optional[np.ndarray]     # the shared header (shared entries with an accepted header), else None
    header_status: int
    frames: list                     # (status, EncodedFrame or None) per frame


def expect(mh, entry, imgs, *, flags=0, init_zero=False, slot=None, header=None):
    """What the host codec says of every frame. flags as for run(); slot: the capacity."""
    from metalhuffman_amd import codec
    limit = bool(flags & LIMIT)
    fmt = flags & NO_DELTA
    h, w = imgs[0].shape
    slot = roomy_slot(w, h) if slot is None else slot
    hdr, hst = None, OK
    if entry in SHARED:
        if header is not None:
            hdr = np.ascontiguousarray(header, np.uint8)
        else:
            try:
                hdr = codec.shared_header(imgs, fmt, init_zero, limit_lengths=limit)
            except mh.MHError as e:
                hst = e.status
    out = []
    for im in imgs:
        if hst != OK:
            out.append((hst, None))
            continue
        try:
            ef = mh.encode_frame(im, flags=fmt, init_zero_delta=init_zero, limit_lengths=limit and hdr is None, header=hdr)
        except mh.MHError as e:
            out.append((e.status, None))
            continue
        out.append((CAPACITY, None) if r4(ef.codes.size) > slot else (OK, ef))
    return Expected(hdr, hst, out)


# What the runs of this process saw where the header leaves the outcome open (reported by
# test_gpu_encode_sweep.py; never asserted): the values of the bytes [codes_len, round_up(codes_len, 4))
# of accepted frames, and whether a rejected frame's d_block_init slice was written.
SEEN = {"pad bytes": set(), "rejected init": set()}


def _same(a, b, what):
    assert np.array_equal(a, b), f"the second round over the workspace differs in {what}"


def check(mh, runs, imgs, exp, rc=OK):
    """Both rounds against the host codec, frame by frame, and against each other."""
    for r in runs:
        assert r.rc == rc, (r.rc, rc)
        lens, st = r.codes_len, r.status
        if r.entry in SHARED:
            assert int(r.host["hst"].view(np.int32)[0]) == exp.header_status
            if exp.header_status == OK:
                assert np.array_equal(r.host["canon"], exp.header), "the shared header"
        if r.entry in BATCHED:
            assert np.array_equal(r.host["fco"].view(np.uint64), np.arange(r.n + 1, dtype=np.uint64) * np.uint64(r.slot))
        for f, (status, ef) in enumerate(exp.frames):
            assert int(st[f]) == status, (f, int(st[f]), status)
            if status != OK:
                assert int(lens[f]) == 0, f
                assert (r.codes(f) == FILL_BYTES).all(), f"rejected frame {f}: code bytes written"
                assert (r.offsets(f) == 0x3C3C3C3C).all(), f"rejected frame {f}: offsets written"
                if r.init_zero:
                    SEEN["rejected init"].add((r.entry, "written" if (r.init(f) != FILL_BYTES).any() else "untouched"))
                continue                # its d_block_init slice and its header: unspecified
            k = ef.codes.size
            assert int(lens[f]) == k, (f, int(lens[f]), k)
            assert np.array_equal(r.header(f), ef.canon), f
            got = r.codes(f)
            if not np.array_equal(got[:k], ef.codes):
                bad = np.flatnonzero(got[:k] != ef.codes)
                raise AssertionError(f"frame {f}: {bad.size} of {k} code bytes differ, first at {int(bad[0])}, "
                                     f"last at {int(bad[-1])}")
            SEEN["pad bytes"].update(int(v) for v in got[k: r4(k)])
            tail = got[r4(k):]
            assert (tail == FILL_BYTES).all(), (f"frame {f}: {int((tail != FILL_BYTES).sum())} byte(s) written "
                                               f"behind round_up(codes_len, 4) = {r4(k)} of a slot of {r.slot}")
            assert np.array_equal(r.offsets(f), ef.block_offsets), f
            if r.init_zero:
                assert np.array_equal(r.init(f), ef.block_init), f
    if len(runs) == 2:
        a, b = runs
        for k in ("offs", "lens", "st", "hst", "fco"):
            if k in a.host:
                _same(a.host[k], b.host[k], k)
        for f, (status, ef) in enumerate(exp.frames):
            if status == OK:
                _same(a.codes(f)[:ef.codes.size], b.codes(f)[:ef.codes.size], f"frame {f}'s codes")
                _same(a.header(f), b.header(f), f"frame {f}'s header")
                if a.init_zero:
                    _same(a.init(f), b.init(f), f"frame {f}'s init bytes")
            else:
                _same(a.codes(f), b.codes(f), f"rejected frame {f}'s slot")


def check_untouched(runs, rc):
    """A call refused before any launch: the return code, and every output as it was filled."""
    for r in runs:
        assert r.rc == rc, (r.rc, rc)
        for k, v in r.host.items():
            assert (v == r.dev[k].fill).all(), f"{r.entry}: {k} written by a refused call"


def round_trip(mh, device, r, imgs, exp):
    """The accepted frames of a round, decoded on the device from the encoder's own outputs:
    mh_build_luts_device + mh_decode_frames (a header per frame) or mh_build_tables_device +
    mh_decode (the shared header). The outputs go in as they are where every frame was accepted
    and the slots are 16-byte aligned; else the accepted slots are copied to an aligned tensor."""
    import torch
    from metalhuffman_amd import decoder as D
    acc = [f for f, (s, _) in enumerate(exp.frames) if s == OK]
    if not acc:
        return
    o = r.dev
    codes, offs = o["codes"].view(), o["offs"].view().view(torch.int32)
    init = o["init"].view() if r.init_zero else None
    direct = len(acc) == r.n and o["codes"].ptr % 16 == 0 and r.slot % 16 == 0
    if direct:
        fco = o["fco"].view().view(torch.int64) if "fco" in o else \
            torch.arange(r.n + 1, dtype=torch.int64, device=device) * r.slot
        fr = D.DeviceFrames(r.w, r.h, r.n, offs, codes, fco if r.n > 1 else None, init, r.flags & NO_DELTA)
    else:
        sizes = [r16(int(r.codes_len[f])) for f in acc]
        starts = np.concatenate([[0], np.cumsum(sizes)])
        packed = torch.zeros(int(starts[-1]), dtype=torch.uint8, device=device)
        for s, f in zip(starts, acc):
            k = int(r.codes_len[f])
            packed[int(s): int(s) + k] = codes[f * r.slot: f * r.slot + k]
        sel = torch.tensor(acc, device=device)
        fr = D.DeviceFrames(r.w, r.h, len(acc), offs.view(r.n, r.nb)[sel].reshape(-1).contiguous(), packed,
                            torch.from_numpy(starts.astype(np.int64)).to(device) if len(acc) > 1 else None,
                            init.view(r.n, r.nb)[sel].reshape(-1).contiguous() if init is not None else None,
                            r.flags & NO_DELTA)
    canon = o["canon"].view()
    if r.entry in SHARED:
        tabs = D.DeviceTables.from_canonical_header(canon.clone(), device)
        out = D.decode(fr, tabs)
        assert tabs.check_status() >= 0
    else:
        ts = D.DeviceTableSet.from_canonical_headers(canon.view(r.n, 256)[torch.tensor(acc, device=device)], device)
        out = D.decode_frames(fr, ts)
        ts.check_status()
    torch.cuda.synchronize(device)
    got = out.cpu().numpy()
    for p, f in enumerate(acc):
        assert np.array_equal(got[p, :, :r.w], imgs[f]), f"frame {f} does not decode to its image"


def run_checked(mh, device, entry, imgs, *, flags=0, init_zero=False, layout=Layout(), slot=None, header=None,
                ws_fill=None, cap=None):
    """run + expect + check + round_trip -> (the second round, the expectation)."""
    runs = run(mh, device, entry, imgs, flags=flags, init_zero=init_zero, layout=layout, slot=slot, header=header,
               ws_fill=ws_fill, cap=cap)
    exp = expect(mh, entry, imgs, flags=flags, init_zero=init_zero, slot=runs[0].slot if cap is None else cap,
                 header=header)
    check(mh, runs, imgs, exp)
    round_trip(mh, device, runs[1], imgs, exp)
    return runs[1], exp


def natural_frames(bigbridge, w, h, n, seed=0):
    """n distinct frames of natural histograms: crops of the picture tiled over the plane, every
    other one with its 8x8 blocks shuffled (the same histogram of deltas, another order of blocks)."""
    from metalhuffman_amd import frames as F
    bw, bh = blocks(w, h)
    r = np.random.default_rng([seed, w, h, n, 7])
    out = []
    for f in range(n):
        y, x = int(r.integers(0, bigbridge.shape[0])), int(r.integers(0, bigbridge.shape[1]))
        rows, cols = (y + np.arange(8 * bh)) % bigbridge.shape[0], (x + np.arange(8 * bw)) % bigbridge.shape[1]
        im = np.ascontiguousarray(bigbridge[np.ix_(rows, cols)])      # a crop of np.tile(bigbridge, ...)
        if f % 2:
            im = F.block_shuffle(im, seed + f)
        out.append(np.ascontiguousarray(im[:h, :w]))
    return out


def accepted_frames(mh, entry, bigbridge, w, h, n, seed=0):
    """natural_frames that the host codec accepts under the entry's table (now and then the tree of
    a natural histogram is deeper than 16): the first of the seeds seed, seed + 100, ... that does."""
    for k in range(8):
        imgs = natural_frames(bigbridge, w, h, n, seed + 100 * k)
        header = supplied_header(imgs) if entry == "shared_supplied" else None
        if all(s == OK for s, _ in expect(mh, entry, imgs, header=header).frames):
            return imgs
    raise AssertionError(f"no accepted frames of {w} x {h} for {entry} among eight seeds")


def supplied_header(imgs, flags=0, init_zero=False):
    """The header the shared_supplied cases bring: the host's for the batch (length-limited where
    the batch's tree is deeper than 16, so it is always a usable code)."""
    from metalhuffman_amd import codec
    return codec.shared_header(imgs, flags & NO_DELTA, init_zero, limit_lengths=True)


# ---- the seeded sweep -------------------------------------------------------------------------------------

BW_PICKS = (1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 199, 200)
SWEEP_SALT = 23
SWEEP_DEFAULT_CASES = 48
DEEP_SYMBOLS = 19               # helpers.fibonacci_deltas(19, ...): a tree 18 deep
DEEP_MIN_BLOCKS = 172           # 10,945 symbols hold one whole Fibonacci histogram of 19 symbols
PAD_KINDS = ("none", "8", "odd", "large")
FITS = ("roomy", "exact", "tight")


@dataclasses.dataclass(frozen=True)
class SweepCase:
    entry: str
    i: int
    bw: int
    bh: int
    W: int
    H: int
    n: int
    pad_kind: str
    layout: Layout
    no_delta: bool
    init_zero: bool
    limit: bool
    ws_fill: Optional[int]       # None: a zero-filled workspace and MH_ENCODE_WORKSPACE_ZEROED
    fit: str                     # the slot: roomy, exactly the largest frame, or the largest frame left out
    deep: Optional[int]          # the frame whose tree is deeper than 16, or None

    @property
    def flags(self):
        return (NO_DELTA if self.no_delta else 0) | (LIMIT if self.limit else 0)

    @property
    def stride(self):
        return self.layout.stride

    def vec(self, f=0):
        """Whether frame f goes through the 8-byte loads (the host switch of mh_encode.hip)."""
        if self.W % 8:
            return False
        if self.entry == "single":
            return (self.layout.delta + f * self.stride) % 8 == 0
        return self.layout.delta % 8 == 0 and self.stride % 8 == 0

    def pair(self):
        return self.entry != "single" and self.vec() and self.bw % 2 == 0

    def describe(self):
        return (f"sweep_case({self.entry!r}, {self.i}): {self.bw} x {self.bh} blocks, {self.W} x {self.H}, n {self.n}, "
                f"pad {self.pad_kind}, {self.layout}, no_delta {self.no_delta}, init {self.init_zero}, limit "
                f"{self.limit}, ws_fill {self.ws_fill}, fit {self.fit}, deep {self.deep}")


def sweep_case(entry, i):
    """Case i of `entry`: everything follows from (entry, i) alone."""
    e, i = ENTRIES.index(entry), int(i)
    r = np.random.default_rng([e, i, SWEEP_SALT])
    # every other case walks the width thresholds in turn; the rest are uniform
    bw = BW_PICKS[(i // 2 + 3 * e) % len(BW_PICKS)] if i % 2 == 0 else int(r.integers(1, 201))
    bh = int(r.integers(1, 25))
    W = 8 * bw - (0 if r.random() < 0.6 else int(r.integers(1, 8)))
    H = 8 * bh - int(r.integers(0, 8))
    n = int(r.integers(1, 6))
    u = r.random()
    delta = 0 if u < 0.4 else 8 if u < 0.6 else int(r.integers(1, 16))
    pad_kind = PAD_KINDS[int(r.integers(0, 4))]
    pad = {"none": 0, "8": 8, "odd": 2 * int(r.integers(0, 20)) + 1,
           "large": 4112 if r.random() < 0.5 else 4096 + int(r.integers(0, 64))}[pad_kind]
    no_delta, init_zero = bool(r.random() < 0.25), bool(r.random() < 0.4)
    limit = bool(r.random() < 0.4)
    ws_fill = None if r.random() < 0.5 else int(r.integers(1, 256))
    fit = FITS[int(r.choice(3, p=[0.5, 0.3, 0.2]))]
    deep = None
    if r.random() < 1 / 6:
        deep = int(r.integers(0, n))
        if bw * bh < DEEP_MIN_BLOCKS:
            bw = max(bw, 8)
            bh = max(bh, -(-DEEP_MIN_BLOCKS // bw))
        W, H = 8 * bw, 8 * bh    # image_of_symbols: whole blocks
    g = 4 if entry == "single" else 16
    lay = Layout(delta=delta, stride=W * H + pad, codes_off=g * int(r.integers(0, 16)),
                 offs_off=4 * int(r.integers(0, 5)), init_off=int(r.integers(0, 16)), canon_off=int(r.integers(0, 16)),
                 len_off=8 * int(r.integers(0, 3)), status_off=4 * int(r.integers(0, 3)))
    return SweepCase(entry, i, bw, bh, W, H, n, pad_kind, lay, no_delta, init_zero, limit, ws_fill, fit, deep)


def sweep_images(case, bigbridge):
    imgs = natural_frames(bigbridge, case.W, case.H, case.n, seed=1000 * ENTRIES.index(case.entry) + case.i)
    if case.deep is not None:
        d = fibonacci_deltas(DEEP_SYMBOLS, case.bw * case.bh * 64, seed=case.i)
        # every block starts with symbol 0 (swapped in from inside the block), so the init-byte format,
        # which takes each block's first delta out of the histogram, keeps the tree as deep
        b = d.reshape(-1, 64)
        for k in np.flatnonzero(b[:, 0]):
            j = np.flatnonzero(b[k] == 0)
            if j.size:
                b[k, 0], b[k, j[0]] = 0, b[k, 0]
        imgs[case.deep] = image_of_symbols(d, case.W, case.H, no_delta=case.no_delta)
    return imgs


def sweep_plan(mh, case, bigbridge):
    """-> (images, header or None, slot, Expected): the slot from the host's code lengths (exact:
    the largest accepted frame fits to the word; tight: the largest is left out)."""
    imgs = sweep_images(case, bigbridge)
    header = supplied_header(imgs, case.flags, case.init_zero) if case.entry == "shared_supplied" else None
    kw = dict(flags=case.flags, init_zero=case.init_zero, header=header)
    roomy = expect(mh, case.entry, imgs, **kw)
    g = 4 if case.entry == "single" else 16
    sizes = sorted({-(-r4(ef.codes.size) // g) * g for s, ef in roomy.frames if s == OK})
    if case.fit == "roomy" or not sizes:
        return imgs, header, roomy_slot(case.W, case.H), roomy
    slot = sizes[-1] if case.fit == "exact" else sizes[-2] if len(sizes) > 1 else max(g, sizes[-1] - g)
    return imgs, header, slot, expect(mh, case.entry, imgs, slot=slot, **kw)


def run_sweep_case(mh, device, case, bigbridge):
    imgs, header, slot, exp = sweep_plan(mh, case, bigbridge)
    runs = run(mh, device, case.entry, imgs, flags=case.flags, init_zero=case.init_zero, layout=case.layout, slot=slot,
               header=header, ws_fill=case.ws_fill)
    try:
        check(mh, runs, imgs, exp)
        round_trip(mh, device, runs[1], imgs, exp)
    except AssertionError as err:
        raise AssertionError(f"{case.describe()}: {err}") from err


def sweep_range():
    """(first, count) of the default sweep, or of another one asked for through the environment."""
    import os
    return int(os.environ.get("MH_ENCODE_SWEEP_FIRST", "0")), int(os.environ.get("MH_ENCODE_SWEEP_CASES",
                                                                                 str(SWEEP_DEFAULT_CASES)))


# ---- shapes on the kernels' thresholds (test_gpu_encode_layouts.py; asserted in test_encode_sweep_cases.py) ----

# Constants of mh_encode.hip: kStepBlocks = 16 (blocks per packer step; below it the batched
# packer's row loader divides), group_row's 32 (the four-kernel split), kCodeTile = 128 and
# kBatchTile = 256 (blocks per tile, fused and batched; tile_rows wraps once from there on),
# kPackWaves = 4 (tiles per packer workgroup), kReduceTiles = 96 (tiles per reduction workgroup,
# shared built mode), kFusedMaxTiles = 512 (the largest fused frame).
K_STEP_BLOCKS, K_CODE_TILE, K_BATCH_TILE, K_PACK_WAVES, K_REDUCE_TILES, K_FUSED_MAX_TILES = 16, 128, 256, 4, 96, 512
THRESHOLD_WIDTHS = (1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257)


def tile_blocks(entry):
    return K_CODE_TILE if entry == "single" else K_BATCH_TILE


def threshold_targets(entry):
    """Block counts to land on: one packer step, one tile, one packer workgroup of tiles."""
    t = tile_blocks(entry)
    return (K_STEP_BLOCKS, t, K_PACK_WAVES * t)


def threshold_heights(entry, bw):
    """Heights in blocks at which bw x bh lands on each target, or just below and just above it
    (the two nearest counts a frame of that width has), sorted."""
    out = set()
    for t in threshold_targets(entry):
        lo = t // bw
        out.update(b for b in ((lo - 1, lo, lo + 1) if t % bw == 0 else (lo, lo + 1)) if b >= 1)
    return sorted(out)


def threshold_shapes(entry, bw):
    """[(W, H)]: per height, a width ending on the block and one 1 pixel into the last block; the
    pixel height ends on the block for even heights in blocks and 3 rows into it for odd ones."""
    return [(8 * bw - d, 8 * bh - (5 if bh % 2 else 0)) for bh in threshold_heights(entry, bw) for d in (0, 7)]
