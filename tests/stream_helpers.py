"""A raw-ABI driver for the two stream front ends (test_gpu_stream_layouts.py, test_gpu_stream_sweep.py,
test_stream_sweep_cases.py): mh_stream_create / mh_stream_submit ("table": one table pair fixed at
creation), mh_stream_create_headers / mh_stream_submit_header ("headers": a canonical header per
frame) and mh_stream_group_* (table mode, members on a list of devices), called through ctypes so
that every argument is reached: host buffers in slot layout or apart, pinned or pageable, caller
rasters at byte offset 8 inside pattern-filled tensors or the stream's own, graph replays or direct
launches, with or without a prepared table, any submit order, any told code length.

Every submit gets host buffers of its own, kept untouched until the stream is synchronised, and is
followed by a consumer: a device-to-device copy of the slot's raster into the submission's private
result tensor, queued on mh_stream_slot_stream(slot). So every frame of a back-to-back run is
checked with no host wait between the submits.

The standard for a result is a direct mh_decode (mh_decode_headers) call over the frame's own
bytes and the same tables, over all round_up(W, 8) x H bytes; then the source image in the columns
< W, and the oracle's shader decode for chosen frames. A rejected header must leave what the slot's
raster held, byte for byte; the driver follows every slot's expected content from creation on."""
from __future__ import annotations

import contextlib
import ctypes
import dataclasses
import os
from typing import Optional

import numpy as np

MODES = ("table", "headers")
FORMATS = ("delta", "no_delta", "init")
OK, INVALID, TOO_LONG, CAPACITY, TABLE = 0, -1, -3, -4, -5
NO_DELTA = 0x1
CODES_PAD = 4
GUARD = 256                     # guard bytes on both sides of a caller's raster, at the least
RASTER_OFF = 8                  # a caller's raster starts 8 bytes past a 256-byte boundary: the weakest legal alignment
RESULT_FILL, REF_FILL = 0xEE, 0x5A
ENV = "MH_STREAM_GRAPHS"
KINDS = ("noise", "flat", "ramp", "walk", "sparse", "mid")


def r8(v):
    return (int(v) + 7) // 8 * 8


def r16(v):
    return (int(v) + 15) // 16 * 16


def n_blocks(w, h):
    return -(-w // 8) * -(-h // 8)


# ---- frame sets ----------------------------------------------------------------------------------

def image(kind, w, h, seed):
    """One u8 [h, w] image. noise: uniform bytes (dense bits under any header); flat: one value with
    at most three other pixels (the shortest frame); ramp, walk, sparse, mid: lengths in between."""
    r = np.random.default_rng([seed, w, h, KINDS.index(kind)])
    if kind == "noise":
        return r.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "flat":
        im = np.full((h, w), int(r.integers(0, 256)), np.uint8)
        for _ in range(int(r.integers(0, 4))):
            im[int(r.integers(0, h)), int(r.integers(0, w))] = int(r.integers(0, 256))
        return im
    if kind == "ramp":
        y, x = np.mgrid[0:h, 0:w]
        return ((3 * x + 5 * y + int(r.integers(0, 256))) & 0xFF).astype(np.uint8)
    if kind == "walk":
        return (np.cumsum(r.integers(-2, 3, (h, w)), axis=1) + r.integers(0, 256, (h, 1)) & 0xFF).astype(np.uint8)
    if kind == "sparse":
        return np.where(r.random((h, w)) < 0.1, r.integers(0, 256, (h, w)), 0).astype(np.uint8)
    return r.integers(0, 16, (h, w), dtype=np.uint8)


@dataclasses.dataclass
class FrameSet:
    mode: str
    fmt: str
    w: int
    h: int
    imgs: list
    efs: list                   # table mode: all under efs[0].canon

    @property
    def flags(self):
        return NO_DELTA if self.fmt == "no_delta" else 0

    @property
    def init(self):
        return self.fmt == "init"

    @property
    def sizes(self):
        return [int(ef.codes.size) for ef in self.efs]


def frame_set(mh, mode, w, h, n, fmt="delta", seed=0, kinds=KINDS):
    """n frames of w x h, frame f of kind kinds[f % len(kinds)] (frame 0 dense noise, frame 1 near
    constant). table: different code lengths under ONE header, codec.shared_header(...,
    limit_lengths=True) of them all; headers: a header each, limit_lengths=True, so no frame is
    ever rejected for depth."""
    from metalhuffman_amd import codec
    assert mode in MODES and fmt in FORMATS
    flags, init = (NO_DELTA if fmt == "no_delta" else 0), fmt == "init"
    imgs = [image(kinds[f % len(kinds)], w, h, seed + 17 * f) for f in range(n)]
    if mode == "table":
        hdr = codec.shared_header(imgs, flags, init, limit_lengths=True)
        efs = [mh.encode_frame(im, flags=flags, init_zero_delta=init, header=hdr) for im in imgs]
    else:
        efs = [mh.encode_frame(im, flags=flags, init_zero_delta=init, limit_lengths=True) for im in imgs]
    return FrameSet(mode, fmt, w, h, imgs, efs)


def slot_order(sizes, slots):
    """A submit order in which every slot takes its longest frame first and its shortest next: the
    `slots` longest frames (longest into slot 0), then the `slots` shortest of the others (shortest
    into slot 0), then the rest. Each frame once."""
    by = sorted(range(len(sizes)), key=lambda i: (-sizes[i], i))
    first, others = by[:slots], by[slots:]
    second = others[::-1][:slots]
    return first + second + [i for i in others if i not in second]


def second_under_half(sizes, order, slots):
    """Whether some slot's second frame is under half its first frame's length."""
    return any(2 * sizes[order[k + slots]] < sizes[order[k]] for k in range(min(slots, len(order) - slots)))


# ---- the driver ----------------------------------------------------------------------------------

@contextlib.contextmanager
def graphs_env(graphs):
    """MH_STREAM_GRAPHS for the creates inside: None = not set (each mode's default), True / False =
    1 / 0, "env" = whatever the environment holds (a test's monkeypatch.setenv)."""
    if graphs == "env":
        yield
        return
    old = os.environ.pop(ENV, None)
    if graphs is not None:
        os.environ[ENV] = "1" if graphs else "0"
    try:
        yield
    finally:
        os.environ.pop(ENV, None)
        if old is not None:
            os.environ[ENV] = old


def _pattern(n, salt):
    return ((np.arange(n, dtype=np.uint64) * 167 + 13 + 29 * salt) & 0xFF).astype(np.uint8)


class _Raster:
    """A caller's raster: `size` bytes RASTER_OFF past a 256-byte boundary inside its own tensor,
    every byte of which starts as a position-dependent pattern."""

    def __init__(self, device, size, salt):
        import torch
        total = GUARD + 256 + RASTER_OFF + size + GUARD
        self.t = torch.empty(total, dtype=torch.uint8, device=device)
        p = self.t.data_ptr()
        self.start = (p + GUARD + 255) // 256 * 256 + RASTER_OFF - p
        self.size, self.ptr = size, p + self.start
        self.pattern = _pattern(total, salt)
        self.t.copy_(torch.from_numpy(self.pattern))
        assert self.ptr % 256 == RASTER_OFF and self.start >= GUARD and total - self.start - size >= GUARD

    def view(self):
        return self.t[self.start: self.start + self.size]

    def host(self, what):
        """The payload, after asserting that every guard byte still holds the pattern."""
        a = self.t.cpu().numpy()
        inside = np.zeros(a.size, bool)
        inside[self.start: self.start + self.size] = True
        bad = np.flatnonzero((a != self.pattern) & ~inside)
        assert bad.size == 0, (f"{what}: {bad.size} guard byte(s) written, first at raster{int(bad[0]) - self.start:+d}, "
                               f"last at raster{int(bad[-1]) - self.start:+d} (the raster has {self.size} bytes)")
        return a[self.start: self.start + self.size].copy()


@dataclasses.dataclass
class _Sub:
    k: int
    frame: int
    header: Optional[bytes]     # the header that was submitted in the frame's place, or None
    member: int
    slot: int
    result: object              # u8[out_bytes] on the device: the consumer's copy


class Driver:
    """One stream (members None) or one group (members: a list of device ordinals; table mode, the
    group's own rasters) over a FrameSet.
    packed: the host parts of a submit lie in slot layout (one copy), else apart and in another order
    (one copy per part); init bytes always have a buffer of their own. pinned: host memory pinned or
    pageable.
    owned: the stream's own rasters (mh_stream_output) or caller rasters in guarded tensors.
    prepared: table mode with d_lut or with d_lut == NULL. graphs: see graphs_env. cap: codes_capacity
    (default: the longest frame). reserve: result tensors made ready before the first submit."""

    def __init__(self, mh, device, fs, *, slots, packed=True, pinned=True, owned=False, prepared=True, graphs=None,
                 cap=None, members=None, consume=True, reserve=None):
        import torch
        from metalhuffman_amd import _native as N
        from metalhuffman_amd import decoder as D
        from metalhuffman_amd.stream import _device_view
        self.mh, self.N, self.L, self.device, self.fs = mh, N, mh.lib(), device, fs
        self.slots, self.packed, self.pinned, self.consume = slots, packed, pinned, consume
        self.headers = fs.mode == "headers"
        self.group = members is not None
        assert not (self.group and self.headers), "groups are table mode only"
        self.owned = owned or self.group
        self.w, self.h = fs.w, fs.h
        self.nb, self.pitch = n_blocks(fs.w, fs.h), r8(fs.w)
        self.off_bytes, self.out_bytes = r16(4 * self.nb), self.pitch * fs.h
        self.cap = max(fs.sizes) if cap is None else cap
        n_members = len(members) if self.group else 1
        self.n_members = n_members
        self.tables = []
        if not self.headers:
            t1, t2 = fs.efs[0].tables()
            assert all((ef.canon == fs.efs[0].canon).all() for ef in fs.efs), "table mode: one header"
            self.tables = [D.DeviceTables.upload(t1, t2, device, prepare_lut=prepared) for _ in range(n_members)]
        self._init_dummy = torch.zeros(8, dtype=torch.uint8, device=device) if fs.init else None
        self.rasters = None if self.owned else [_Raster(device, self.out_bytes, s) for s in range(slots)]
        reserve = max(16, 4 * slots * n_members + 1) if reserve is None else reserve
        self._pool = torch.full((reserve, self.out_bytes), RESULT_FILL, dtype=torch.uint8, device=device)
        torch.cuda.synchronize(device)      # patterns, tables and fills are in place before any slot stream runs
        protos = (N.mh_frame * n_members)()
        for m in range(n_members):
            p = protos[m]
            if self.tables:
                t = self.tables[m]
                p.d_table1, p.d_table2, p.table2_entries = t.table1.data_ptr(), t.table2.data_ptr(), t.table2_entries
                p.d_lut = t.lut.data_ptr() if t.lut is not None else None
                assert (t.lut is not None) == prepared
            p.d_block_init = self._init_dummy.data_ptr() if fs.init else None
            p.dims = N.mh_dims(fs.w, fs.h, -(-fs.w // 8), -(-fs.h // 8))
            p.n_frames, p.flags = 1, fs.flags
        outs = None if self.owned else (ctypes.c_void_p * slots)(*[r.ptr for r in self.rasters])
        self._g = ctypes.c_void_p()
        h = ctypes.c_void_p()
        with graphs_env(graphs), torch.cuda.device(device):
            if self.group:
                devs = (ctypes.c_int * n_members)(*members)
                rc = self.L.mh_stream_group_create(protos, n_members, devs, self.cap, slots, ctypes.byref(self._g))
                assert rc == OK, f"mh_stream_group_create: {rc}"
                assert self.L.mh_stream_group_size(self._g) == n_members
                self.handles = [self.L.mh_stream_group_member(self._g, m) for m in range(n_members)]
            else:
                create = self.L.mh_stream_create_headers if self.headers else self.L.mh_stream_create
                rc = create(ctypes.byref(protos[0]), self.cap, slots, outs, ctypes.byref(h))
                assert rc == OK, f"{'mh_stream_create_headers' if self.headers else 'mh_stream_create'}: {rc}"
                self.handles = [h.value]
        assert all(self.handles)
        self.closed = False
        torch.cuda.synchronize(device)
        # every raster as creation left it: the content a rejected first frame must keep
        self.views, self.cur = {}, {}
        for m in range(n_members):
            for s in range(slots):
                if self.owned:
                    pitch = ctypes.c_size_t(0)
                    ptr = self.L.mh_stream_output(self.handles[m], s, ctypes.byref(pitch))
                    assert ptr and pitch.value == self.pitch, (ptr, pitch.value, self.pitch)
                    self.views[m, s] = _device_view(ptr, (self.out_bytes,), device)
                    self.cur[m, s] = self.views[m, s].cpu().numpy().copy()
                else:
                    r = self.rasters[s]
                    assert self.L.mh_stream_output(self.handles[m], s, None) == r.ptr
                    self.views[m, s] = r.view()
                    self.cur[m, s] = r.host(f"after creation, slot {s}")
                    if self.headers:    # header mode stores nothing; table mode's warm-up stores inside the raster only
                        assert np.array_equal(self.cur[m, s], r.pattern[r.start: r.start + r.size]), \
                            f"header-mode creation wrote slot {s}'s raster"
        self._streams, self._keep, self.subs, self._refs, self.last = {}, [], [], {}, {}
        self.accepted = 0

    # -- host staging --

    def _host(self, n):
        import torch
        t = torch.zeros(max(n, 1), dtype=torch.uint8)
        if self.pinned:
            t = t.pin_memory()
        assert t.is_pinned() == self.pinned and t.data_ptr() % 16 == 0
        self._keep.append(t)
        return t

    def _stage(self, ef, codes, header):
        """-> (header ptr or None, offsets ptr, codes ptr, init ptr or None) of fresh host buffers."""
        offs = np.ascontiguousarray(ef.block_offsets, np.uint32).view(np.uint8)
        assert offs.size == 4 * self.nb
        parts = ([np.frombuffer(header, np.uint8)] if self.headers else []) + [offs, codes]
        if self.packed:
            starts = ([0, 256, 256 + self.off_bytes] if self.headers else [0, self.off_bytes])
            buf = self._host(starts[-1] + codes.size)
            for s, p in zip(starts, parts):
                buf.numpy()[s: s + p.size] = p
            ptrs = [buf.data_ptr() + s for s in starts]
        else:
            # apart, and in the opposite order of the slot layout (codes, offsets, header), 64 bytes and
            # more between them: the library cannot take the parts for one buffer in slot layout
            starts, at = [], 0
            for p in parts[::-1]:
                starts.append(at)
                at += (p.size + 63) // 64 * 64 + 64
            buf = self._host(at)
            for s, p in zip(starts, parts[::-1]):
                buf.numpy()[s: s + p.size] = p
            ptrs = [buf.data_ptr() + s for s in starts][::-1]
            o, c = ptrs[-2], ptrs[-1]
            lies_packed = c == o + self.off_bytes and (not self.headers or o == ptrs[0] + 256)
            assert not lies_packed, "separate buffers happen to lie in slot layout"
        ip = None
        if self.fs.init:
            b = self._host(self.nb)
            b.numpy()[:self.nb] = ef.block_init
            ip = b.data_ptr()
        return ([None] + ptrs if not self.headers else ptrs) + [ip]

    # -- calls --

    def _slot_stream(self, m, s):
        import torch
        if (m, s) not in self._streams:
            ptr = self.L.mh_stream_slot_stream(self.handles[m], s)
            assert ptr
            self._streams[m, s] = torch.cuda.ExternalStream(ptr, device=self.device)
        return self._streams[m, s]

    def submit(self, i, *, header=None, codes_bytes=None, extend=None, expect=OK, wait=False):
        """Frame i from fresh host buffers, then the consumer's copy on the slot's stream.
        header: 256 bytes submitted in the place of the frame's own (header mode). extend: the code
        bytes zero-extended to that many. codes_bytes: what the call is told (default: all staged).
        expect: the return code; a refused submit must leave *slot alone and the rotation where it was.
        wait: mh_stream_wait on the slot before returning. -> (member, slot) or None."""
        import torch
        ef = self.fs.efs[i]
        codes = np.ascontiguousarray(ef.codes, np.uint8)
        if extend is not None:
            assert extend >= codes.size
            codes = np.concatenate([codes, np.zeros(extend - codes.size, np.uint8)])
        told = codes.size if codes_bytes is None else codes_bytes
        hdr = None
        if self.headers:
            hdr = bytes(header) if header is not None else np.ascontiguousarray(ef.canon, np.uint8).tobytes()
            assert len(hdr) == 256
        hp, op, cp, ip = self._stage(ef, codes, hdr)
        member, slot = ctypes.c_uint32(0xABCD), ctypes.c_uint32(0xABCD)
        if self.group:
            rc = self.L.mh_stream_group_submit(self._g, cp, told, op, ip, ctypes.byref(member), ctypes.byref(slot))
        elif self.headers:
            rc = self.L.mh_stream_submit_header(self.handles[0], hp, cp, told, op, ip, ctypes.byref(slot))
        else:
            rc = self.L.mh_stream_submit(self.handles[0], cp, told, op, ip, ctypes.byref(slot))
        assert rc == expect, f"submit {len(self.subs)} (frame {i}, {told} bytes told): returned {rc}, expected {expect}"
        if rc != OK:
            assert slot.value == 0xABCD and member.value == 0xABCD, "a refused submit wrote *slot"
            return None
        k = self.accepted
        self.accepted += 1
        want = (k % self.n_members, (k // self.n_members) % self.slots)
        got = (member.value if self.group else 0, slot.value)
        assert got == want, f"submit {k}: (member, slot) {got}, expected {want}"
        m, s = got
        assert k < self._pool.shape[0], "reserve more result tensors"
        res = self._pool[k]
        if self.consume:
            with torch.cuda.stream(self._slot_stream(m, s)):
                res.copy_(self.views[m, s], non_blocking=True)
        self.subs.append(_Sub(k, i, None if header is None else hdr, m, s, res))
        self.last[m, s] = self.subs[-1]
        if wait:
            assert self.L.mh_stream_wait(self.handles[m], s) == OK
            if self.headers and header is None:
                assert self.status(s) == OK, f"submit {k}: slot {s}'s status is {self.status(s)}"
        return got

    def run(self, order, wait=False):
        for i in order:
            self.submit(i, wait=wait)

    def status(self, slot):
        st = ctypes.c_int32(77)
        assert self.L.mh_stream_slot_status(self.handles[0], slot, ctypes.byref(st)) == OK
        return int(st.value)

    def sync(self):
        import torch
        rc = self.L.mh_stream_group_synchronize(self._g) if self.group else self.L.mh_stream_synchronize(self.handles[0])
        assert rc == OK, rc
        torch.cuda.synchronize(self.device)

    def close(self):
        """mh_stream_destroy (it waits for what is in flight) must return MH_OK."""
        import torch
        if not self.closed:
            self.closed = True
            self.views = {k: (None if self.owned else v) for k, v in self.views.items()}
            rc = self.L.mh_stream_group_destroy(self._g) if self.group else self.L.mh_stream_destroy(self.handles[0])
            assert rc == OK, f"destroy returned {rc}"
            torch.cuda.synchronize(self.device)

    # -- the standard --

    def reference(self, i, header=None):
        """(raster u8[H, pitch], verdict): a direct mh_decode / mh_decode_headers call over frame i's
        own bytes (codes_bytes = its own length) and the stream's tables, into a REF_FILL-filled raster."""
        import torch
        key = (i, header)
        if key in self._refs:
            return self._refs[key]
        N, fs, ef, dev = self.N, self.fs, self.fs.efs[i], self.device
        codes = torch.from_numpy(np.ascontiguousarray(ef.codes, np.uint8)).to(dev)
        offs = torch.from_numpy(np.ascontiguousarray(ef.block_offsets, np.uint32).view(np.int32)).to(dev)
        init = torch.from_numpy(np.ascontiguousarray(ef.block_init, np.uint8)).to(dev) if fs.init else None
        out = torch.full((self.out_bytes,), REF_FILL, dtype=torch.uint8, device=dev)
        fr = N.mh_frame()
        fr.d_block_offsets, fr.d_codes, fr.codes_bytes = offs.data_ptr(), codes.data_ptr(), codes.numel()
        fr.d_block_init = init.data_ptr() if init is not None else None
        fr.dims = N.mh_dims(fs.w, fs.h, -(-fs.w // 8), -(-fs.h // 8))
        fr.n_frames, fr.flags = 1, fs.flags
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        verdict = OK
        if self.headers:
            hd = torch.from_numpy(np.frombuffer(ef.canon.tobytes() if header is None else header, np.uint8).copy()).to(dev)
            st = torch.full((1,), 77, dtype=torch.int32, device=dev)
            rc = self.L.mh_decode_headers(ctypes.byref(fr), hd.data_ptr(), None, st.data_ptr(), out.data_ptr(), self.pitch,
                                          self.out_bytes, stream)
        else:
            t = self.tables[0]
            fr.d_table1, fr.d_table2, fr.table2_entries = t.table1.data_ptr(), t.table2.data_ptr(), t.table2_entries
            fr.d_lut = t.lut.data_ptr() if t.lut is not None else None
            rc = self.L.mh_decode(ctypes.byref(fr), out.data_ptr(), self.pitch, self.out_bytes, stream)
        assert rc == OK, f"the reference decode of frame {i}: {rc}"
        torch.cuda.synchronize(dev)
        if self.headers:
            verdict = int(st.cpu()[0])
        ras = out.cpu().numpy()
        if verdict != OK:
            assert (ras == REF_FILL).all(), "the reference decode of a rejected header wrote its raster"
        self._refs[key] = (ras, verdict)
        return self._refs[key]

    def _oracle(self, oracle, sub):
        from metalhuffman_amd.codec import Huffman
        fs, ef = self.fs, self.fs.efs[sub.frame]
        canon = ef.canon if sub.header is None else np.frombuffer(sub.header, np.uint8)
        t1, t2 = Huffman.generateSplitLookupTables(canon)
        return oracle.decode_frame_shader(ef.block_offsets, ef.codes, t1, t2, fs.w, fs.h, block_init=ef.block_init,
                                          delta=fs.fmt != "no_delta")

    def _differ(self, got, want, what):
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
            cols = got.shape[-1] if got.ndim == 2 else self.pitch
            y, x = divmod(int(bad[0]), cols)
            raise AssertionError(f"{what}: {bad.size} byte(s) differ, first at row {y}, column {x}: "
                                 f"{int(got.reshape(-1)[bad[0]]):#04x}, expected {int(want.reshape(-1)[bad[0]]):#04x}")

    def check(self, oracle=None, oracle_subs=(0,), verdicts=None):
        """After sync() or close(): every submission's result, every raster's final content, every
        guard byte, and in header mode every slot's status. verdicts: {submission: expected verdict}
        for the submissions that are not MH_OK."""
        fs, w = self.fs, self.fs.w
        verdicts = verdicts or {}
        for sub in self.subs:
            what = f"submission {sub.k} (frame {sub.frame}, {fs.sizes[sub.frame]} code bytes, member {sub.member}, slot {sub.slot})"
            ref, verdict = self.reference(sub.frame, sub.header)
            assert verdict == verdicts.get(sub.k, OK), f"{what}: the direct decode's verdict is {verdict}"
            if verdict == OK:
                self.cur[sub.member, sub.slot] = ref
            sub.verdict = verdict
            want = self.cur[sub.member, sub.slot]           # a rejected frame: what the raster held before
            if not self.consume:
                continue
            got = sub.result.cpu().numpy()
            self._differ(got, want, what + (" against the direct decode" if verdict == OK else ": a rejected frame's raster changed"))
            if verdict == OK:
                img = got.reshape(fs.h, self.pitch)[:, :w]
                self._differ(img, fs.imgs[sub.frame], what + " against the image")
                if oracle is not None and sub.k in oracle_subs:
                    self._differ(img, self._oracle(oracle, sub), what + " against the oracle")
        if oracle is not None and self.consume:
            assert any(s.k in oracle_subs and s.verdict == OK for s in self.subs), "no frame went to the oracle"
        for (m, s), want in self.cur.items():
            what = f"member {m}, slot {s}"
            if not self.owned:
                got = self.rasters[s].host("after the run, " + what)
            elif not self.closed:
                got = self.views[m, s].cpu().numpy()
            else:
                continue
            self._differ(got, want, "the final raster of " + what)
        if self.headers and not self.closed:
            for s in range(self.slots):
                want = self.last[0, s].verdict if (0, s) in self.last else OK
                assert self.status(s) == want, (s, self.status(s), want)

    def finish(self, oracle=None, oracle_subs=(0,), verdicts=None):
        self.sync()
        self.check(oracle, oracle_subs, verdicts)
        self.close()
        if not self.owned:
            for s, r in enumerate(self.rasters):
                r.host(f"after destroy, slot {s}")


def run_checked(mh, oracle, device, fs, order, *, wait=False, **kw):
    d = Driver(mh, device, fs, **kw)
    try:
        d.run(order, wait=wait)
        d.finish(oracle)
    finally:
        d.close()
    return d


# ---- the seeded sweep --------------------------------------------------------------------------------

SWEEP_DEFAULT_CASES = 32
EDGES = (1, 7, 8, 9, 63, 64, 65, 264)
SIZES = EDGES + (33, 130, 200)          # 11 values: taken in turn with strides coprime to 11


@dataclasses.dataclass(frozen=True)
class SweepCase:
    mode: str
    i: int
    W: int
    H: int
    slots: int
    frames: int
    fmt: str
    packed: bool
    pinned: bool
    owned: bool
    graphs: bool
    prepared: bool              # table mode only (header mode has no table)
    wait: bool

    @property
    def nb(self):
        return n_blocks(self.W, self.H)

    def describe(self):
        return (f"sweep_case({self.mode!r}, {self.i}): {self.W} x {self.H} ({self.nb} blocks), {self.slots} slot(s), "
                f"{self.frames} frames, {self.fmt}, {'one buffer' if self.packed else 'separate buffers'}, "
                f"{'pinned' if self.pinned else 'pageable'}, {'own' if self.owned else 'caller'} rasters, graphs "
                f"{self.graphs}, prepared {self.prepared}, {'waiting' if self.wait else 'back to back'}")


def sweep_case(mode, i):
    """Case i of `mode`: everything follows from (mode, i) alone, from fixed lists taken in turn."""
    m, i = MODES.index(mode), int(i)
    W = SIZES[(i + 4 * m) % len(SIZES)]
    H = SIZES[(5 * i + 3 + m) % len(SIZES)]
    slots = 1 + (i + m) % 4
    frames = 2 + (i + i // 8 + 3 * m) % 8
    fmt = FORMATS[(i + i // 3 + m) % 3]
    j = (13 * i + 5 + 7 * m) % 32           # a bijection of 0..31: five balanced, independent bits
    bit = [bool((j >> b) & 1) for b in range(5)]
    wait = bool((i // 2 + i // 16 + m) % 2)
    return SweepCase(mode, i, W, H, slots, frames, fmt, bit[0], bit[1], bit[2], bit[3], bit[4], wait)


def sweep_frames(mh, case):
    """-> (FrameSet, submit order): slot_order over the case's frames."""
    fs = frame_set(mh, case.mode, case.W, case.H, case.frames, case.fmt, seed=1000 * MODES.index(case.mode) + case.i)
    return fs, slot_order(fs.sizes, case.slots)


def run_sweep_case(mh, oracle, device, case):
    fs, order = sweep_frames(mh, case)
    try:
        run_checked(mh, oracle, device, fs, order, wait=case.wait, slots=case.slots, packed=case.packed,
                    pinned=case.pinned, owned=case.owned, prepared=case.prepared, graphs=case.graphs)
    except Exception as e:
        raise AssertionError(f"{case.describe()}\n{type(e).__name__}: {e}") from e


def sweep_range():
    """(first, count) of the default sweep, or of another one asked for through the environment."""
    return int(os.environ.get("MH_STREAM_SWEEP_FIRST", "0")), int(os.environ.get("MH_STREAM_SWEEP_CASES",
                                                                                 str(SWEEP_DEFAULT_CASES)))
