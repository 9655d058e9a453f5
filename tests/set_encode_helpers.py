"""A raw-ABI driver for mh_encode_set_device_async (test_gpu_encode_set.py), in the style of
encode_helpers.py: every frame's pixels in an allocation of its own inside seeded garbage, every
output at a 256-byte boundary inside a guard-filled tensor, and the host codec (mh.encode_frame),
frame by frame, as the standard; never another GPU encode."""
from __future__ import annotations

import contextlib
import ctypes
import dataclasses
from typing import Optional

import numpy as np

import encode_helpers as EH
from encode_helpers import FILL_BYTES, FILL_STATUS, FILL_U32, FILL_U64, LIMIT, NO_DELTA, OK, r4, r16

# the tile and pack-unit edges (kBatchTile = 256 blocks, a pack unit of 4 tiles), large, small, large
EDGE_SET = [(256, 256), (128, 128), (2056, 8), (9, 7), (264, 256), (1, 1), (40, 400)]


def images(bigbridge, sizes, seed=0):
    """One natural frame per size (crops of the picture, every other one block-shuffled)."""
    return [EH.natural_frames(bigbridge, w, h, 1, seed + 7 * i + (i % 2))[0] if (w, h) != (1, 1)
            else np.array([[37 + i]], np.uint8) for i, (w, h) in enumerate(sizes)]


@dataclasses.dataclass
class Source:
    """Where frame f's samples lie: `tensor` keeps the allocation alive."""
    tensor: object
    pixels: int
    pitch: int
    ps: int


def planar_sources(device, imgs, aligned, seed=3):
    """Each frame in an allocation of its own. aligned: rows padded to a multiple of 4 bytes behind a
    4-byte aligned address (the dword mode at pixel stride 1); else tight rows at an odd address."""
    import torch
    out = []
    for i, im in enumerate(imgs):
        h, w = im.shape
        pitch = (w + 3) // 4 * 4 + 4 if aligned else w
        lead = 64 if aligned else 61
        buf = np.random.default_rng([seed, i, w, h]).integers(0, 256, 256 + lead + pitch * h + 64, dtype=np.uint8)
        t = torch.empty(buf.size, dtype=torch.uint8, device=device)
        base = (t.data_ptr() + 255) // 256 * 256 - t.data_ptr() + lead
        rows = buf[base: base + pitch * h].reshape(h, pitch)
        rows[:, :w] = im
        t.copy_(torch.from_numpy(buf))
        out.append(Source(t, t.data_ptr() + base, pitch, 1))
    return out


def interleaved_sources(device, planes_of, K, pitch_extra, seed=5):
    """HWC images: planes_of[i] is the list of K planes [H_i, W_i] of image i, interleaved with a row
    pitch of W * K + pitch_extra rounded up to 4 when pitch_extra is 0 (the dword mode), else as it is
    (3 W + 1: the byte mode). Frame i * K + c is plane c of image i."""
    import torch
    out = []
    for i, planes in enumerate(planes_of):
        h, w = planes[0].shape
        pitch = (w * K + 3) // 4 * 4 if pitch_extra == 0 else w * K + pitch_extra
        buf = np.random.default_rng([seed, i, w, h, K]).integers(0, 256, 256 + pitch * h + 64, dtype=np.uint8)
        t = torch.empty(buf.size, dtype=torch.uint8, device=device)
        base = (t.data_ptr() + 255) // 256 * 256 - t.data_ptr()
        rows = buf[base: base + pitch * h].reshape(h, pitch)
        for c in range(K):
            rows[:, c: w * K: K] = planes[c]
        t.copy_(torch.from_numpy(buf))
        out += [Source(t, t.data_ptr() + base + c, pitch, K) for c in range(K)]
    return out


def roomy_cap(w, h):
    return EH.roomy_slot(w, h)


@dataclasses.dataclass
class SetRun:
    rc: int
    plan: object                # codec.SetPlan
    caps: list
    nbs: list
    flags: int
    init_zero: bool
    host: dict                  # name -> the payload on the host (guards already checked)
    dev: dict                   # name -> _Out
    plan_dev: object
    alive: object = None        # what the launches read and write besides the outputs

    def collect(self):
        """The outputs on the host, every guard byte compared (after a synchronisation)."""
        self.host = {k: v.host(f"set: {k}") for k, v in self.dev.items()}
        return self

    def _first(self, f):
        return int(self.plan.geoms[f, 0])

    def codes(self, f):
        s = sum(self.caps[:f])
        return self.host["codes"][s: s + self.caps[f]]

    def offsets(self, f):
        return self.host["offs"].view(np.uint32)[self._first(f): self._first(f) + self.nbs[f]]

    def init(self, f):
        return self.host["init"][self._first(f): self._first(f) + self.nbs[f]]

    def header(self, f):
        return self.host["canon"][256 * f: 256 * f + 256]


def run(mh, device, imgs, srcs, *, flags=0, init_zero=False, caps=None, workspace=None, ws_fill=0x5C, zeroed=False,
        null=(), totals=None, stream=None, sync=True):
    """One call -> SetRun. The workspace (any content: filled with ws_fill when made here) may be
    handed on to a second call. zeroed: a zero-filled workspace and MH_ENCODE_WORKSPACE_ZEROED.
    null: of "lens" and "st", the optional outputs passed as NULL. totals: a changed copy of the
    planner's to hand to the entry (every output keeps its planned size). stream: a torch stream
    other than the current one. sync False: nothing waits; SetRun.collect() does."""
    import torch
    sizes = [(im.shape[1], im.shape[0]) for im in imgs]
    caps = [roomy_cap(w, h) for w, h in sizes] if caps is None else list(caps)
    plan = mh.encode_set_plan([(s.pixels, s.pitch, s.ps, w, h, c) for s, (w, h), c in zip(srcs, sizes, caps)], flags)
    t = plan.totals
    n = len(imgs)
    nbs = [EH.blocks(w, h)[0] * EH.blocks(w, h)[1] for w, h in sizes]
    assert t.total_blocks == sum(nbs) and t.codes_bytes == sum(caps)
    assert set(null) <= {"lens", "st"}
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        if workspace is None:
            workspace = torch.full((int(t.workspace_bytes) + 256,), 0 if zeroed else ws_fill, dtype=torch.uint8,
                                   device=device)
        plan_dev = torch.from_numpy(plan.plan).to(device)
        o = dict(codes=EH._Out(device, int(t.codes_bytes), 0, FILL_BYTES),
                 offs=EH._Out(device, 4 * int(t.total_blocks), 0, FILL_U32),
                 canon=EH._Out(device, 256 * n, 0, FILL_BYTES),
                 lens=EH._Out(device, 8 * n, 0, FILL_U64),
                 fco=EH._Out(device, 8 * (n + 1), 0, FILL_U64),
                 st=EH._Out(device, 4 * n, 0, FILL_STATUS))
        if init_zero:
            o["init"] = EH._Out(device, int(t.total_blocks), 0, FILL_BYTES)
    for k in null:
        del o[k]
    if zeroed:
        flags |= EH.ZEROED
    wsp = (workspace.data_ptr() + 255) // 256 * 256
    wsb = workspace.numel() - (wsp - workspace.data_ptr())
    s = torch.cuda.current_stream(device) if stream is None else stream
    rc = mh.lib().mh_encode_set_device_async(
        plan_dev.data_ptr(), ctypes.byref(t if totals is None else totals), flags, o["canon"].ptr, o["codes"].ptr,
        int(t.codes_bytes), o["lens"].ptr if "lens" in o else None, o["fco"].ptr, o["offs"].ptr,
        o["init"].ptr if init_zero else None, o["st"].ptr if "st" in o else None, wsp, wsb, ctypes.c_void_p(s.cuda_stream))
    r = SetRun(int(rc), plan, caps, nbs, flags, init_zero, None, o, plan_dev, (srcs, workspace))
    if sync:
        torch.cuda.synchronize(device)
        r.collect()
    return r, workspace


def expect(mh, imgs, caps, flags=0, init_zero=False):
    """(status, EncodedFrame or None) per frame, from the host codec."""
    out = []
    for im, cap in zip(imgs, caps):
        try:
            ef = mh.encode_frame(im, flags=flags & NO_DELTA, init_zero_delta=init_zero, limit_lengths=bool(flags & LIMIT))
        except mh.MHError as e:
            out.append((e.status, None))
            continue
        out.append((EH.CAPACITY, None) if r4(ef.codes.size) > cap else (OK, ef))
    return out


def check(r, exp, frames=None, fco_end=None):
    """One call's outputs against the host codec, frame by frame. An optional output that went in as
    NULL is left out, and the verdict is read off the other one (d_codes_len 0: rejected). frames:
    the frames to compare (default: all); fco_end: d_frame_code_offsets[n] where it is not the plan's."""
    assert r.rc == OK, r.rc
    assert len(exp) == len(r.caps)
    lens = r.host["lens"].view(np.uint64) if "lens" in r.host else None
    st = r.host["st"].view(np.int32) if "st" in r.host else None
    want_fco = np.concatenate([[0], np.cumsum(r.caps)]).astype(np.uint64)
    if fco_end is not None:
        want_fco[-1] = fco_end
    assert np.array_equal(r.host["fco"].view(np.uint64), want_fco), "d_frame_code_offsets"
    frames = range(len(exp)) if frames is None else frames
    if st is not None:
        assert [int(st[f]) for f in frames] == [exp[f][0] for f in frames], ([int(s) for s in st], [s for s, _ in exp])
    for f in frames:
        status, ef = exp[f]
        got = r.codes(f)
        if status != OK:
            assert lens is None or int(lens[f]) == 0, f
            assert (got == FILL_BYTES).all(), f"rejected frame {f}: code bytes written"
            assert (r.offsets(f) == 0x3C3C3C3C).all(), f"rejected frame {f}: offsets written"
            continue                # its d_block_init entries and its header: unspecified
        k = ef.codes.size
        assert lens is None or int(lens[f]) == k, (f, int(lens[f]), k)
        assert np.array_equal(r.header(f), ef.canon), f"frame {f}: header"
        if not np.array_equal(got[:k], ef.codes):
            bad = np.flatnonzero(got[:k] != ef.codes)
            raise AssertionError(f"frame {f}: {bad.size} of {k} code bytes differ, first at {int(bad[0])}, last at "
                                 f"{int(bad[-1])}")
        assert (got[k: r4(k)] == 0).all(), f"frame {f}: pad bytes {got[k: r4(k)]}"
        tail = got[r4(k):]
        assert (tail == FILL_BYTES).all(), (f"frame {f}: {int((tail != FILL_BYTES).sum())} byte(s) written behind "
                                           f"round_up(codes_len, 4) = {r4(k)} of a slot of {r.caps[f]}")
        assert np.array_equal(r.offsets(f), ef.block_offsets), f"frame {f}: block offsets"
        if r.init_zero:
            assert np.array_equal(r.init(f), ef.block_init), f"frame {f}: init bytes"


def fetch_rule(records):
    """totals.fetch_mode by the rule of include/metalhuffman.h, from (pixels, row_pitch, pixel_stride,
    width, height, ...) records: dword loads when every record has the same pixel_stride <= 4, every
    row_pitch (for height > 1) is a multiple of 4 and every pixels % 4 < pixel_stride; else bytes."""
    ps = records[0][2]
    dwords = ps <= 4 and all(r[2] == ps and r[0] % 4 < ps and (r[4] == 1 or r[1] % 4 == 0) for r in records)
    return ps if dwords else 0xFF


def frame_set_of(r):
    """A SetRun's outputs as the decoders' DeviceFrameSet: views of the guarded tensors, and the plan's
    own geometry records (d_plan + geoms_offset)."""
    import torch
    from metalhuffman_amd import decoder as D
    t, n = r.plan.totals, len(r.caps)
    o = r.dev
    geoms = r.plan_dev[int(t.geoms_offset): int(t.geoms_offset) + 16 * n].view(torch.int32).view(n, 4)
    sizes = tuple((int(g[1]), int(g[2])) for g in r.plan.geoms)
    return D.DeviceFrameSet(int(t.max_width), int(t.max_height), n, sizes, int(t.total_blocks),
                            o["offs"].view().view(torch.int32), o["codes"].view(), o["fco"].view().view(torch.int64),
                            geoms, o["init"].view() if r.init_zero else None, r.flags & NO_DELTA, int(t.codes_bytes))


def decode_back(device, r, imgs, exp):
    """The set decoded straight back on the device (set_helpers.run_crops): the four corners of every
    frame, the crop size the set's smallest frame capped at 24 x 16, tables built on the device from
    the device headers, the encoder's d_status as d_frame_status (where it went in as NULL: the
    expected status of the frames whose d_codes_len is 0 on the device, else the table build's; where
    both went in as NULL no frame is rejected and the table build's words go in).
    Accepted frames' crops are the source pixels; a rejected frame's report its status and write
    nothing; every byte of the guarded output is compared."""
    import torch
    import set_helpers as S
    from metalhuffman_amd import decoder as D
    n = len(imgs)
    cw, ch = min(24, min(im.shape[1] for im in imgs)), min(16, min(im.shape[0] for im in imgs))
    fs = frame_set_of(r)
    tabs = D.DeviceTableSet.from_canonical_headers(r.dev["canon"].view().view(n, 256), device)
    if "st" in r.dev:
        fst = r.dev["st"].view().view(torch.int32)
    elif "lens" not in r.dev:       # both NULL: only in a case without a rejection
        assert all(s == OK for s, _ in exp)
        fst = "tables"
    else:
        want = torch.tensor([s for s, _ in exp], dtype=torch.int32, device=device)
        fst = torch.where(r.dev["lens"].view().view(torch.int64) == 0, want, tabs.status)
    desc = [(f, x0, y0, 0) for f, im in enumerate(imgs)
            for x0, y0 in ((0, 0), (im.shape[1] - cw, 0), (0, im.shape[0] - ch), (im.shape[1] - cw, im.shape[0] - ch))]
    lay = S.run_crops(device, fs, tabs, desc, (cw, ch), frame_status=fst)
    assert lay.rc == 0, lay.rc
    S.check(lay, [[S.pixels(imgs, d, (cw, ch))] if exp[d[0]][0] == OK else None for d in desc])
    assert lay.status == [exp[d[0]][0] for d in desc], (lay.status, [exp[d[0]][0] for d in desc])


# ---- the seeded sweep of sets (test_gpu_encode_set_sweep.py; asserted in test_encode_set_sweep_cases.py) ----

SET_SWEEP_SALT = 56
SET_SWEEP_DEFAULT_CASES = 48
BLOCK_CAP = 6000                # a case's blocks: the host codec's time
BLOCK_CAP_WIDE = 1500           # ... at a pixel stride of 255 (the source's bytes)
KINDS = ("planar", "interleaved", "windows", "strided")
KIND_OF = ("interleaved", "planar", "interleaved", "windows", "interleaved", "strided", "interleaved", "planar")   # i % 8
# interleaved: (K, first plane taken) in turn -- all planes, then every suffix
PLANES_OF = ((1, 0), (2, 1), (3, 0), (4, 3), (3, 2), (2, 0), (4, 1), (3, 1), (4, 0), (4, 2), (4, 3), (3, 2))
BYTE_STRIDES = (5, 7, 16, 255)
# the edge list: (name, W or None, H or None, grid in blocks); None: anywhere in the grid's last block
EDGES = (("1x1", 1, 1, (1, 1)), ("8x8", 8, 8, (1, 1)), ("nb255", None, None, (51, 5)), ("nb256", None, None, (32, 8)),
         ("nb257", None, None, (257, 1)), ("nb1023", None, None, (93, 11)), ("nb1024", None, None, (64, 16)),
         ("nb1025", None, None, (205, 5)), ("w2033", 2033, None, (255, 0)), ("w2041", 2041, None, (256, 0)),
         ("w2048", 2048, None, (256, 0)), ("w2056", 2056, None, (257, 0)))
PATTERNS = ("none", "first", "last", "pair", "multi", "random")
SLOTS = ("roomy", "exact", "less16", "cap16")
DEEP_MIN_BLOCKS = 110           # limit_helpers.fib_counts_within: 18 Fibonacci counts need 6,764 symbols


@dataclasses.dataclass(frozen=True)
class Rec:
    """Frame f's samples: `off` bytes behind allocation `alloc`'s 256-byte aligned base."""
    alloc: int
    off: int
    pitch: int
    ps: int
    w: int
    h: int

    def record(self, base=0):
        return (base + self.off, self.pitch, self.ps, self.w, self.h)

    @property
    def nb(self):
        return EH.blocks(self.w, self.h)[0] * EH.blocks(self.w, self.h)[1]

    @property
    def span(self):
        return self.off + (self.h - 1) * self.pitch + (self.w - 1) * self.ps + 1


@dataclasses.dataclass(frozen=True)
class SetCase:
    i: int
    kind: str
    K: int                      # interleaved: channels of a pixel
    first: int                  # ... and the first plane taken (> 0: a suffix of the planes)
    aligned: bool               # drawn for the dword mode (before the breaker)
    breaker: Optional[str]      # None, "address" or "pitch": the one allocation that breaks the dword mode
    recs: tuple                 # Rec per frame
    windows: Optional[tuple]    # windows: (picture, x0, y0) per frame
    pictures: tuple             # windows: (PW, PH) per picture
    edge: str
    edge_pos: int               # the first frame of the edge size
    pattern: str
    slots: tuple                # one of SLOTS per frame
    deep: Optional[int]
    no_delta: bool
    init_zero: bool
    limit: bool
    ws_fill: Optional[int]      # None: a zero-filled workspace and MH_ENCODE_WORKSPACE_ZEROED
    null_lens: bool
    null_status: bool

    @property
    def n(self):
        return len(self.recs)

    @property
    def flags(self):
        return (NO_DELTA if self.no_delta else 0) | (LIMIT if self.limit else 0)

    @property
    def null(self):
        return (("lens",) if self.null_lens else ()) + (("st",) if self.null_status else ())

    @property
    def fetch_mode(self):
        """By the header's rule, the allocations' bases being 256-byte aligned."""
        return fetch_rule([r.record() for r in self.recs])

    def alloc_bytes(self, a):
        return max(r.span for r in self.recs if r.alloc == a) + 64

    def describe(self):
        return (f"set sweep_case({self.i}): {self.kind} K {self.K} first {self.first}, aligned {self.aligned}, breaker "
                f"{self.breaker}, frames {[(r.w, r.h) for r in self.recs]}, records {[r.record() for r in self.recs]}, "
                f"edge {self.edge} at {self.edge_pos}, pattern {self.pattern}, slots {self.slots}, deep {self.deep}, "
                f"no_delta {self.no_delta}, init {self.init_zero}, limit {self.limit}, ws_fill {self.ws_fill}, "
                f"null {self.null}")


def _tiles(bw, bh):
    return -(-bw * bh // EH.K_BATCH_TILE)


def sweep_case(i):
    """Case i: everything follows from i alone. Frames are drawn per UNIT (one frame; interleaved: the
    C planes taken of one image, which share a size and an allocation)."""
    i = int(i)
    r = np.random.default_rng([i, SET_SWEEP_SALT])
    kind = KIND_OF[i % 8]
    K, first = PLANES_OF[(i // 2) % len(PLANES_OF)] if kind == "interleaved" else (1, 0)
    C = K - first
    ps = K if kind == "interleaved" else BYTE_STRIDES[(i // 8) % 4] if kind == "strided" else 1
    pattern = PATTERNS[int(r.choice(len(PATTERNS), p=[0.3, 0.12, 0.12, 0.16, 0.15, 0.15]))]
    if pattern == "multi" and C > 1:
        pattern = "pair"        # sibling planes share a size: no multi-tile frame between one-tile ones
    n = 1 if r.random() < 0.08 else int(r.integers(1, 13))
    least = {"pair": 3, "multi": 3, "first": 2, "last": 2}.get(pattern, 1)      # frames the pattern needs
    units = max(n // C, -(-least // C))
    # grids in blocks and the pixels cut off the last block, per unit
    grid = [[int(np.exp(r.uniform(0.0, np.log(301.0)))), int(r.integers(1, 25))] for _ in range(units)]
    cut = [(0 if r.random() < 0.4 else int(r.integers(1, 8)), int(r.integers(0, 8))) for _ in range(units)]
    pinned = set()
    name, eW, eH, (ebw, ebh) = EDGES[i % len(EDGES)]
    ebh = ebh or int(r.integers(1, 4))
    edge_multi = _tiles(ebw, ebh) > 1
    m = None
    if pattern == "multi":
        m = int(r.integers(1, units - 1))
        pos = m if edge_multi else int(r.choice([u for u in range(units) if u != m]))
        if _tiles(*grid[m]) == 1:
            grid[m] = [int(r.integers(33, 121)), int(r.integers(9, 21))]
        for u in (m - 1, m + 1):
            if _tiles(*grid[u]) > 1:
                grid[u][1] = 256 // grid[u][0] if grid[u][0] <= 256 else 1
                grid[u][0] = min(grid[u][0], 256)
        pinned.add(m)
    else:
        pos = int(r.integers(0, units))
    grid[pos] = [ebw, ebh]
    pinned.add(pos)
    deep = None
    free = [u for u in range(units) if u not in pinned and (m is None or abs(u - m) > 1)]
    if kind != "windows" and free and r.random() < 0.25:
        deep = int(r.choice(free))
        bw = int(r.integers(8, 33))
        grid[deep] = [bw, -(-DEEP_MIN_BLOCKS // bw) + int(r.integers(0, 6))]
        cut[deep] = (0, 0)      # image_from_histogram: whole blocks
        pinned.add(deep)
    # the cap: the pinned units keep their size, the others shrink in turn to what is left
    cap = (BLOCK_CAP_WIDE if ps == 255 else BLOCK_CAP) // C
    left = cap - sum(grid[u][0] * grid[u][1] for u in pinned)
    todo = units - len(pinned)
    for u in range(units):
        if u in pinned:
            continue
        todo -= 1
        room = max(1, left - todo)
        if grid[u][0] * grid[u][1] > room:
            grid[u][0] = min(grid[u][0], room)
            grid[u][1] = max(1, room // grid[u][0])
        left -= grid[u][0] * grid[u][1]
    dims = [(8 * bw - cx, 8 * bh - cy) for (bw, bh), (cx, cy) in zip(grid, cut)]
    dims[pos] = (eW or dims[pos][0], eH or dims[pos][1])
    # where the samples lie
    aligned = bool(r.random() < (0.5 if kind == "planar" else 0.75)) and ps <= 4
    recs, windows, pictures = [], None, ()
    if kind == "windows":
        npic = 1 if r.random() < 0.6 else 2
        pic_of = [int(r.integers(0, npic)) for _ in range(units)]
        pic_of[0] = 0
        npic = max(pic_of) + 1
        pictures, leads, pitches = [], [], []
        for p in range(npic):
            PW = max(w for (w, h), q in zip(dims, pic_of) if q == p) + int(r.integers(0, 200))
            PH = max(h for (w, h), q in zip(dims, pic_of) if q == p) + int(r.integers(0, 40))
            pictures.append((PW, PH))
            leads.append(4 * int(r.integers(0, 16)) if aligned else int(r.integers(0, 64)))
            pitches.append(r4(PW) + 4 * int(r.integers(0, 3)) if aligned else PW + int(r.integers(0, 8)))
        windows = []
        for (w, h), p in zip(dims, pic_of):
            x0, y0 = int(r.integers(0, pictures[p][0] - w + 1)), int(r.integers(0, pictures[p][1] - h + 1))
            x0 -= x0 % 4 if aligned else 0
            windows.append((p, x0, y0))
            recs.append(Rec(p, leads[p] + y0 * pitches[p] + x0, pitches[p], 1, w, h))
        pictures, windows = tuple(pictures), tuple(windows)
    else:
        for u, (w, h) in enumerate(dims):
            lead = 4 * int(r.integers(0, 16)) if aligned else int(r.integers(0, 64))
            pitch = r4(w * ps) + 4 * int(r.integers(0, 3)) if aligned else w * ps + int(r.integers(0, 9))
            recs += [Rec(u, lead + c, pitch, ps, w, h) for c in range(first, K)]
    # the breaker: one allocation's address or pitch (windows: one window's address) breaks the dword mode
    breaker = None
    if fetch_rule([q.record() for q in recs]) != 0xFF and r.random() < 0.35:
        by_address = [f for f, q in enumerate(recs) if ps < 4 and (kind != "windows" or pictures[q.alloc][0] > q.w)]
        by_pitch = [f for f, q in enumerate(recs) if q.h > 1 and kind != "windows"]
        want = "address" if r.random() < 0.5 else "pitch"
        if want == "address" and by_address or not by_pitch:
            if by_address:
                f = int(r.choice(by_address))
                q = recs[f]
                if kind == "windows":
                    p, x0, y0 = windows[f]
                    x1 = x0 + 1 if x0 + q.w < pictures[p][0] else x0 - 1
                    windows = windows[:f] + ((p, x1, y0),) + windows[f + 1:]
                    recs[f] = dataclasses.replace(q, off=q.off + x1 - x0)
                else:   # the allocation's first record lands on byte ps of a dword
                    a0 = min(x.off for x in recs if x.alloc == q.alloc)
                    d = (ps - a0) % 4
                    recs = [dataclasses.replace(x, off=x.off + d) if x.alloc == q.alloc else x for x in recs]
                breaker = "address"
        else:
            a = recs[int(r.choice(by_pitch))].alloc
            d = int(r.integers(1, 4))
            recs = [dataclasses.replace(x, pitch=x.pitch + d) if x.alloc == a else x for x in recs]
            breaker = "pitch"
    n = len(recs)
    # slots
    slots = ["roomy" if r.random() < 0.6 else "exact" for _ in range(n)]
    small = lambda: SLOTS[2 + int(r.integers(0, 2))]
    if pattern == "first":
        slots[0] = small()
    elif pattern == "last":
        slots[n - 1] = small()
    elif pattern == "pair":
        p = int(r.integers(0, n - 1))
        slots[p], slots[p + 1] = small(), small()
    elif pattern == "multi":
        slots[m] = small()
    elif pattern == "random":
        for f in range(n if n == 1 else n - 1):     # the last of several frames is kept
            if r.random() < 0.2:
                slots[f] = small()
    deep_frame = None if deep is None else deep * C + int(r.integers(0, C))
    no_delta, init_zero, limit = bool(r.random() < 0.25), bool(r.random() < 0.4), bool(r.random() < 0.4)
    ws_fill = None if r.random() < 0.5 else int(r.integers(1, 256))
    null_lens, null_status = bool(r.random() < 0.25), bool(r.random() < 0.25)
    if null_lens and null_status and (pattern != "none" or (deep is not None and not limit)):
        null_lens = bool(r.random() < 0.5)          # a verdict needs one of them
        null_status = not null_lens
    return SetCase(i, kind, K, first, aligned, breaker, tuple(recs), windows, pictures, name, pos * C, pattern, tuple(slots),
                   deep_frame, no_delta, init_zero, limit, ws_fill, null_lens, null_status)


def sweep_images(case, bigbridge):
    """The frames' pixels: natural ones (windows: slices of natural pictures), and the deep frame."""
    import limit_helpers as LH
    if case.kind == "windows":
        pics = [EH.natural_frames(bigbridge, PW, PH, 1, seed=5000 + 13 * case.i + p)[0]
                for p, (PW, PH) in enumerate(case.pictures)]
        return [np.ascontiguousarray(pics[p][y0: y0 + q.h, x0: x0 + q.w]) for q, (p, x0, y0) in zip(case.recs, case.windows)]
    imgs = [EH.natural_frames(bigbridge, q.w, q.h, 1, seed=5000 + 13 * case.i + f)[0] for f, q in enumerate(case.recs)]
    if case.deep is not None:
        q = case.recs[case.deep]
        imgs[case.deep] = LH.image_from_histogram(LH.fib_histogram(20, q.w * q.h, seed=case.i), q.w, q.h, seed=case.i,
                                                  no_delta=case.no_delta)
    return imgs


def sweep_plan(mh, case, bigbridge):
    """-> (images, caps, expectation): the slots from the host's code lengths. exact: r16(r4(codes_len));
    less16: 16 below that, cap16: 16 bytes (neither can reject a frame of 16 code bytes or fewer: the
    expectation is the host codec's either way); a frame the host rejects for its tree keeps roomy."""
    imgs = sweep_images(case, bigbridge)
    roomy = [roomy_cap(q.w, q.h) for q in case.recs]
    free = expect(mh, imgs, [1 << 62] * case.n, case.flags, case.init_zero)
    caps = []
    for (s, ef), slot, big in zip(free, case.slots, roomy):
        exact = r16(r4(ef.codes.size)) if s == OK else big
        caps.append({"roomy": big, "exact": exact, "less16": max(16, exact - 16), "cap16": 16}[slot] if s == OK else big)
    exp = [(s, ef) if s != OK or r4(ef.codes.size) <= c else (EH.CAPACITY, None) for (s, ef), c in zip(free, caps)]
    return imgs, caps, exp


def materialize(device, case, imgs):
    """The case's allocations on the device, each seeded garbage with the frames' samples written in
    (the bytes between samples -- other channels, pitch padding -- stay garbage) -> [Source]."""
    import torch
    out = [None] * case.n
    for a in sorted({q.alloc for q in case.recs}):
        size = case.alloc_bytes(a)
        buf = np.random.default_rng([SET_SWEEP_SALT, case.i, a]).integers(0, 256, 256 + size, dtype=np.uint8)
        t = torch.empty(buf.size, dtype=torch.uint8, device=device)
        base = (t.data_ptr() + 255) // 256 * 256 - t.data_ptr()
        for f, q in enumerate(case.recs):
            if q.alloc == a:
                np.lib.stride_tricks.as_strided(buf[base + q.off:], (q.h, q.w), (q.pitch, q.ps))[...] = imgs[f]
                out[f] = Source(t, t.data_ptr() + base + q.off, q.pitch, q.ps)
        t.copy_(torch.from_numpy(buf))
    return out


def run_sweep_case(mh, device, case, bigbridge):
    imgs, caps, exp = sweep_plan(mh, case, bigbridge)
    try:
        srcs = materialize(device, case, imgs)
        r, _ = run(mh, device, imgs, srcs, flags=case.flags, init_zero=case.init_zero, caps=caps,
                   zeroed=case.ws_fill is None, ws_fill=case.ws_fill, null=case.null)
        want = fetch_rule([(s.pixels, s.pitch, s.ps, q.w, q.h) for s, q in zip(srcs, case.recs)])
        assert r.plan.totals.fetch_mode == want == case.fetch_mode, (r.plan.totals.fetch_mode, want, case.fetch_mode)
        check(r, exp)
        decode_back(device, r, imgs, exp)
    except AssertionError as err:
        raise AssertionError(f"{case.describe()}: {err}") from err


def sweep_range():
    """(first, count) of the default sweep, or of another one asked for through the environment."""
    import os
    return (int(os.environ.get("MH_ENCODE_SET_SWEEP_FIRST", "0")),
            int(os.environ.get("MH_ENCODE_SET_SWEEP_CASES", str(SET_SWEEP_DEFAULT_CASES))))
