"""Helpers of the defect tests (test_defect_cases.py, test_gpu_check_sweep.py, test_gpu_defect_isolation.py):
a seeded generator of batches in which some frames carry a defect, and what the decode contract
(include/metalhuffman.h, mh_frame) says about every block of them, computed without any code under test.

The reference walk of block b is the oracle's 64 steps from offsets[b] over the frame's slot, bytes at or
past the slot's end reading zero (oracle.walk_frame, pinned here against oracle.check_frame's totals).
Block b is SPECIFIED when its walk ends at or before offsets[b + 1] -- the frame's last block: at or
before 8 x the slot's bytes. Specified pixels must equal the oracle's decode of the frame's own slot;
the others may hold anything, but only where the entry may write. The expected raster is
oracle.decode_frame_shader over a copy of the slot with 256 zero bytes behind it (it reads unbounded).

A case follows from (entry, i) alone: defect_case(mh, oracle, entry, i)."""
from __future__ import annotations

import ctypes
import dataclasses
import os

import numpy as np

import norm_helpers as NH
import region_helpers as R
import scaled_helpers as S
import slice_helpers as SH
from helpers import frame_under_header, header_zoo, kraft_sum

DECODES = ("decode_tables", "decode_batch", "decode_small", "frame")   # the four ways into mh_decode
NORMS = ("crops_norm", "crops_norm_planes")
ENTRIES = DECODES + SH.ENTRIES + NORMS
CHECK = "check"
ALL = ENTRIES + (CHECK,)

# two incomplete headers beside slice_helpers' flavours: only under these does a window match no code
FLAVOURS = dict(SH.FLAVOURS, single=("single", "delta"), quarter=("quarter", "delta"))
GROUPS = {
    "natural": ("escapes", "noesc", "flat", "no_delta", "block_init"),
    "8x256": ("8x256",),            # the flat byte step
    "16x256": ("16x256",),          # every tile takes decode_halves
    "incomplete": ("single", "quarter"),
}
INCOMPLETE = GROUPS["incomplete"]
DECODE_KINDS = ("none", "flip", "ff", "seeded", "replace", "move", "equal", "cut")
CHECK_KINDS = ("swap", "past")      # break the decoders' precondition: mh_check only (as a truncated T2)
GBW_PICKS = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 66, 79, 80)
SALT = 31
DEFAULT_CASES = 40
PLANES = 2
_HEADERS: dict = {}
_CASES: dict = {}


def headers():
    """slice_helpers' five headers, the single-symbol code and a natural header with a quarter of its
    used lengths zeroed (Kraft sums below 1: asserted)."""
    if not _HEADERS:
        zoo = header_zoo()
        _HEADERS.update(SH.headers())
        _HEADERS["single"] = next(z for z in zoo if z.name == "1x1/b")
        _HEADERS["quarter"] = next(z for z in zoo if z.kind == "incomplete" and int((z.canon > 0).sum()) >= 16
                                   and z.longest >= 10)
        assert int((_HEADERS["single"].canon > 0).sum()) == 1 and _HEADERS["single"].longest == 1
        assert all(kraft_sum(_HEADERS[h].canon) < 65536 for h in INCOMPLETE)
        # 256 codes of 16 bits fill 256 of the 65536 windows: slice_helpers' 16x256 is incomplete too
        assert [h for h in _HEADERS if not complete(h)] == ["16x256", "single", "quarter"]
    return _HEADERS


def complete(header):
    """Kraft sum 1: every 16-bit window matches a code, so no stream has a zero-width lookup."""
    return kraft_sum(_HEADERS[header].canon) == 65536


def group_of(flavour):
    return next(g for g, fl in GROUPS.items() if flavour in fl)


@dataclasses.dataclass
class DefectFrame:
    header: str
    kind: str                 # the defect applied (a kind that does not fit the grid falls back, see _apply)
    ef: object                # EncodedFrame: codes = the SLOT's bytes (a multiple of 16), offsets as damaged
    tail: np.ndarray          # bytes that follow the slot in memory when nothing else does (the cut-off rest)
    damaged: np.ndarray       # bool[nb]: blocks whose code bits or offsets were touched
    ends: np.ndarray          # u64[nb]: the reference walk's end bit
    stalls: np.ndarray        # u32[nb]: its zero-width steps
    spec: np.ndarray          # bool[nb]
    report: np.ndarray        # u32[4]: oracle.check_frame over the slot (with the case's T2)
    want: object = None       # u8[H, W], None for a check-only frame
    care: object = None       # bool[H, W]: the pixels of specified blocks

    @property
    def clean(self):
        return self.kind == "none"


@dataclasses.dataclass
class DefectCase:
    entry: str
    i: int
    grid: tuple               # (grid W, grid H, declared W, declared H)
    flavour: str
    tables: str               # "shared" or "set"
    frames: list              # DefectFrame
    what: object = None       # run_contained's `what`; samples carry a flags word
    k: int = 0
    geom: str = "tight"
    norm: object = None       # (format, [(scale, bias)] per plane)
    t2_entries: int = 0       # check only: T2 truncated to this many entries (0: whole)

    @property
    def fmt(self):
        return FLAVOURS[self.flavour][1]

    def describe(self):
        gw, gh, W, H = self.grid
        fr = [(f.header, f.kind, f"{int(f.spec.sum())}/{f.spec.size} specified") for f in self.frames]
        return (f"defect_case({self.entry!r}, {self.i}): grid {gw // 8} x {gh // 8} blocks declared {W} x {H}, "
                f"{self.flavour}, tables {self.tables}, frames {fr}, what {self.what}, k {self.k}, geom {self.geom}, "
                f"norm {self.norm}, t2_entries {self.t2_entries}")

    def rect_blocks(self):
        """[(frame, bool[gbh, gbw] of the blocks the rectangle touches)] per rectangle or sample plane."""
        gw, gh, W, H = self.grid
        gbw, gbh = gw // 8, gh // 8
        out = []

        def blocks(x0, y0, w, h):
            m = np.zeros((gbh, gbw), bool)
            m[y0 // 8: (y0 + h + 7) // 8, x0 // 8: (x0 + w + 7) // 8] = True
            return m
        n = len(self.frames)
        if self.entry in DECODES + ("frames", "headers"):
            return [(f, np.ones((gbh, gbw), bool)) for f in range(n)]
        if self.entry in ("region", "region_scaled"):
            return [(f, blocks(*R.region_pixels(self.what, W, H))) for f in range(n)]
        rs, size = self.what
        for r in rs:
            if self.entry in ("windows", "windows_scaled"):
                out.append((r[0], blocks(*R.region_pixels((r[1], r[2], size[0], size[1]), W, H))))
            else:
                for c in range(PLANES if self.entry == "crops_norm_planes" else 1):
                    out.append((r[0] + c, blocks(r[1], r[2], size[0], size[1])))
        return out


def _ranges(ef):
    offs = ef.block_offsets.astype(np.int64)
    return offs, np.append(offs[1:], 8 * ef.payload_bytes)


def _pick_blocks(r, nb):
    """1..nb // 4 (at most 6) distinct blocks: steered to both sides of a tile boundary or to the frame's
    last block about half of the time."""
    k = int(r.integers(1, min(6, nb // 4) + 1))
    steer = r.random()
    fixed = []
    if steer < 0.3 and nb > 64 and k >= 2:
        fixed = [63, 64]
    elif steer < 0.55:
        fixed = [nb - 1]
    rest = [int(b) for b in r.permutation(nb) if int(b) not in fixed][: k - len(fixed)]
    return sorted(fixed + rest)


def _apply(r, kind, ef):
    """-> (kind applied, slot bytes, bytes behind the slot, offsets, damaged). A kind the grid has no room
    for (the caps of test_defect_cases.py: at least 3/4 of a damaged frame's blocks stay specified, so a
    per-block kind needs 4 blocks and an offset kind, which can cost two blocks, 8) falls back to `replace`
    or `flip`."""
    nb = ef.n_blocks
    payload = ef.payload_bytes
    offs, ends = _ranges(ef)
    codes = ef.codes.copy()
    damaged = np.zeros(nb, bool)
    cut = None
    if kind in CHECK_KINDS:
        new = offs.copy()
        if kind == "swap" and nb >= 2:
            a, b = sorted(int(v) for v in r.choice(nb, 2, replace=False))
            new[a], new[b] = offs[b], offs[a]
            damaged[[a, b]] = True
        else:
            kind, b = "past", int(r.integers(0, nb))
            new[b] = 8 * (-(-codes.size // 16) * 16) + int(r.integers(1, 5000))
            damaged[b] = True
        offs = new
    if kind not in ("none", "replace") + CHECK_KINDS and nb < 4:
        kind = "replace"
    if kind in ("move", "equal") and nb < 8:
        kind = "flip"
    if kind == "cut":
        lo = -(-int(-(-offs[-1] // 8)) // 16) * 16          # every offset stays <= 8 x slot
        choices = list(range(max(lo, 16), payload, 16))
        if choices:
            cut = int(r.choice(choices))
            damaged[-1] = True
        else:
            kind = "flip"
    if kind in ("flip", "ff", "seeded"):
        bits = np.unpackbits(codes[:payload])
        for b in _pick_blocks(r, nb):
            lo, hi = int(offs[b]), int(ends[b])
            if kind == "flip":
                at = r.integers(lo, hi, int(r.integers(1, 5)))
                bits[at] ^= 1
            elif kind == "ff":
                bits[lo:hi] = 1
            else:
                bits[lo:hi] = r.integers(0, 2, hi - lo, dtype=np.uint8)
            damaged[b] = True
        codes[:payload] = np.packbits(bits)
    elif kind == "replace":
        codes[:payload] = r.integers(0, 256, payload, dtype=np.uint8)
        damaged[:] = True
    elif kind == "move":
        b = int(r.integers(1, nb))
        d = int(r.integers(1, 41)) * (1 if r.random() < 0.5 else -1)
        offs = offs.copy()
        offs[b] = min(max(offs[b] + d, offs[b - 1]), ends[b])
        damaged[[b - 1, b]] = True
    elif kind == "equal":
        b = int(r.integers(0, nb - 1))
        offs = offs.copy()
        if r.random() < 0.5:
            offs[b + 1] = offs[b]
        else:
            offs[b] = offs[b + 1]
        damaged[[b, b + 1]] = True
    slot = np.zeros(-(-codes.size // 16) * 16, np.uint8)
    slot[: codes.size] = codes
    tail = np.zeros(0, np.uint8)
    if cut is not None:
        slot, tail = slot[:cut].copy(), slot[cut:].copy()
    return kind, slot, tail, offs.astype(np.uint32), damaged


def _reference(oracle, df, W, H, decode, t2_entries):
    """Fills in the walk, the specified mask, the report and (decode) the expected raster and its mask."""
    ef = df.ef
    t1, t2 = ef.tables()
    if t2_entries:
        t2 = t2[: 2 * t2_entries]
    slot, offs, nb = ef.codes, ef.block_offsets, ef.block_offsets.size
    df.ends, df.stalls = oracle.walk_frame(offs, slot, t1, t2)
    limit = np.append(offs[1:].astype(np.uint64), np.uint64(8 * slot.size))
    df.spec = df.ends <= limit
    df.report = oracle.check_frame(offs, slot, t1, t2)
    # the walk against orc_check_frame's totals: its words are sums over the same blocks
    miss = np.append(df.ends[:-1] != offs[1:].astype(np.uint64), df.ends[-1] > np.uint64(8 * slot.size))
    bad = np.flatnonzero((df.stalls > 0) | miss)
    assert int(df.report[0]) == int(df.stalls.sum()) and int(df.report[2]) == int(miss.sum())
    assert int(df.report[3]) == (int(bad[0]) if bad.size else 0xFFFFFFFF)
    if df.report.tolist() == [0, 0, 0, 0xFFFFFFFF]:
        assert df.spec.all(), "a frame the check reports clean is specified in full (contract point 3)"
    if decode:
        assert df.spec[~df.damaged].all(), "a block whose code bits and offsets are intact is specified"
        gbw = (W + 7) // 8
        padded = np.concatenate([slot, np.zeros(256, np.uint8)])     # zeros from the slot's end on
        df.want = oracle.decode_frame_shader(offs, padded, t1, t2, W, H, block_init=ef.block_init,
                                             delta=not (ef.flags & 1))
        df.care = np.kron(df.spec.reshape(-1, gbw), np.ones((8, 8), bool)).astype(bool)[:H, :W].copy()
        df.want.setflags(write=False)
        df.care.setflags(write=False)


def _about(r, at, size, total):
    """An origin in [0, total - size] of an extent that covers position `at`."""
    return int(min(max(at - int(r.integers(0, size)), 0), total - size))


def defect_case(mh, oracle, entry, i):
    """Case i of `entry` (cached; read-only)."""
    key = (entry, int(i))
    if key not in _CASES:
        _CASES[key] = _make(oracle, entry, int(i))
    return _CASES[key]


def _make(oracle, entry, i):
    e = ALL.index(entry)
    r = np.random.default_rng([e, i, SALT])
    gbw = GBW_PICKS[(i // 2 + 3 * e) % len(GBW_PICKS)] if i % 2 == 0 else int(r.integers(1, 81))
    gbh = int(r.integers(1, 7))
    W, H = 8 * gbw - int(r.integers(0, 8)), 8 * gbh - int(r.integers(0, 8))
    names = list(FLAVOURS)
    flavour = names[(i + 2 * e) % len(names)]
    header, fmt = FLAVOURS[flavour]
    n = int(r.integers(2, 6))
    tables = "shared" if entry in DECODES + (CHECK,) or r.random() < 0.5 else "set"
    kinds = DECODE_KINDS + (CHECK_KINDS if entry == CHECK else ())
    clean = int(r.integers(0, n))
    t2_entries = 512 if entry == CHECK and r.random() < 0.25 else 0
    frames = []
    # with the first delta outside the codes a zero symbol takes its place: the header must have one
    mixable = [h for h in headers() if fmt != "init_zero_delta" or headers()[h].canon[0]]
    for f in range(n):
        hd = str(r.choice(mixable)) if tables == "set" and f and r.random() < 0.5 else header
        # the first frame that is not the clean one walks the kinds in turn; the rest draw
        first = f == (1 if clean == 0 else 0)
        kind = "none" if f == clean else kinds[1 + (i + e) % (len(kinds) - 1)] if first else str(r.choice(kinds))
        ef, _ = frame_under_header(headers()[hd].canon, 8 * gbw, 8 * gbh, [gbw, gbh, names.index(flavour), f, i, e, 2027],
                                   no_delta=fmt == "no_delta", init_zero_delta=fmt == "init_zero_delta")
        kind, slot, tail, offs, damaged = _apply(np.random.default_rng([e, i, f, SALT + 1]), kind, ef)
        ef = dataclasses.replace(ef, width=W, height=H, codes=slot, block_offsets=offs)
        df = DefectFrame(hd, kind, ef, tail, damaged, None, None, None, None)
        _reference(oracle, df, W, H, entry != CHECK, t2_entries)
        frames.append(df)
    if entry == "frame":      # one frame per launch (run_case): the first damaged one, then the clean one
        frames = [next((f for f in frames if not f.clean), frames[0]), frames[clean]]
    case = DefectCase(entry, i, (8 * gbw, 8 * gbh, W, H), flavour, tables, frames, t2_entries=t2_entries)
    n = len(frames)
    case.k = int(r.integers(1, 4)) if entry in SH.SCALED else 0
    case.geom = "tight" if r.random() < 0.5 else "loose"
    cleans = [f for f in range(n) if frames[f].clean]
    dirty = [f for f in range(n) if not frames[f].clean]

    def hurt(f):   # (bx, by) of a damaged block of frame f
        b = int(r.choice(np.flatnonzero(frames[f].damaged)))
        return b % gbw, b // gbw
    one = r.random() < 0.2    # rectangles of one block: some lie wholly in damage
    if entry in ("region", "region_scaled"):
        bw, bh = (1, 1) if one else (SH._size(r, gbw), SH._size(r, gbh))
        if dirty and r.random() < 0.6:
            bx, by = hurt(dirty[0])
            case.what = (_about(r, bx, bw, gbw), _about(r, by, bh, gbh), bw, bh)
        else:
            case.what = (SH._axis(r, gbw, bw), SH._axis(r, gbh, bh), bw, bh)
    elif entry in ("windows", "windows_scaled"):
        bw, bh = (1, 1) if one else (SH._size(r, gbw), SH._size(r, gbh))
        rs = [(int(r.choice(cleans)), SH._axis(r, gbw, bw), SH._axis(r, gbh, bh))]
        for j in range(int(r.integers(1, 5))):
            f = int(r.choice(dirty)) if dirty and j == 0 else int(r.integers(0, n))
            if not frames[f].clean and r.random() < 0.75:
                bx, by = hurt(f)
                rs.append((f, _about(r, bx, bw, gbw), _about(r, by, bh, gbh)))
            else:
                rs.append((f, SH._axis(r, gbw, bw), SH._axis(r, gbh, bh)))
        case.what = (rs, (bw, bh))
    elif entry in ("crops",) + NORMS:
        planes = PLANES if entry == "crops_norm_planes" else 1
        if one:
            w, h = int(r.integers(1, min(8, W) + 1)), int(r.integers(1, min(8, H) + 1))
        else:
            w, h = SH._size(r, W), SH._size(r, H)
        if entry in NORMS and r.random() < 0.4 and W >= 8:
            w = max(8, w // 8 * 8)           # a width a mirrored crop may have
        flags = lambda: () if entry == "crops" else (NH.MIRROR if w % 8 == 0 and r.random() < 0.5 else 0,)
        last = n - planes                    # the last frame a sample may start at
        mixed = [f for f in range(last + 1) if len({frames[f + c].clean for c in range(planes)}) == planes]
        starts = mixed if planes > 1 and mixed else [f for f in cleans if f <= last] or [0]
        rs = [(int(r.choice(starts)), SH._axis(r, W, w), SH._axis(r, H, h)) + flags()]
        for j in range(int(r.integers(1, 5))):
            f = int(r.integers(0, last + 1))
            hurtable = [f + c for c in range(planes) if not frames[f + c].clean]
            if hurtable and r.random() < 0.75:
                bx, by = hurt(hurtable[0])
                if one:
                    x0 = min(8 * bx + int(r.integers(0, 8 - w + 1)), W - w)
                    y0 = min(8 * by + int(r.integers(0, 8 - h + 1)), H - h)
                else:
                    x0 = int(min(max(8 * bx + int(r.integers(-w + 1, 8)), 0), W - w))
                    y0 = int(min(max(8 * by + int(r.integers(-h + 1, 8)), 0), H - h))
                rs.append((f, x0, y0) + flags())
            else:
                rs.append((f, SH._axis(r, W, w), SH._axis(r, H, h)) + flags())
        case.what = (rs, (w, h))
        if entry in NORMS:
            if i % 2 == 0:
                case.norm = (NH.F32, [(1.0, 0.0)] * planes)
            else:
                pairs = NH.PAIRS + NH.random_pairs(16, seed=SALT)
                case.norm = (int(r.integers(0, 3)), [pairs[int(r.integers(0, len(pairs)))] for _ in range(planes)])
    return case


def sweep_range():
    """(first, count) of the default sweep, or of another asked for through the environment."""
    return int(os.environ.get("MH_DEFECT_SWEEP_FIRST", "0")), int(os.environ.get("MH_DEFECT_SWEEP_CASES",
                                                                                  str(DEFAULT_CASES)))


# ---- the device side ------------------------------------------------------------------------------------

def pack(device, dfs, W, H, force_offsets=False):
    """The frames' slots one behind the other -- a slot that was cut short is followed at once by the
    next frame's first byte, the last slot by its own cut-off rest -- as DeviceFrames. One frame goes
    without an offset array (unless force_offsets): codes_bytes is the slot, a view into the longer
    allocation."""
    import torch
    from metalhuffman_amd import decoder as D
    starts = [0]
    for df in dfs:
        assert df.ef.codes.size % 16 == 0
        starts.append(starts[-1] + df.ef.codes.size)
    whole = np.concatenate([df.ef.codes for df in dfs] + [dfs[-1].tail, np.zeros(16, np.uint8)])
    big = torch.from_numpy(whole).to(device)
    assert big.data_ptr() % 16 == 0
    codes = big[: starts[-1]]
    offs = np.concatenate([df.ef.block_offsets for df in dfs]).astype(np.uint32)
    ef0 = dfs[0].ef
    init = None
    if ef0.block_init is not None:
        init = torch.from_numpy(np.concatenate([df.ef.block_init for df in dfs])).to(device)
    fco = torch.tensor(starts, dtype=torch.int64, device=device) if len(dfs) > 1 or force_offsets else None
    fr = D.DeviceFrames(W, H, len(dfs), torch.from_numpy(offs.view(np.int32)).to(device), codes, fco, init,
                        ef0.flags, starts[-1])
    fr._whole = big
    return fr


def batch_frames(device, case):
    """The frames of a launch: the case's, cycled for decode_batch until the launch has more tiles than
    the small kernel takes (4 per compute unit)."""
    import torch
    dfs = list(case.frames)
    if case.entry == "decode_batch":
        _, _, W, H = case.grid
        tiles = -(-((W + 7) // 8) * ((H + 7) // 8) // 64)
        cus = torch.cuda.get_device_properties(device).multi_processor_count
        reps = -(-(4 * cus + 1) // (tiles * len(dfs)))
        dfs = dfs * reps
        assert tiles * len(dfs) > 4 * cus
    return dfs


def upload(device, case):
    """-> (slice_helpers.Uploaded, tables, the launch's DefectFrames)."""
    from metalhuffman_amd import decoder as D
    _, _, W, H = case.grid
    dfs = batch_frames(device, case)
    fr = pack(device, dfs, W, H)
    canons = np.stack([np.asarray(df.ef.canon, np.uint8) for df in dfs])
    if case.entry == "headers":
        tabs = None
    elif case.entry in DECODES + (CHECK,):
        t1, t2 = dfs[0].ef.tables()
        if case.t2_entries:
            t2 = t2[: 2 * case.t2_entries]
        tabs = D.DeviceTables.upload(t1, t2, device, prepare_lut=case.entry not in ("decode_tables", CHECK))
    elif case.tables == "shared" and case.entry != "frames":
        assert all(np.array_equal(c, canons[0]) for c in canons)
        t1, t2 = dfs[0].ef.tables()
        tabs = D.DeviceTables.upload(t1, t2, device)
    else:
        tabs = D.DeviceTableSet.from_canonical_headers(canons, device)
    return SH.Uploaded(fr, [df.want for df in dfs], canons), tabs, dfs


def _norm_geometry(geom, row, rows):
    pitch = row if geom == "tight" else row + 48
    stride = rows * pitch + (0 if geom == "tight" else 80)
    return pitch, stride, 4096 if geom == "tight" else 4096 + 16, 8 * pitch + 4096


def run_case(device, case):
    """One launch of the case's entry into a pattern-guarded buffer: every guard byte is compared, and
    every pixel of a specified block with the reference."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    if case.entry == "frame" and len(case.frames) > 1:     # the single-frame entry: a launch per frame
        for df in case.frames:
            run_case(device, dataclasses.replace(case, frames=[df]))
        return
    up, tabs, dfs = upload(device, case)
    cares = [df.care for df in dfs]
    entry, fr = case.entry, up.frames
    _, _, W, H = case.grid
    stream = torch.cuda.current_stream(device).cuda_stream
    if entry in SH.ENTRIES:
        return SH.run_contained(entry, device, case.geom, up, tabs, case.what, case.k, care=cares)
    if entry in DECODES:
        assert (fr.frame_code_offsets is None) == (entry == "frame")
        cols = (W + 7) // 8 * 8
        pitch, stride, lead = S.scaled_geometry(case.geom, cols, H, 8)
        st = D._frame_struct(fr, tabs)

        def launch(d_out):
            N.check(N.lib().mh_decode(ctypes.byref(st), d_out, pitch, stride, stream), "mh_decode")
        return SH.run_slots(device, cols, H, [(df.want, False) for df in dfs], (pitch, stride, lead, 8 * pitch + 4096),
                            launch, label=lambda p: f"{entry}, frame {p} ({dfs[p].kind})", cares=cares)
    # the two normalised entries: elements as bytes, bit patterns through norm_helpers.table_bits
    rs, (w, h) = case.what
    fmt, pairs = case.norm
    E, C = NH.ESIZE[fmt], len(pairs)
    T = [NH.table_bits(fmt, *p) for p in pairs]
    row = NH.up8(w) * E
    pitch, stride, lead, tail = _norm_geometry(case.geom, row, h)
    pics, masks = [], []
    for s in rs:
        for c in range(C):
            bits = NH.expected_crop(T[c], dfs[s[0] + c].want, s, (w, h))
            m = NH.expected_crop(np.arange(256) > 0, np.where(dfs[s[0] + c].care, 255, 0).astype(np.uint8), s, (w, h))
            pics.append((np.ascontiguousarray(bits).view(np.uint8).reshape(h, w * E), False))
            masks.append(np.repeat(m, E, axis=1))
    desc = torch.tensor([[int(v) for v in s] for s in rs], dtype=torch.int32, device=device)
    status = torch.full((len(rs),), 77, dtype=torch.int32, device=device)
    st, _ = D._frames_entry(fr)
    if isinstance(tabs, D.DeviceTables):
        luts, lstride, fstatus = tabs.lut.data_ptr(), 0, None
    else:
        luts, lstride, fstatus = tabs.luts.data_ptr(), tabs.stride, tabs.status.data_ptr()

    def launch(d_out):
        if entry == "crops_norm":
            rc = N.lib().mh_decode_crops_norm(ctypes.byref(st), desc.data_ptr(), len(rs), w, h, fmt, pairs[0][0],
                                              pairs[0][1], luts, lstride, fstatus, status.data_ptr(), d_out, pitch,
                                              stride, stream)
        else:
            arr = ctypes.c_float * C
            rc = N.lib().mh_decode_crops_norm_planes(ctypes.byref(st), desc.data_ptr(), len(rs), w, h, fmt, C, 1,
                                                     arr(*[p[0] for p in pairs]), arr(*[p[1] for p in pairs]), luts,
                                                     lstride, fstatus, status.data_ptr(), d_out, pitch, stride,
                                                     C * stride, stream)
        N.check(rc, "mh_decode_" + entry)
        torch.cuda.synchronize(device)
        return status
    return SH.run_slots(device, row, h, pics, (pitch, stride, lead, tail), launch,
                        label=lambda p: f"{entry}, sample {p // C} = {rs[p // C]} of {(w, h)}, plane {p % C}, byte columns",
                        cares=masks, align=(16, 0))


# ---- mh_check ---------------------------------------------------------------------------------------------

GUARD_WORDS = 8


def made_frame(oracle, header, gbw, gbh, seed, edit=None, t2_entries=0):
    """A frame of `header` on a gbw x gbh grid (declared whole) for mh_check, with its oracle report:
    edit(slot bytes, offsets, payload bytes), when given, damages the two arrays in place."""
    ef, _ = frame_under_header(headers()[header].canon, 8 * gbw, 8 * gbh, [gbw, gbh, seed, 2028])
    slot = np.zeros(-(-ef.codes.size // 16) * 16, np.uint8)
    slot[: ef.codes.size] = ef.codes
    offs = ef.block_offsets.copy()
    if edit is not None:
        edit(slot, offs, ef.payload_bytes)
    df = DefectFrame(header, "none" if edit is None else "edit", dataclasses.replace(ef, codes=slot, block_offsets=offs),
                     np.zeros(0, np.uint8), np.zeros(offs.size, bool), None, None, None, None)
    _reference(oracle, df, 8 * gbw, 8 * gbh, False, t2_entries)
    return df


def check_tables(device, df, t2_entries=0):
    from metalhuffman_amd import decoder as D
    t1, t2 = df.ef.tables()
    return D.DeviceTables.upload(t1, t2[: 2 * t2_entries] if t2_entries else t2, device, prepare_lut=False)


def gpu_check(device, fr, tabs, stream=None):
    """mh_check through the C ABI into a report that was dirty before the call -- every byte 0xA5 -- and
    lies between guard words, which must survive -> u32[n_frames, 4] on the host."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    n = fr.n_frames
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(device)):
        buf = torch.full(((2 * GUARD_WORDS + 4 * n) * 4,), 0xA5, dtype=torch.uint8, device=device)
    st = D._frame_struct(fr, tabs)
    sp = (stream if stream is not None else torch.cuda.current_stream(device)).cuda_stream
    N.check(N.lib().mh_check(ctypes.byref(st), buf.data_ptr() + 4 * GUARD_WORDS, sp), "mh_check")
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize(device)
    words = buf.cpu().numpy().view(np.uint32)
    guard = np.concatenate([words[:GUARD_WORDS], words[GUARD_WORDS + 4 * n:]])
    assert (guard == 0xA5A5A5A5).all(), "mh_check wrote outside its 4 words per frame"
    return words[GUARD_WORDS: GUARD_WORDS + 4 * n].reshape(n, 4).copy()


def assert_reports(got, dfs, what):
    want = np.stack([df.report for df in dfs])
    if not np.array_equal(got, want):
        f = int(np.flatnonzero((got != want).any(axis=1))[0])
        raise AssertionError(f"{what}: frame {f} reports {got[f].tolist()}, the oracle {want[f].tolist()}")
