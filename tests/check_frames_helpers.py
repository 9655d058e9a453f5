"""Helpers of the mh_check_frames / mh_check_headers tests (test_check_frame_cpu.py, test_check_frames_abi.py,
test_gpu_check_frames.py), on top of defect_helpers: which seeded cases the tests run, a few made frames,
and the two C entries called into report, verdict and header-status buffers that were 0xA5 before the call
and lie between guard words that must survive (the pattern of defect_helpers.gpu_check)."""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np

import defect_helpers as DH

CLEAN = [0, 0, 0, 0xFFFFFFFF]
N_CASES = 40
MH_ERR_STREAM = -9
DIRTY = np.int32(np.uint32(0xA5A5A5A5).view(np.int32))
_CASES: dict = {}


def cases(mh, oracle, entry):
    """Cases 0..39 of `entry`; of the check cases only those with a whole T2 (no prepared table and no
    header expresses a truncated one)."""
    if entry not in _CASES:
        every = [DH.defect_case(mh, oracle, entry, i) for i in range(N_CASES)]
        _CASES[entry] = [c for c in every if not c.t2_entries]
    return _CASES[entry]


def bad_header(canon, name):
    """`canon` as it is ("good"), with a length over 16 ("too_long": -3), with a Kraft sum over 1
    ("kraft": -5), or with both ("both": -3, the length is judged first)."""
    c = np.array(canon, np.uint8)
    used = np.flatnonzero(c)
    if name in ("kraft", "both"):
        c[:] = 1                      # 256 codes of one bit
    if name in ("too_long", "both"):
        c[used[0]] = 17
    assert name in ("good", "too_long", "kraft", "both")
    return c


def stall(*blocks):
    """made_frame's edit: under the single-symbol code ('0') a set bit at a block's start matches no code,
    so the block's 64 steps are zero width and it ends where it began."""
    def edit(slot, offs, payload):
        for b in blocks:
            bit = int(offs[b])
            slot[bit >> 3] |= 0x80 >> (bit & 7)
    return edit


def single_frames(oracle, gbw, gbh, n, hurt):
    """n single-symbol frames of gbw x gbh blocks; hurt = {frame: [blocks]} get a stall each."""
    return [DH.made_frame(oracle, "single", gbw, gbh, f, stall(*hurt[f]) if f in hurt else None) for f in range(n)]


def far_offset_frames(oracle):
    """Single-symbol frames of 9 x 2 blocks with one block offset at 0xFFFFFFFF, just past 8 x slot, and
    both: zero bits are codes, so those blocks walk on past the slot, 64 bits, without a stall."""
    out = []
    for where in ({5: 0xFFFFFFFF}, {17: None}, {0: 0xFFFFFFFF, 9: None}, {17: 0xFFFFFFFF}):
        def edit(slot, offs, payload, where=where):
            for b, v in where.items():
                offs[b] = 8 * slot.size + 3 if v is None else v
        df = DH.made_frame(oracle, "single", 9, 2, len(out), edit)
        assert int(df.report[0]) == 0 and int(df.report[2]) >= 1
        assert (df.ends[list(where)] == df.ef.block_offsets[list(where)].astype(np.uint64) + 64).all()
        out.append(df)
    return out


def cut_slot(oracle, df, nbytes, tail_value=0xFF):
    """`df` with its slot cut to nbytes (any number), `tail_value` bytes behind it, and its reference redone."""
    tail = np.full(df.ef.codes.size - nbytes + 16, tail_value, np.uint8)
    out = dataclasses.replace(df, ef=dataclasses.replace(df.ef, codes=df.ef.codes[:nbytes].copy()), tail=tail)
    gw = 8 * df.ef.block_width
    DH._reference(oracle, out, gw, 8 * df.ef.block_height, False, 0)
    return out


def pack_one(device, df):
    """One frame without an offset array whose slot may be any number of bytes: the slot, then df.tail,
    in one allocation; codes_bytes is the slot."""
    import torch
    from metalhuffman_amd import decoder as D
    whole = np.concatenate([df.ef.codes, df.tail, np.zeros(16, np.uint8)])
    big = torch.from_numpy(whole).to(device)
    assert big.data_ptr() % 16 == 0
    n = df.ef.codes.size
    offs = torch.from_numpy(df.ef.block_offsets.astype(np.uint32).view(np.int32)).to(device)
    fr = D.DeviceFrames(df.ef.width, df.ef.height, 1, offs, big[:n], None, None, df.ef.flags, n)
    fr._whole = big
    return fr


# ---- the device side --------------------------------------------------------------------------------------

G = DH.GUARD_WORDS


@dataclasses.dataclass
class Guarded:
    """report | verdict | header status, each between guard words, every byte 0xA5."""
    buf: object
    n: int

    def ptr(self, which):
        n = self.n
        word = {"report": G, "verdict": 2 * G + 4 * n, "header": 3 * G + 5 * n}[which]
        return self.buf.data_ptr() + 4 * word

    def read(self):
        """-> (report u32[n, 4], verdict i32[n], header status i32[n]); the guards are compared."""
        n = self.n
        w = self.buf.cpu().numpy().view(np.uint32)
        spans = [(G, 4 * n), (2 * G + 4 * n, n), (3 * G + 5 * n, n)]
        keep = np.zeros(w.size, bool)
        for a, k in spans:
            keep[a: a + k] = True
        assert (w[~keep] == 0xA5A5A5A5).all(), "a check entry wrote outside its report, verdict and header status"
        rep, ver, hdr = (w[a: a + k].copy() for a, k in spans)
        return rep.reshape(n, 4), ver.view(np.int32), hdr.view(np.int32)


def guarded(device, n):
    import torch
    return Guarded(torch.full(((4 * G + 6 * n) * 4,), 0xA5, dtype=torch.uint8, device=device), n)


def table_args(tabs):
    """(luts pointer, stride, the set's status tensor or None) of a DeviceTableSet or a DeviceTables (stride 0)."""
    from metalhuffman_amd import decoder as D
    if isinstance(tabs, D.DeviceTables):
        assert tabs.lut is not None
        return tabs.lut.data_ptr(), 0, None
    return tabs.luts.data_ptr(), tabs.stride, tabs.status


def check_frames(device, fr, tabs, status="own", verdict=True):
    """mh_check_frames through the C ABI -> (report, verdict or None). status: "own" (the table set's),
    None, or an int32 tensor."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    luts, stride, own = table_args(tabs)
    st = own if isinstance(status, str) else status
    g = guarded(device, fr.n_frames)
    frs, _ = D._frames_entry(fr)
    rc = N.lib().mh_check_frames(ctypes.byref(frs), luts, stride, st.data_ptr() if st is not None else None,
                                 g.ptr("report"), g.ptr("verdict") if verdict else None,
                                 torch.cuda.current_stream(device).cuda_stream)
    N.check(rc, "mh_check_frames")
    torch.cuda.synchronize(device)
    rep, ver, hdr = g.read()
    assert (hdr == DIRTY).all()
    if not verdict:
        assert (ver == DIRTY).all()
    return rep, ver if verdict else None


def check_headers(device, fr, canons, status=None, verdict=True, header_status=True):
    """mh_check_headers through the C ABI -> (report, verdict or None, header status or None)."""
    import torch
    from metalhuffman_amd import _native as N, decoder as D
    hdr_t = torch.from_numpy(np.ascontiguousarray(canons, np.uint8)).to(device)
    g = guarded(device, fr.n_frames)
    frs, _ = D._frames_entry(fr)
    rc = N.lib().mh_check_headers(ctypes.byref(frs), hdr_t.data_ptr(), status.data_ptr() if status is not None else None,
                                  g.ptr("header") if header_status else None, g.ptr("report"),
                                  g.ptr("verdict") if verdict else None, torch.cuda.current_stream(device).cuda_stream)
    N.check(rc, "mh_check_headers")
    torch.cuda.synchronize(device)
    rep, ver, hdr = g.read()
    if not verdict:
        assert (ver == DIRTY).all()
    if not header_status:
        assert (hdr == DIRTY).all()
    return rep, ver if verdict else None, hdr if header_status else None


def want_verdict(dfs):
    return [0 if df.report.tolist() == CLEAN else MH_ERR_STREAM for df in dfs]


def assert_checked(got, dfs, what):
    """Every frame's report equals the oracle's, and verdict == (report != clean)."""
    rep, ver = got[0], got[1]
    DH.assert_reports(rep, dfs, what)
    if ver is not None:
        assert ver.tolist() == want_verdict(dfs), (what, ver.tolist(), want_verdict(dfs))


def canons_of(dfs):
    return np.stack([np.asarray(df.ef.canon, np.uint8) for df in dfs])


def shape(mh, fr, headers=False):
    """(workgroups per frame, waves per workgroup) of the walk's launch."""
    from metalhuffman_amd import _native as N, decoder as D
    frs, _ = D._frames_entry(fr)
    g, w = ctypes.c_uint32(0), ctypes.c_uint32(0)
    entry = N.lib().mh_check_headers_shape if headers else N.lib().mh_check_frames_shape
    N.check(entry(ctypes.byref(frs), None, ctypes.byref(g), ctypes.byref(w)), "shape")
    return int(g.value), int(w.value)
