"""A raw-ABI driver for mh_encode_set_device_async (test_gpu_encode_set.py), in the style of
encode_helpers.py: every frame's pixels in an allocation of its own inside seeded garbage, every
output at a 256-byte boundary inside a guard-filled tensor, and the host codec (mh.encode_frame),
frame by frame, as the standard; never another GPU encode."""
from __future__ import annotations

import ctypes
import dataclasses

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


def run(mh, device, imgs, srcs, *, flags=0, init_zero=False, caps=None, workspace=None, ws_fill=0x5C):
    """One call -> SetRun. The workspace (any content: filled with ws_fill when made here) may be
    handed on to a second call."""
    import torch
    sizes = [(im.shape[1], im.shape[0]) for im in imgs]
    caps = [roomy_cap(w, h) for w, h in sizes] if caps is None else list(caps)
    plan = mh.encode_set_plan([(s.pixels, s.pitch, s.ps, w, h, c) for s, (w, h), c in zip(srcs, sizes, caps)], flags)
    t = plan.totals
    n = len(imgs)
    nbs = [EH.blocks(w, h)[0] * EH.blocks(w, h)[1] for w, h in sizes]
    assert t.total_blocks == sum(nbs) and t.codes_bytes == sum(caps)
    if workspace is None:
        workspace = torch.full((int(t.workspace_bytes) + 256,), ws_fill, dtype=torch.uint8, device=device)
    wsp = (workspace.data_ptr() + 255) // 256 * 256
    wsb = workspace.numel() - (wsp - workspace.data_ptr())
    plan_dev = torch.from_numpy(plan.plan).to(device)
    o = dict(codes=EH._Out(device, int(t.codes_bytes), 0, FILL_BYTES),
             offs=EH._Out(device, 4 * int(t.total_blocks), 0, FILL_U32),
             canon=EH._Out(device, 256 * n, 0, FILL_BYTES),
             lens=EH._Out(device, 8 * n, 0, FILL_U64),
             fco=EH._Out(device, 8 * (n + 1), 0, FILL_U64),
             st=EH._Out(device, 4 * n, 0, FILL_STATUS))
    if init_zero:
        o["init"] = EH._Out(device, int(t.total_blocks), 0, FILL_BYTES)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    rc = mh.lib().mh_encode_set_device_async(
        plan_dev.data_ptr(), ctypes.byref(t), flags, o["canon"].ptr, o["codes"].ptr, int(t.codes_bytes), o["lens"].ptr,
        o["fco"].ptr, o["offs"].ptr, o["init"].ptr if init_zero else None, o["st"].ptr, wsp, wsb, stream)
    torch.cuda.synchronize(device)
    host = {k: v.host(f"set: {k}") for k, v in o.items()}
    return SetRun(int(rc), plan, caps, nbs, flags, init_zero, host, o, plan_dev), workspace


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


def check(r, exp):
    """One call's outputs against the host codec, frame by frame."""
    assert r.rc == OK, r.rc
    assert len(exp) == len(r.caps)
    lens, st = r.host["lens"].view(np.uint64), r.host["st"].view(np.int32)
    want_fco = np.concatenate([[0], np.cumsum(r.caps)]).astype(np.uint64)
    assert np.array_equal(r.host["fco"].view(np.uint64), want_fco), "d_frame_code_offsets"
    assert [int(s) for s in st] == [s for s, _ in exp], ([int(s) for s in st], [s for s, _ in exp])
    for f, (status, ef) in enumerate(exp):
        got = r.codes(f)
        if status != OK:
            assert int(lens[f]) == 0, f
            assert (got == FILL_BYTES).all(), f"rejected frame {f}: code bytes written"
            assert (r.offsets(f) == 0x3C3C3C3C).all(), f"rejected frame {f}: offsets written"
            continue                # its d_block_init entries and its header: unspecified
        k = ef.codes.size
        assert int(lens[f]) == k, (f, int(lens[f]), k)
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
