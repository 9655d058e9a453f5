"""The two stream front ends (mh_stream_* in csrc/mh_stream.cpp and csrc/mh_stream_headers.cpp) and
the stream groups through the raw ABI (stream_helpers.Driver), as named cases at the smallest
geometries that reach the code: host buffers in slot layout and apart, pinned and pageable, frames
of different code lengths under one header (a short frame in front of a dense frame's stale bytes),
graph replays and direct launches, with and without a prepared table, delta / no delta / init
bytes, caller rasters at byte offset 8 inside guarded tensors and the stream's own, back-to-back
submits with a consumer on the slot's stream, groups with init bytes, header verdicts under load,
destroy with frames in flight, the capacity edges and what creation stores.

Every result is compared over its whole round_up(W, 8) x H bytes with a direct mh_decode /
mh_decode_headers call, in its columns < W with the image, and for one frame per test with the
oracle's shader decode of the frame's own bytes."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import stream_helpers as SH
from helpers import image_from_block_deltas, kraft_sum

pytestmark = pytest.mark.gpu

_SETS = {}


def _frames(mh, mode, w, h, n, fmt="delta", seed=0):
    key = (mode, w, h, n, fmt, seed)
    if key not in _SETS:
        _SETS[key] = SH.frame_set(mh, mode, w, h, n, fmt, seed)
    return _SETS[key]


LAYOUTS = pytest.mark.parametrize("packed", [True, False], ids=["one_buffer", "separate_buffers"])
BOTH_MODES = pytest.mark.parametrize("mode", SH.MODES)


# ---- geometry -------------------------------------------------------------------------------------

@BOTH_MODES
@LAYOUTS
@pytest.mark.parametrize("w,h", [(8, 8), (24, 8), (40, 24), (520, 264)])
def test_tiny_geometries(mh, oracle, device, mode, packed, w, h):
    """8 x 8: one block, 16 bytes of offsets against 4 used; 24 x 8 and 40 x 24 (15 blocks): 4 * NB
    off the 16-byte grid; 520 x 264: 2145 blocks, 4 * NB % 16 == 4."""
    nb = SH.n_blocks(w, h)
    assert {(8, 8): 1, (24, 8): 3, (40, 24): 15, (520, 264): 2145}[w, h] == nb and 4 * nb % 16 != 0
    fs = _frames(mh, mode, w, h, 5)
    d = SH.run_checked(mh, oracle, device, fs, SH.slot_order(fs.sizes, 2), slots=2, packed=packed)
    assert d.off_bytes == SH.r16(4 * nb) > 4 * nb


@BOTH_MODES
@LAYOUTS
def test_own_rasters_at_a_width_off_the_8_pixel_grid(mh, oracle, device, mode, packed):
    """1001 x 777 into the stream's own rasters: mh_stream_output's pitch is 1008 (asserted by the
    driver for every slot), and all 1008 x 777 bytes are compared."""
    fs = _frames(mh, mode, 1001, 777, 3)
    d = SH.run_checked(mh, oracle, device, fs, SH.slot_order(fs.sizes, 2), slots=2, packed=packed, owned=True)
    assert d.pitch == 1008 and d.out_bytes == 1008 * 777


# ---- lengths --------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,packed", [("table", True), ("table", False), ("headers", False)],
                         ids=["table-one_buffer", "table-separate_buffers", "headers-separate_buffers"])
@pytest.mark.parametrize("slots", [2, 3])
@pytest.mark.parametrize("w,h", [(40, 24), (264, 64)])
def test_short_frames_in_front_of_stale_bytes(mh, oracle, device, mode, packed, slots, w, h):
    """Every slot takes its longest frame first (frame 0, dense noise, goes to slot 0) and its
    shortest next, then the rest. The slot's decode is told codes_bytes = capacity, so only the short
    frame's own MH_CODES_PAD zero bytes stand between its last block and the long frame's bytes."""
    fs = _frames(mh, mode, w, h, 2 * slots + 2, seed=3)
    order = SH.slot_order(fs.sizes, slots)
    assert SH.second_under_half(fs.sizes, order, slots) and fs.sizes[order[slots]] == min(fs.sizes)
    assert len(set(fs.sizes)) >= 4
    SH.run_checked(mh, oracle, device, fs, order, slots=slots, packed=packed)


# ---- modes ----------------------------------------------------------------------------------------

@LAYOUTS
@pytest.mark.parametrize("fmt", SH.FORMATS)
@pytest.mark.parametrize("prepared", [True, False], ids=["prepared", "no_lut"])
@pytest.mark.parametrize("graphs", [None, False], ids=["graph_replay", "direct"])
def test_table_mode_launch_kinds_and_formats(mh, oracle, device, graphs, prepared, fmt, packed):
    """{graph replay (the default), MH_STREAM_GRAPHS=0} x {prepared table, d_lut == NULL} x {delta,
    MH_FLAG_NO_DELTA, init bytes}; separate buffers with init bytes are three copies a submit."""
    fs = _frames(mh, "table", 72, 24, 5, fmt, seed=5)
    SH.run_checked(mh, oracle, device, fs, SH.slot_order(fs.sizes, 2), slots=2, packed=packed, prepared=prepared,
                   graphs=graphs)


@LAYOUTS
@pytest.mark.parametrize("fmt", SH.FORMATS)
@pytest.mark.parametrize("graphs", [None, True], ids=["direct", "graph_replay"])
def test_header_mode_launch_kinds_and_formats(mh, oracle, device, graphs, fmt, packed):
    """{direct (the default), MH_STREAM_GRAPHS=1} x the three formats; separate buffers with init
    bytes are four copies a submit."""
    fs = _frames(mh, "headers", 72, 24, 5, fmt, seed=5)
    SH.run_checked(mh, oracle, device, fs, SH.slot_order(fs.sizes, 2), slots=2, packed=packed, graphs=graphs)


@BOTH_MODES
def test_the_variable_is_read_at_every_create(mh, oracle, device, monkeypatch, mode):
    """monkeypatch.setenv in-process, the driver leaving the environment alone: streams made one
    after the other under MH_STREAM_GRAPHS=0, =1 and without it are all exact."""
    fs = _frames(mh, mode, 72, 24, 5, "delta", seed=5)
    for value in ("0", "1", None, "0"):
        if value is None:
            monkeypatch.delenv(SH.ENV, raising=False)
        else:
            monkeypatch.setenv(SH.ENV, value)
        SH.run_checked(mh, oracle, device, fs, [0, 1, 2, 3, 4], slots=2, graphs="env")


# ---- pageable host memory --------------------------------------------------------------------------

@BOTH_MODES
@LAYOUTS
@pytest.mark.parametrize("fmt", ["delta", "init"])
def test_pageable_host_memory(mh, oracle, device, mode, packed, fmt):
    """Host buffers from the ordinary allocator, one per submit, left alone until the stream is
    synchronised."""
    fs = _frames(mh, mode, 136, 40, 6, fmt, seed=7)
    SH.run_checked(mh, oracle, device, fs, SH.slot_order(fs.sizes, 2), slots=2, packed=packed, pinned=False)


# ---- queued load -----------------------------------------------------------------------------------

@BOTH_MODES
@pytest.mark.parametrize("slots", [1, 2, 3, 64])
def test_back_to_back_submits_are_all_checked(mh, oracle, device, mode, slots):
    """4 * slots + 1 submits of frames of different lengths with the consumer's copy behind each
    and no host wait; slot numbers are i % slots (the driver asserts each); every result is checked
    afterwards."""
    fs = _frames(mh, mode, 40, 24, 9, seed=9)
    assert len(set(fs.sizes)) >= 5
    order = SH.slot_order(fs.sizes, min(slots, 4))
    seq = [order[k % 9] for k in range(4 * slots + 1)]
    d = SH.run_checked(mh, oracle, device, fs, seq, slots=slots, packed=slots % 2 == 1)
    assert [s.slot for s in d.subs] == [k % slots for k in range(4 * slots + 1)]


@pytest.mark.parametrize("fmt", ["delta", "init"])
@pytest.mark.parametrize("members", [[0], [0, 0, 0]], ids=["one_member", "three_members"])
def test_group_back_to_back_through_the_raw_abi(mh, oracle, device, members, fmt):
    """mh_stream_group_submit with and without h_block_init: submit k goes to member k % n, slot
    (k // n) % slots (the driver asserts each), 4 * slots * n + 1 submits back to back."""
    fs = _frames(mh, "table", 40, 24, 9, fmt, seed=9)
    n, slots = len(members), 2
    order = SH.slot_order(fs.sizes, slots)
    seq = [order[k % 9] for k in range(4 * slots * n + 1)]
    d = SH.run_checked(mh, oracle, device, fs, seq, slots=slots, members=members, packed=fmt == "init")
    assert [(s.member, s.slot) for s in d.subs] == [(k % n, (k // n) % slots) for k in range(len(seq))]


def test_group_init_rule_and_flag_rule(mh, device):
    """A group made without init bytes refuses a submit that brings them and the reverse
    (MH_ERR_INVALID_ARG, nothing queued, the member rotation where it was); a group reports a refused
    flag through its member's create."""
    import torch
    from metalhuffman_amd import _native as N
    for fmt in ("delta", "init"):
        fs = _frames(mh, "table", 40, 24, 9, fmt, seed=9)
        d = SH.Driver(mh, device, fs, slots=2, members=[0, 0])
        assert d.submit(0) == (0, 0)
        h = torch.zeros(4096, dtype=torch.uint8).pin_memory()
        m, s = ctypes.c_uint32(7), ctypes.c_uint32(7)
        wrong_init = None if fmt == "init" else h.data_ptr() + 2048
        assert d.L.mh_stream_group_submit(d._g, h.data_ptr() + 1024, 64, h.data_ptr(), wrong_init, ctypes.byref(m),
                                          ctypes.byref(s)) == SH.INVALID
        assert (m.value, s.value) == (7, 7)
        assert d.submit(1) == (1, 0)
        d.finish()
    fs = _frames(mh, "table", 40, 24, 9, "delta", seed=9)
    d = SH.Driver(mh, device, fs, slots=2)                    # for its tables
    proto = N.mh_frame()
    t = d.tables[0]
    proto.d_table1, proto.d_table2, proto.table2_entries = t.table1.data_ptr(), t.table2.data_ptr(), t.table2_entries
    proto.dims, proto.n_frames = N.mh_dims(40, 24, 5, 3), 1
    devs = (ctypes.c_int * 1)(0)
    for flags in (0x2, 0x4, 0x5, 0x100, 0x200):
        proto.flags = flags
        g = ctypes.c_void_p(0x77)
        assert d.L.mh_stream_group_create(ctypes.byref(proto), 1, devs, 4096, 2, ctypes.byref(g)) == SH.INVALID
        assert not g.value
    d.close()


# ---- the Python group wrapper ------------------------------------------------------------------------

def test_frame_stream_group_carries_init_bytes(mh, device):
    """FrameStreamGroup(block_init=True).submit(codes, offsets, init): the C ABI's h_block_init is
    reachable from Python."""
    import torch
    from metalhuffman_amd import decoder as D
    from metalhuffman_amd.stream import FrameStreamGroup, pinned_frame
    fs = _frames(mh, "table", 40, 24, 9, "init", seed=9)
    t1, t2 = fs.efs[0].tables()
    tabs = [D.DeviceTables.upload(t1, t2, device) for _ in range(2)]
    g = FrameStreamGroup(tabs, 40, 24, max(fs.sizes), slots=2, block_init=True)
    hosts = [pinned_frame(ef) + (torch.from_numpy(ef.block_init).pin_memory(),) for ef in fs.efs]
    where = [g.submit(c, o, i) for c, o, i in hosts]
    assert where == [(k % 2, (k // 2) % 2) for k in range(9)]
    g.synchronize()
    for k in range(5, 9):                                     # the last frame of every (member, slot)
        m, s = where[k]
        assert np.array_equal(g.output(m, s)[:, :40].cpu().numpy(), fs.imgs[k]), k
    with pytest.raises(mh.MHError):
        g.submit(hosts[0][0], hosts[0][1])
    g.close()


# ---- header mode: verdicts under load ----------------------------------------------------------------

def _verdict_frames(mh):
    """64 x 40: three ordinary frames, a one-symbol frame (an incomplete code) and a frame of exactly
    uniform deltas (the flat 8-bit code), with a Kraft-sum-over-1 and a length-17 header."""
    w, h = 64, 40
    imgs = [SH.image(k, w, h, 21) for k in ("walk", "sparse", "mid")]
    imgs.append(np.zeros((h, w), np.uint8))
    deltas = np.tile(np.arange(256, dtype=np.uint8), SH.n_blocks(w, h) * 64 // 256)
    np.random.default_rng(4).shuffle(deltas)
    imgs.append(image_from_block_deltas(deltas, w, h))
    efs = [mh.encode_frame(im, limit_lengths=True) for im in imgs]
    assert int((efs[3].canon > 0).sum()) == 1 and kraft_sum(efs[3].canon) < 65536
    assert (efs[4].canon == 8).all()
    canon = efs[0].canon
    assert kraft_sum(canon) == 65536
    over = canon.copy()
    over[np.flatnonzero(canon > 1)[0]] -= 1
    assert kraft_sum(over) > 65536 and over.max() <= 16
    long17 = canon.copy()
    long17[np.flatnonzero(canon == 0)[0] if (canon == 0).any() else 0] = 17
    return SH.FrameSet("headers", "delta", w, h, imgs, efs), bytes(over), bytes(long17)


@LAYOUTS
def test_header_verdicts_under_load(mh, oracle, device, packed):
    """Rejected headers (-5, -3), a one-symbol header and the flat 8-bit code among valid frames,
    back to back through 3 slots. Every slot_status is read after later submits to OTHER slots; a
    rejected frame's raster, pad columns included, keeps its previous content byte for byte -- the
    creation's pattern for a slot's first frame."""
    fs, over, long17 = _verdict_frames(mh)
    d = SH.Driver(mh, device, fs, slots=3, packed=packed)
    d.submit(0, header=over)            # 0 -> slot 0: rejected, the pattern stays
    d.submit(1)                         # 1 -> slot 1
    assert d.status(0) == SH.TABLE
    d.submit(2)                         # 2 -> slot 2
    d.submit(0)                         # 3 -> slot 0
    d.submit(1, header=long17)          # 4 -> slot 1: rejected, frame 1 stays
    d.submit(3)                         # 5 -> slot 2: one symbol
    assert d.status(1) == SH.TOO_LONG
    d.submit(2, header=over)            # 6 -> slot 0: rejected, frame 0 stays
    d.submit(4)                         # 7 -> slot 1: flat 8-bit
    assert d.status(0) == SH.TABLE and d.status(2) == SH.OK
    d.submit(0)                         # 8 -> slot 2
    assert d.status(1) == SH.OK
    d.finish(oracle, oracle_subs=(5, 7), verdicts={0: SH.TABLE, 4: SH.TOO_LONG, 6: SH.TABLE})
    assert [s.verdict for s in d.subs] == [SH.TABLE, 0, 0, 0, SH.TOO_LONG, 0, SH.TABLE, 0, 0]


# ---- destroy in flight -------------------------------------------------------------------------------

@BOTH_MODES
@pytest.mark.parametrize("slots", [2, 3])
def test_destroy_with_frames_in_flight(mh, device, mode, slots):
    """2 * slots submits into caller rasters and mh_stream_destroy at once: MH_OK, the rasters hold
    the last `slots` frames, every guard byte is intact."""
    fs = _frames(mh, mode, 520, 264, 5, seed=11)
    d = SH.Driver(mh, device, fs, slots=slots, consume=False)
    for k in range(2 * slots):
        d.submit(k % 5)
    d.close()
    d.check()
    for s in range(slots):
        got = d.rasters[s].host(f"slot {s}").reshape(264, 520)
        assert np.array_equal(got, fs.imgs[(slots + s) % 5]), s


# ---- capacity ----------------------------------------------------------------------------------------

@BOTH_MODES
def test_capacity_edges(mh, oracle, device, mode):
    """A codes_capacity that is no multiple of 16: a frame of exactly that many bytes decodes; 3 bytes
    and round_up(capacity, 16) + 1 are MH_ERR_CAPACITY and leave the slot rotation where it was (the
    driver asserts the next slot); every length in between is accepted (include/metalhuffman.h)."""
    fs = _frames(mh, mode, 40, 24, 3, seed=13)
    longest = int(np.argmax(fs.sizes))
    cap = max(fs.sizes) + (1 if (max(fs.sizes) + 1) % 16 else 2)
    top = SH.r16(cap)
    assert cap % 16 != 0 and top - cap >= 1
    d = SH.Driver(mh, device, fs, slots=2, cap=cap, reserve=32)
    d.submit(longest, extend=cap)
    d.submit(1, codes_bytes=3, expect=SH.CAPACITY)
    d.submit(longest, extend=top + 1, expect=SH.CAPACITY)
    d.submit(1, codes_bytes=0, expect=SH.CAPACITY)
    for n in range(cap + 1, top + 1):
        d.submit(longest, extend=n)
    d.submit(1, extend=top + 16, codes_bytes=top + 16, expect=SH.CAPACITY)
    d.submit(2)
    d.finish(oracle)
    assert d.accepted == 2 + top - cap


# ---- creation ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(24, 8), (520, 264), (1001, 77)])
def test_creation_stores_inside_the_rasters_only(mh, device, w, h):
    """Table-mode creation decodes zeroed slot buffers once per slot (the warm-up; once more under
    the capture, which does not run): it stores into the caller's rasters, and only inside their
    round_up(W, 8) x H bytes. Header-mode creation stores nothing. Both are asserted by the driver
    after creation; here also that table mode does store, and the same for direct launches."""
    for graphs in (None, False):
        fs = _frames(mh, "table", w, h, 2, seed=15)
        d = SH.Driver(mh, device, fs, slots=3, graphs=graphs)
        for s, r in enumerate(d.rasters):
            assert not np.array_equal(d.cur[0, s], r.pattern[r.start: r.start + r.size]), s
        d.finish()
    for graphs in (None, True):
        d = SH.Driver(mh, device, _frames(mh, "headers", w, h, 2, seed=15), slots=3, graphs=graphs)
        d.finish()
