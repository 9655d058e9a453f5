"""The C-ABI of the set encoder (include/metalhuffman.h: mh_set_source, mh_set_frame, mh_set_totals,
mh_encode_set_plan_bytes, mh_encode_set_plan, mh_encode_set_device_async). CPU only: every host
check of the entry is made before any HIP call, with fake pointers; each case fails one check, the
cases that probe the ORDER fail two and expect the earlier one's code, and a case that must PASS a
rule is stopped by a workspace of 0 bytes, the last check of all."""
from __future__ import annotations

import copy
import ctypes

import pytest

OK, INVALID, DIMS, CAPACITY, ALIGN = 0, -1, -2, -4, -6
PLAN, CANON, CODES, LENS, FCO, OFFS, INIT, STATUS, WS = (
    0x10000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 0x90000, 0x100000)
SOURCES = [(0x7000_0000, 64, 1, 64, 48, 8192), (0x7100_0000, 300, 3, 100, 9, 4096), (0x7200_0000, 8, 1, 8, 8, 144)]


def _totals(mh):
    return mh.encode_set_plan(SOURCES).totals


def _call(mh, **kw):
    """The entry with one or two arguments (or fields of the totals) replaced."""
    t = copy.copy(_totals(mh))
    a = dict(plan=PLAN, totals=t, flags=0, canon=CANON, codes=CODES, codes_bytes=None, lens=LENS, fco=FCO, offs=OFFS,
             init=None, status=STATUS, ws=WS, ws_bytes=None)
    for k in list(kw):
        if hasattr(t, k) and k not in a:
            setattr(t, k, kw.pop(k))
    a.update(kw)
    if a["codes_bytes"] is None:
        a["codes_bytes"] = t.codes_bytes
    if a["ws_bytes"] is None:
        a["ws_bytes"] = t.workspace_bytes
    tp = ctypes.byref(a["totals"]) if a["totals"] is not None else None
    return mh.lib().mh_encode_set_device_async(a["plan"], tp, a["flags"], a["canon"], a["codes"], a["codes_bytes"],
                                               a["lens"], a["fco"], a["offs"], a["init"], a["status"], a["ws"],
                                               a["ws_bytes"], None)


def test_symbols_exported(mh):
    lib = ctypes.CDLL(mh.LIB_PATH)
    for name in ("mh_encode_set_plan_bytes", "mh_encode_set_plan", "mh_encode_set_device_async"):
        assert hasattr(lib, name), name
        assert name in mh.EXPORTS, name
    assert callable(mh.encode_set_plan)
    from metalhuffman_amd import encoder
    assert callable(encoder.encode_set_async) and callable(encoder.encode_image_set_async)
    assert hasattr(encoder, "AsyncEncodedSet")


def test_structs_are_the_headers():
    from metalhuffman_amd import _native as N

    def offsets(S):
        return [(f, getattr(S, f).offset) for f, _ in S._fields_]

    assert ctypes.sizeof(N.mh_set_source) == 40
    assert offsets(N.mh_set_source) == [("pixels", 0), ("row_pitch", 8), ("pixel_stride", 16), ("width", 20),
                                        ("height", 24), ("reserved", 28), ("codes_cap", 32)]
    assert ctypes.sizeof(N.mh_set_frame) == 64
    assert offsets(N.mh_set_frame) == [("pixels", 0), ("slot_offset", 8), ("codes_cap", 16), ("row_pitch", 24),
                                       ("pixel_stride", 28), ("width", 32), ("height", 36), ("block_width", 40),
                                       ("n_blocks", 44), ("n_tiles", 48), ("first_tile", 52), ("first_block", 56),
                                       ("reserved", 60)]
    assert ctypes.sizeof(N.mh_set_totals) == 80
    assert offsets(N.mh_set_totals) == [("codes_bytes", 0), ("workspace_bytes", 8), ("plan_bytes", 16),
                                        ("geoms_offset", 24), ("split_map_offset", 32), ("pack_map_offset", 40),
                                        ("n_frames", 48), ("total_blocks", 52), ("total_tiles", 56), ("split_grid", 60),
                                        ("pack_grid", 64), ("max_width", 68), ("max_height", 72), ("fetch_mode", 76)]
    assert ctypes.sizeof(N.mh_frame_geom) == 16
    assert (N.MH_SET_TILE_BLOCKS, N.MH_SET_PACK_TILES, N.MH_SET_FETCH_BYTES) == (256, 4, 255)


def test_header_declares_the_set_encoder():
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "metalhuffman.h")) as f:
        text = f.read()
    for name in ("mh_set_source", "mh_set_frame", "mh_set_totals", "mh_encode_set_plan_bytes", "mh_encode_set_plan",
                 "mh_encode_set_device_async", "MH_SET_TILE_BLOCKS 256u", "MH_SET_PACK_TILES 4u"):
        assert name in text, name
    frame_set = text[text.index("Crops from a SET of frames"): text.index("} mh_frame_geom;")]
    assert "a set encoder" not in frame_set
    for left in ("a shared table over a set", "mh_check_frames over a set", "compaction of the code"):
        assert left in " ".join(text.split()).replace("*/ /* ", ""), left


SINGLE = [
    (dict(plan=None), INVALID), (dict(totals=None), INVALID), (dict(canon=None), INVALID), (dict(codes=None), INVALID),
    (dict(fco=None), INVALID), (dict(offs=None), INVALID), (dict(ws=None), INVALID),
    (dict(n_frames=0), INVALID), (dict(total_tiles=0, split_grid=0), INVALID), (dict(total_blocks=0), INVALID),
    (dict(flags=0x40), INVALID), (dict(flags=0x2), INVALID), (dict(flags=0x400), INVALID),
    (dict(fetch_mode=0), INVALID), (dict(fetch_mode=5), INVALID), (dict(fetch_mode=256), INVALID),
    (dict(max_width=0), DIMS), (dict(max_height=0), DIMS), (dict(max_width=65536), DIMS), (dict(max_height=65536), DIMS),
    (dict(codes=CODES + 4), ALIGN), (dict(plan=PLAN + 8), ALIGN), (dict(ws=WS + 128), ALIGN),
    (dict(codes_bytes=8192 + 4096 + 144 - 1), CAPACITY),
    (dict(n_frames=0x80000000), CAPACITY), (dict(total_tiles=0x80000000, split_grid=0x80000000), CAPACITY),
    (dict(split_grid=1), CAPACITY), (dict(pack_grid=0), CAPACITY), (dict(pack_grid=1000), CAPACITY),
    (dict(ws_bytes=0), CAPACITY),
]


@pytest.mark.parametrize("kw,status", SINGLE)
def test_each_check(mh, kw, status):
    assert _call(mh, **kw) == status


def test_workspace_is_the_planners(mh):
    t = _totals(mh)
    assert t.codes_bytes == 8192 + 4096 + 144
    assert _call(mh, ws_bytes=t.workspace_bytes - 1) == CAPACITY
    # a caller that edits the totals' workspace figure down does not shrink the kernels' carve
    assert _call(mh, workspace_bytes=256, ws_bytes=256) == CAPACITY


ORDER = [
    (dict(plan=None, flags=0x40, max_width=0, codes=CODES + 4, ws_bytes=0), INVALID),
    (dict(fco=None, max_width=0), INVALID),
    (dict(flags=0x40, max_width=0, codes=CODES + 4, ws_bytes=0), INVALID),
    (dict(fetch_mode=7, max_height=0), INVALID),
    (dict(max_width=0, plan=PLAN + 4, ws_bytes=0), DIMS),
    (dict(max_height=70000, codes_bytes=0), DIMS),
    (dict(plan=PLAN + 4, codes_bytes=0), ALIGN),
    (dict(ws=WS + 16, ws_bytes=0), ALIGN),
    (dict(codes_bytes=0, ws_bytes=0), CAPACITY),
]


@pytest.mark.parametrize("kw,status", ORDER)
def test_check_order(mh, kw, status):
    assert _call(mh, **kw) == status


@pytest.mark.parametrize("kw", [dict(flags=0x1), dict(flags=0x100), dict(flags=0x200), dict(flags=0x301),
                                dict(lens=None), dict(status=None), dict(init=INIT), dict(fetch_mode=3),
                                dict(fetch_mode=255), dict(codes_bytes=1 << 40)])
def test_accepted_up_to_the_workspace(mh, kw):
    """Optional outputs, every flag and every fetch mode pass all checks but the last."""
    assert _call(mh, ws_bytes=0, **kw) == CAPACITY
