"""The C-ABI of the image encoders (include/metalhuffman.h: mh_encode_images_device_async,
mh_encode_images_shared_device_async and their workspace functions) and codec.image_planes, their
host definition. Every host check is made before any HIP call, with fake pointers, in the frames
entries' order plus the layout's own rules. CPU only: a call that passed every check would launch,
so each case here fails one check, the cases that probe the ORDER fail two and expect the earlier
one's code, and a case that must PASS a layout rule is stopped by a workspace of 0 bytes, the last
check of all. The seeded GPU sweep's coverage is asserted here too."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import encode_images_helpers as IH

OK, INVALID, DIMS, CAPACITY, ALIGN = 0, -1, -2, -4, -6
PIX, CANON_IN, CANON, CODES, LENS, FCO, OFFS, STATUS, HSTATUS, WS = (
    0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x90000, 0xA0000, 0x100000)
W, H, N, C = 64, 64, 2, 3
LAYOUT = dict(image_stride=W * H * 4, row_pitch=W * 4, pixel_stride=4, first_channel=0, n_planes=C, plane_major=0)
NO_LAYOUT = "no layout"


def _args(mh, **kw):
    a = dict(pix=PIX, lay=None, n=N, w=W, h=H, flags=0, canon_in=None, canon=CANON, codes=CODES, slot=16384,
             lens=LENS, fco=FCO, offs=OFFS, init=None, status=STATUS, hstatus=HSTATUS, ws=WS, ws_bytes=None)
    lay = dict(LAYOUT)
    for k in list(kw):
        if k in LAYOUT:
            lay[k] = kw.pop(k)
    a.update(kw)
    from metalhuffman_amd import _native as N_
    a["lay"] = None if a["lay"] == NO_LAYOUT else ctypes.byref(N_.mh_image_layout(**lay))
    a["planes"] = lay["n_planes"]
    return a


def _shared(mh, **kw):
    a = _args(mh, **kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = int(mh.lib().mh_encode_images_shared_workspace_bytes(a["w"], a["h"], a["n"], a["planes"]))
    return mh.lib().mh_encode_images_shared_device_async(
        a["pix"], a["lay"], a["n"], a["w"], a["h"], a["flags"], a["canon_in"], a["canon"], a["codes"], a["slot"],
        a["lens"], a["fco"], a["offs"], a["init"], a["status"], a["hstatus"], a["ws"], a["ws_bytes"], None)


def _per_frame(mh, **kw):
    a = _args(mh, **kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = int(mh.lib().mh_encode_images_workspace_bytes(a["w"], a["h"], a["n"], a["planes"]))
    return mh.lib().mh_encode_images_device_async(
        a["pix"], a["lay"], a["n"], a["w"], a["h"], a["flags"], a["canon"], a["codes"], a["slot"], a["lens"],
        a["fco"], a["offs"], a["init"], a["status"], a["ws"], a["ws_bytes"], None)


def _all(mh, status, **kw):
    assert _per_frame(mh, **kw) == status
    assert _shared(mh, **kw) == status
    assert _shared(mh, canon_in=CANON_IN, **kw) == status


def test_symbols_exported(mh):
    lib = ctypes.CDLL(mh.LIB_PATH)
    for name in ("mh_encode_images_device_async", "mh_encode_images_shared_device_async",
                 "mh_encode_images_workspace_bytes", "mh_encode_images_shared_workspace_bytes"):
        assert hasattr(lib, name), name
        assert name in mh.EXPORTS, name


def test_layout_struct_is_the_headers():
    from metalhuffman_amd import _native as N_
    L = N_.mh_image_layout
    assert ctypes.sizeof(L) == 32
    assert [(f, getattr(L, f).offset) for f, _ in L._fields_] == [
        ("image_stride", 0), ("row_pitch", 8), ("pixel_stride", 16), ("first_channel", 20), ("n_planes", 24),
        ("plane_major", 28)]
    assert N_.MH_IMAGE_TILE_SPAN_MAX == IH.SPAN_MAX
    assert [N_.image_tile_rows(w) for w in (1, 8, 9, 2032, 2033, 65535)] == [2048, 2048, 1032, 24, 16, 16]
    assert all(N_.image_tile_rows(w) == IH.tile_rows(w) for w in range(1, 4200, 7))


def test_workspaces_are_the_frames_ones_at_n_times_c(mh):
    L = mh.lib()
    for w, h, n, c in [(1, 1, 1, 1), (64, 64, 2, 3), (2048, 1536, 64, 3), (1040, 1032, 3, 4), (13, 11, 5, 2)]:
        assert int(L.mh_encode_images_workspace_bytes(w, h, n, c)) == int(L.mh_encode_frames_workspace_bytes(w, h, n * c))
        assert int(L.mh_encode_images_shared_workspace_bytes(w, h, n, c)) == \
            int(L.mh_encode_frames_shared_workspace_bytes(w, h, n * c))
    assert int(L.mh_encode_images_workspace_bytes(8, 8, 0x80000000, 1)) == 0          # more than 2^31 - 1 frames
    assert int(L.mh_encode_images_shared_workspace_bytes(8, 8, 0x40000000, 2)) == 0


# one failing check each: the frames entries' checks, then the layout's
SINGLE = [
    (dict(pix=None), INVALID), (dict(codes=None), INVALID), (dict(offs=None), INVALID), (dict(ws=None), INVALID),
    (dict(n=0), INVALID),
    (dict(lay=NO_LAYOUT), INVALID), (dict(n_planes=0), INVALID), (dict(n_planes=5, pixel_stride=8), INVALID),
    (dict(plane_major=2), INVALID),
    (dict(flags=0x40), INVALID), (dict(flags=0x2), INVALID), (dict(flags=0x400), INVALID),
    (dict(w=0), DIMS), (dict(h=0), DIMS), (dict(w=65536), DIMS), (dict(h=65536), DIMS),
    (dict(pixel_stride=0), DIMS), (dict(pixel_stride=2), DIMS), (dict(first_channel=2), DIMS),
    (dict(first_channel=0xFFFFFFFF, n_planes=1), DIMS),                    # the sum does not wrap
    (dict(codes=CODES + 4), ALIGN), (dict(slot=16380), ALIGN), (dict(ws=WS + 128), ALIGN),
    (dict(row_pitch=W * 4 - 1), CAPACITY),
    (dict(image_stride=63 * W * 4 + W * 4 - 1), CAPACITY),                 # one byte under an image's span
    (dict(ws_bytes=0), CAPACITY),
]


@pytest.mark.parametrize("kw,status", SINGLE)
def test_each_check_and_its_code(mh, kw, status):
    _all(mh, status, **kw)


def test_header_pointers(mh):
    assert _per_frame(mh, canon=None) == INVALID
    assert _shared(mh, canon=None) == INVALID
    assert _shared(mh, canon=None, canon_in=CANON_IN, ws_bytes=0) == CAPACITY     # optional in supplied mode
    assert _shared(mh, lens=None, fco=None, status=None, hstatus=None, init=None, ws_bytes=0) == CAPACITY


# two failing checks: the earlier one's code
ORDER = [
    (dict(pix=None, flags=0x40, w=0, codes=CODES + 4, ws_bytes=0), INVALID),
    (dict(n_planes=0, pixel_stride=0), INVALID),                                # the layout's NULL-class rules first
    (dict(plane_major=2, flags=0x40, w=0), INVALID),
    (dict(lay=NO_LAYOUT, w=0, codes=CODES + 4), INVALID),
    (dict(flags=0x40, pixel_stride=0), INVALID),                                # flags before dims
    (dict(pixel_stride=0, codes=CODES + 4), DIMS),                              # the layout's dims with the dims
    (dict(first_channel=3, row_pitch=1), DIMS),
    (dict(w=0, row_pitch=1), DIMS),
    (dict(codes=CODES + 4, row_pitch=1), ALIGN),                                # alignment before the pitch
    (dict(ws=WS + 16, image_stride=1), ALIGN),
    (dict(row_pitch=1, ws_bytes=0), CAPACITY),
    (dict(image_stride=1, ws_bytes=0), CAPACITY),
]


@pytest.mark.parametrize("kw,status", ORDER)
def test_check_order(mh, kw, status):
    _all(mh, status, **kw)


def test_what_the_layout_rules_let_through(mh):
    """Stopped only by the workspace of 0 bytes (MH_ERR_CAPACITY like the layout's own refusals, so the
    pair of each case shows the rule, not the code): the pitch is not looked at for one row, the image
    stride not for one image, planes 1..3 of 4 and a single plane of 7 are fine, both frame orders."""
    for kw in (dict(h=1, row_pitch=0), dict(n=1, image_stride=0), dict(first_channel=1),
               dict(pixel_stride=7, row_pitch=W * 7, image_stride=W * H * 7, n_planes=1, first_channel=6),
               dict(plane_major=1), dict(row_pitch=W * 4 + 1, image_stride=64 * (W * 4 + 1)),
               dict(n_planes=4), dict(image_stride=63 * W * 4 + W * 4)):
        _all(mh, CAPACITY, ws_bytes=0, **kw)
    # ... and the refusals next to them, with the workspace the call asks for
    _all(mh, CAPACITY, h=2, row_pitch=0)
    _all(mh, CAPACITY, n=2, image_stride=0)


def test_addressing_limit(mh):
    """A tile's descriptor spans at most MH_IMAGE_TILE_SPAN_MAX bytes:
    (min(H, MH_IMAGE_TILE_ROWS(W)) - 1) * row_pitch + W * pixel_stride. One byte over is refused with
    the workspace the call asks for; the GPU tests encode at the limit itself."""
    for w, h, ps in [(8, 2, 1), (8, 3, 3), (16, 9, 4), (2040, 40, 3), (64, 2000, 4), (8, 4000, 1)]:
        rows = min(h, IH.tile_rows(w))
        pitch = (IH.SPAN_MAX - w * ps) // (rows - 1)
        at = dict(w=w, h=h, n=1, pixel_stride=ps, n_planes=1, row_pitch=pitch, image_stride=0, slot=1 << 24)
        assert (rows - 1) * pitch + w * ps <= IH.SPAN_MAX < (rows - 1) * (pitch + 1) + w * ps
        _all(mh, CAPACITY, **dict(at, row_pitch=pitch + 1))
        _all(mh, CAPACITY, **dict(at, row_pitch=1 << 40))
        _all(mh, CAPACITY, **dict(at, row_pitch=(1 << 64) - 1))
    # one row: the pitch does not count, the row itself does
    _all(mh, CAPACITY, w=8, h=1, n=1, n_planes=1, pixel_stride=0x10000000, first_channel=5, row_pitch=0)


def test_planes_count_as_frames_in_the_limits(mh):
    """n_images * C is n_frames: more than 2^31 - 1 frames, and built mode's 2^32 symbols (2048 x 1536
    is 3,145,728 symbols: 1,365 frames fit -- 455 images of 3 planes -- and 456 images do not)."""
    big = 1 << 62
    tiny = dict(w=8, h=8, row_pitch=32, image_stride=256, slot=256)
    _all(mh, CAPACITY, n=0x2AAAAAAB, ws_bytes=big, **tiny)                        # 3 n = 2^31 + 1
    frame = dict(w=2048, h=1536, row_pitch=2048 * 4, image_stride=2048 * 1536 * 4, slot=1 << 23)
    assert _shared(mh, n=456, ws_bytes=big, **frame) == CAPACITY
    for kw in (dict(n=456, canon_in=CANON_IN), dict(n=455)):
        need = int(mh.lib().mh_encode_images_shared_workspace_bytes(2048, 1536, kw["n"], 3))
        assert need > 0 and _shared(mh, ws_bytes=need - 1, **frame, **kw) == CAPACITY


# ---- codec.image_planes: hand-written cases ------------------------------------------------------

def test_image_planes_by_hand(mh):
    a = np.arange(2 * 2 * 3 * 4, dtype=np.uint8).reshape(2, 2, 3, 4)      # [n, H, W, K]: byte = 24 i + 12 y + 4 x + k
    p = mh.image_planes(a)
    assert p.shape == (8, 2, 3) and p.dtype == np.uint8 and p.flags.c_contiguous
    assert p[0].tolist() == [[0, 4, 8], [12, 16, 20]] and p[3].tolist() == [[3, 7, 11], [15, 19, 23]]
    assert p[4].tolist() == [[24, 28, 32], [36, 40, 44]]
    p = mh.image_planes(a, first_channel=1, n_planes=2)                   # frame = 2 i + c
    assert p.shape == (4, 2, 3)
    assert p[1].tolist() == [[2, 6, 10], [14, 18, 22]] and p[2].tolist() == [[25, 29, 33], [37, 41, 45]]
    q = mh.image_planes(a, first_channel=1, n_planes=2, plane_major=True)  # frame = 2 c + i
    assert [q[k].tolist() for k in range(4)] == [p[k].tolist() for k in (0, 2, 1, 3)]
    assert mh.image_planes(a, 1).shape == (6, 2, 3)                       # every channel from the first on
    one = mh.image_planes(a[1], 3, 1)                                     # one [H, W, K] image
    assert one.shape == (1, 2, 3) and one[0].tolist() == [[27, 31, 35], [39, 43, 47]]
    view = a[:, :, 1:, :3]                                                # any view: the values count
    assert np.array_equal(mh.image_planes(view, 0, 3), mh.image_planes(np.ascontiguousarray(view), 0, 3))
    for bad in (dict(first_channel=4), dict(first_channel=2, n_planes=3), dict(n_planes=0), dict(first_channel=-1)):
        with pytest.raises(ValueError):
            mh.image_planes(a, **bad)
    with pytest.raises(ValueError):
        mh.image_planes(a.astype(np.uint16))
    with pytest.raises(ValueError):
        mh.image_planes(a[0, 0])


# ---- the seeded GPU sweep's cases reach what they must ----------------------------------------------

def test_sweep_cases_cover_both_load_paths_every_c_and_both_orders():
    cases = IH.sweep_cases()
    assert 38 <= len(cases) <= 44
    for entry in IH.ENTRIES:
        mine = [c for c in cases if c.entry == entry]
        assert {c.wide for c in mine} == {True, False}, entry
        assert {c.px.C for c in mine} == {1, 2, 3, 4}, entry
        assert {c.px.plane_major for c in mine} == {True, False}, entry
        assert {c.px.ps for c in mine if c.wide} >= {2, 3, 4}, entry
        assert any(c.n > 1 and c.px.gap for c in mine) and any(c.px.pitch_pad % 2 for c in mine), entry
        assert any(c.W % 8 for c in mine if c.wide) and any(c.H % 8 for c in mine if c.wide), entry
        assert any(c.init_zero for c in mine) and any(c.no_delta for c in mine) and any(c.ws_fill for c in mine), entry
    for c in cases:
        px = c.px
        assert 1 <= px.C <= 4 and px.fc + px.C <= px.ps and c.W >= 1 and c.H >= 1, c
        assert (c.H - 1) * px.pitch(c.W) + c.W * px.ps <= px.image_stride(c.W, c.H), c
