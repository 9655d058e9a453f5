"""The set encoder's host planner (mh_encode_set_plan, codec.encode_set_plan; CPU only): geometry
against codec.frame_set_layout for host-encoded frames of the same sizes, slot offsets, the two
workgroup maps, the workspace size, the fetch mode, and every check's code in the documented order."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

INVALID, DIMS, CAPACITY, ALIGN = -1, -2, -4, -6
EDGE_SIZES = [(1, 1), (8, 8), (65535, 8), (8, 65535)]
SPAN_MAX = 0x7FFFFFF0


def r16(v):
    return (v + 15) // 16 * 16


def size_lists():
    """Seeded lists of 1..12 sizes; the edge sizes come round in turn."""
    out = []
    for seed in range(14):
        r = np.random.default_rng([seed, 31])
        n = 1 + seed % 12
        sizes = [(int(r.integers(1, 700)), int(r.integers(1, 500))) for _ in range(n)]
        sizes[int(r.integers(0, n))] = EDGE_SIZES[seed % 4]
        if n > 4:
            sizes[0], sizes[-1] = EDGE_SIZES[(seed + 1) % 4], (2056, 8)
        out.append(sizes)
    out.append(list(EDGE_SIZES))
    return out


def sources(sizes, base=0x7000_0000_0000, ps=1, pad=0, caps=None):
    """Planar (ps = 1) or strided records, one allocation each, 4-byte aligned."""
    out, addr = [], base
    for i, (w, h) in enumerate(sizes):
        pitch = w * ps + pad
        cap = caps[i] if caps is not None else r16(((w + 7) // 8) * ((h + 7) // 8) * 128 + 4) + 16
        out.append((addr, pitch, ps, w, h, cap))
        addr += (pitch * h + 255) // 256 * 256 + 256
    return out


def host_frames(mh, sizes):
    """Host-encoded frames of these sizes (constant images: the geometry alone matters)."""
    return [mh.encode_frame(np.full((h, w), 7, np.uint8)) for w, h in sizes]


@pytest.mark.parametrize("case", range(15))
def test_plan_matches_the_host_layout(mh, case):
    from metalhuffman_amd import _native as N
    sizes = size_lists()[case]
    src = sources(sizes)
    p = mh.encode_set_plan(src)
    t = p.totals
    lay = mh.frame_set_layout(host_frames(mh, sizes))
    assert np.array_equal(p.geoms, lay.geoms)
    assert (t.total_blocks, t.max_width, t.max_height, t.n_frames) == (lay.total_blocks, lay.width, lay.height, len(sizes))
    assert t.geoms_offset % 16 == 0 and t.split_map_offset % 16 == 0 and t.pack_map_offset % 16 == 0
    assert t.plan_bytes == p.plan.size == int(mh.lib().mh_encode_set_plan_bytes(len(src), mh.codec.set_sources(src)[0]))
    recs = p.records
    caps = [s[5] for s in src]
    nbs = [((w + 7) // 8) * ((h + 7) // 8) for w, h in sizes]
    tiles = [-(-nb // N.MH_SET_TILE_BLOCKS) for nb in nbs]
    assert [r.slot_offset for r in recs] == [int(v) for v in np.concatenate([[0], np.cumsum(caps)[:-1]])]
    assert t.codes_bytes == sum(caps)
    assert [r.first_tile for r in recs] == [int(v) for v in np.concatenate([[0], np.cumsum(tiles)[:-1]])]
    assert [r.first_block for r in recs] == [int(g[0]) for g in lay.geoms]
    assert [(r.width, r.height, r.block_width, r.n_blocks, r.n_tiles) for r in recs] == \
        [(w, h, (w + 7) // 8, nb, nt) for (w, h), nb, nt in zip(sizes, nbs, tiles)]
    assert [(r.pixels, r.row_pitch, r.pixel_stride, r.codes_cap) for r in recs] == \
        [(s[0], s[1] if s[4] > 1 else 0, s[2], s[5]) for s in src]
    # the split map: every (frame, tile) exactly once
    want = [(f, k) for f, nt in enumerate(tiles) for k in range(nt)]
    assert t.total_tiles == t.split_grid == len(want)
    assert sorted(map(tuple, p.split_map.tolist())) == want
    # the pack map: every tile exactly once, a unit inside one frame
    seen = []
    for f, k in p.pack_map.tolist():
        assert k % N.MH_SET_PACK_TILES == 0 and k < tiles[f]
        seen += [(f, j) for j in range(k, min(k + N.MH_SET_PACK_TILES, tiles[f]))]
    assert sorted(seen) == want and len(seen) == len(want)
    assert t.pack_grid == len(p.pack_map) == sum(-(-nt // N.MH_SET_PACK_TILES) for nt in tiles)
    # the workspace: at least the sum of its parts (tables, meta, tile counts, tile offsets, tile tails)
    n, nt = len(sizes), len(want)
    assert t.workspace_bytes >= n * 1024 + n * 32 * 8 + nt * 512 + (nt + n) * 4 + nt * 64
    # planar records at aligned addresses: dword loads when every pitch that is used is a multiple of 4
    assert t.fetch_mode == (1 if all(w % 4 == 0 for w, h in sizes if h > 1) else N.MH_SET_FETCH_BYTES)


def test_fetch_modes(mh):
    from metalhuffman_amd import _native as N
    sizes = [(30, 20), (64, 64), (9, 7)]
    # aligned stride-3 records (planes of RGB images, pitch a multiple of 4): channel 0
    rgb = sources(sizes, ps=3, pad=0)
    rgb = [(a, (p + 3) // 4 * 4, ps, w, h, c) for a, p, ps, w, h, c in rgb]
    assert mh.encode_set_plan(rgb).totals.fetch_mode == 3
    for ps in (1, 2, 4):
        s = [(a, (p + 3) // 4 * 4, q, w, h, c) for a, p, q, w, h, c in sources(sizes, ps=ps)]
        assert mh.encode_set_plan(s).totals.fetch_mode == ps
    # ... and channels 1 and 2: the address of a later byte of an aligned pixel
    planes = [(a + c, p, ps, w, h, cap) for a, p, ps, w, h, cap in rgb for c in range(3)]
    assert mh.encode_set_plan(planes).totals.fetch_mode == 3
    # one misaligned record: its address (no byte of a pixel that starts on a dword), or its pitch
    off = list(rgb)
    off[1] = (off[1][0] + 3,) + off[1][1:]
    assert mh.encode_set_plan(off).totals.fetch_mode == N.MH_SET_FETCH_BYTES
    gray = [(a, (p + 3) // 4 * 4, q, w, h, c) for a, p, q, w, h, c in sources(sizes)]
    assert mh.encode_set_plan(gray).totals.fetch_mode == 1
    gray[2] = (gray[2][0] + 1,) + gray[2][1:]
    assert mh.encode_set_plan(gray).totals.fetch_mode == N.MH_SET_FETCH_BYTES
    off = list(rgb)
    off[2] = (off[2][0], off[2][1] + 1) + off[2][2:]
    assert mh.encode_set_plan(off).totals.fetch_mode == N.MH_SET_FETCH_BYTES
    # a misaligned pitch of a one-row frame is ignored
    one = [(0x1000, 7, 3, 5, 1, 32), (0x2000, 16, 3, 5, 2, 32)]
    assert mh.encode_set_plan(one).totals.fetch_mode == 3
    # mixed strides, and a stride above 4
    mixed = list(rgb)
    mixed[0] = (mixed[0][0], 4 * sizes[0][0], 4) + mixed[0][3:]
    assert mh.encode_set_plan(mixed).totals.fetch_mode == N.MH_SET_FETCH_BYTES
    assert mh.encode_set_plan(sources(sizes, ps=5)).totals.fetch_mode == N.MH_SET_FETCH_BYTES


def _plan_rc(mh, src, flags=0, n=None, plan_bytes=None, null=()):
    from metalhuffman_amd import _native as N
    arr, cnt = mh.codec.set_sources(src)
    n = cnt if n is None else n
    size = int(mh.lib().mh_encode_set_plan_bytes(cnt, arr)) if plan_bytes is None else plan_bytes
    buf = np.full(max(size, 64) + 64, 0xEE, np.uint8)
    totals = N.mh_set_totals()
    rc = mh.lib().mh_encode_set_plan(n, None if "sources" in null else arr, flags,
                                     None if "plan" in null else buf.ctypes.data, size,
                                     None if "totals" in null else ctypes.byref(totals))
    assert (buf[size:] == 0xEE).all(), "the planner wrote behind plan_bytes"
    if rc != 0:
        assert (buf == 0xEE).all(), "a refused plan wrote into the blob"
    return rc


def test_planner_checks_in_order(mh):
    good = sources([(40, 30), (100, 9), (8, 8)])

    def bad(i, **kw):
        names = ("pixels", "row_pitch", "pixel_stride", "width", "height", "codes_cap", "reserved")
        s = [list(x) + [0] for x in good]
        for k, v in kw.items():
            s[i][names.index(k)] = v
        return [tuple(x) for x in s]

    assert _plan_rc(mh, good) == 0
    # 1. NULL pointers, n = 0
    for null in ("sources", "plan", "totals"):
        assert _plan_rc(mh, good, null=(null,), plan_bytes=4096) == INVALID
    assert _plan_rc(mh, good, n=0, plan_bytes=4096) == INVALID
    assert mh.lib().mh_encode_set_plan_bytes(0, mh.codec.set_sources(good)[0]) == 0
    assert mh.lib().mh_encode_set_plan_bytes(3, None) == 0
    # 2. a reserved word, an unknown flag -- ahead of every later check on any record
    everything = bad(0, width=0, codes_cap=8, row_pitch=1)
    assert _plan_rc(mh, bad(2, reserved=1), plan_bytes=4096) == INVALID
    assert _plan_rc(mh, [everything[0], everything[1], bad(2, reserved=5)[2]], plan_bytes=4096) == INVALID
    for flag in (0x2, 0x4, 0x400, 0x80000000):
        assert _plan_rc(mh, everything, flags=flag, plan_bytes=4096) == INVALID
    for flag in (0x1, 0x100, 0x200, 0x301):
        assert _plan_rc(mh, good, flags=flag) == 0
    # 3. dims, ahead of alignment and capacity on an earlier record
    for kw in (dict(width=0), dict(height=0), dict(width=65536), dict(height=65536), dict(pixel_stride=0),
               dict(pixel_stride=256)):
        s = bad(2, **kw)
        s[0] = bad(0, codes_cap=8, row_pitch=1)[0]
        assert _plan_rc(mh, s, plan_bytes=4096) == DIMS, kw
    assert _plan_rc(mh, bad(1, pixel_stride=255, row_pitch=255 * 100)) == 0
    # 4. codes_cap, ahead of capacity on an earlier record
    for cap in (0, 8, 24, 1000001):
        s = bad(2, codes_cap=cap)
        s[0] = bad(0, row_pitch=1)[0]
        assert _plan_rc(mh, s, plan_bytes=4096) == ALIGN, cap
    assert _plan_rc(mh, bad(1, codes_cap=16)) == 0
    # 5. capacity: a pitch below a row (height > 1 only), an unaddressable record, the totals, the blob
    assert _plan_rc(mh, bad(0, row_pitch=39), plan_bytes=4096) == CAPACITY
    assert _plan_rc(mh, bad(2, height=1, row_pitch=0)) == 0
    assert _plan_rc(mh, bad(0, row_pitch=SPAN_MAX + 1), plan_bytes=4096) == CAPACITY
    # 40 pixels wide: a tile lies in 8 * (254 // 5 + 2) = 416 rows; 30 rows of pitch p span 29 p + 40
    assert _plan_rc(mh, bad(0, row_pitch=(SPAN_MAX - 40) // 29)) == 0
    assert _plan_rc(mh, bad(0, row_pitch=(SPAN_MAX - 40) // 29 + 1), plan_bytes=4096) == CAPACITY
    # the 13 x 3 frame of test_gpu_encode_set_limits.py, in the middle: (3 - 1) p + 13 ps, in both modes
    for ps in (1, 3):
        top = (SPAN_MAX - 13 * ps) // 2
        for p, want in ((top, 0), (top - top % 4, 0), (top + 1, CAPACITY)):
            assert _plan_rc(mh, bad(1, width=13, height=3, pixel_stride=ps, row_pitch=p), plan_bytes=4096) == want, (ps, p)
    assert _plan_rc(mh, bad(0, codes_cap=2 ** 64 - 16), plan_bytes=4096) == CAPACITY   # the slot sum wraps
    size = int(mh.lib().mh_encode_set_plan_bytes(3, mh.codec.set_sources(good)[0]))
    assert size > 0 and _plan_rc(mh, good, plan_bytes=size - 1) == CAPACITY
    assert _plan_rc(mh, good, plan_bytes=size + 64) == 0


def test_block_total_limit(mh):
    """total_blocks above 2^32 - 1: 64 frames of 65535 x 65535 hold 2^26 blocks each."""
    big = [(0x1000, 65535, 1, 65535, 65535, 16)] * 64
    L = mh.lib()
    # 63 of them fit: 63 * 2^18 tiles and 63 * 2^16 pack units of 8 bytes each behind the records
    assert L.mh_encode_set_plan_bytes(63, mh.codec.set_sources(big)[0]) == 63 * (64 + 16) + 63 * 8 * (2 ** 18 + 2 ** 16)
    assert L.mh_encode_set_plan_bytes(64, mh.codec.set_sources(big)[0]) == 0
    with pytest.raises(mh.MHError) as e:
        mh.encode_set_plan(big)
    assert e.value.status == CAPACITY
