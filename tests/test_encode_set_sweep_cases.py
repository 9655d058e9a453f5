"""The seeded sweep of sets (set_encode_helpers.sweep_case), checked on the CPU: over the default range
-- the cases test_gpu_encode_set_sweep.py runs -- every case follows from its index alone, every drawn
value is inside its stated range, the host codec gives every frame's expected status (a rejection is
an expected value, never a reason to drop a case), the planner's fetch mode is the header's rule, and
the categories the sweep is there for are all hit at least twice. A category the default range misses
is mended in the generator's seed or weights, never here."""
from __future__ import annotations

import pytest

import encode_helpers as EH
import set_encode_helpers as SH
from encode_helpers import CAPACITY, OK, TOO_LONG

N = SH.SET_SWEEP_DEFAULT_CASES
CASES = [SH.sweep_case(i) for i in range(N)]
_PLANS: dict = {}


def _plan(mh, bigbridge, c):
    if c.i not in _PLANS:
        _PLANS[c.i] = SH.sweep_plan(mh, c, bigbridge)
    return _PLANS[c.i]


def _statuses(mh, bigbridge, c):
    return [s for s, _ in _plan(mh, bigbridge, c)[2]]


def _tiles(q):
    return -(-q.nb // EH.K_BATCH_TILE)


def test_a_case_follows_from_its_index_alone():
    assert [SH.sweep_case(i) for i in range(N)] == CASES
    assert len({c.describe() for c in CASES}) == N
    assert len({(c.recs, c.slots) for c in CASES}) == N
    assert N == 48 and SH.sweep_range() == (0, 48)


def test_cases_are_inside_the_drawn_ranges():
    edges = {e[0]: e for e in SH.EDGES}
    for c in CASES:
        assert 1 <= c.n <= 12 and len(c.slots) == c.n and set(c.slots) <= set(SH.SLOTS), c.describe()
        assert sum(q.nb for q in c.recs) <= SH.BLOCK_CAP, c.describe()
        for q in c.recs:
            bw, bh = EH.blocks(q.w, q.h)
            assert 1 <= bw <= 300 and 1 <= bh <= 24 and q.w >= 1 and q.h >= 1, c.describe()
            assert q.pitch >= q.w * q.ps and q.off >= 0
        assert c.kind in SH.KINDS and (c.kind == "interleaved" or (c.K, c.first) == (1, 0))
        assert 1 <= c.K <= 4 and 0 <= c.first < c.K
        ps = {q.ps for q in c.recs}
        assert ps == ({c.K} if c.kind == "interleaved" else ps & set(SH.BYTE_STRIDES) if c.kind == "strided" else {1})
        assert len(ps) == 1
        # the edge frame: its size from the list, at its position
        name, eW, eH, (ebw, ebh) = edges[c.edge]
        q = c.recs[c.edge_pos]
        bw, bh = EH.blocks(q.w, q.h)
        assert bw == ebw and (bh == ebh or (ebh == 0 and 1 <= bh <= 3)), c.describe()
        assert (eW is None or q.w == eW) and (eH is None or q.h == eH)
        if c.kind == "interleaved":   # frame u * C + c is plane first + c of image u: one size, one allocation
            C = c.K - c.first
            assert c.n % C == 0
            for f, q in enumerate(c.recs):
                head = c.recs[f - f % C]
                assert (q.alloc, q.w, q.h, q.pitch, q.off) == (f // C, head.w, head.h, head.pitch, head.off + f % C)
        elif c.kind == "windows":
            assert len(c.windows) == c.n and 1 <= len(c.pictures) <= 2
            assert {p for p, _, _ in c.windows} == set(range(len(c.pictures)))
            for q, (p, x0, y0) in zip(c.recs, c.windows):
                assert q.alloc == p and 0 <= x0 <= c.pictures[p][0] - q.w and 0 <= y0 <= c.pictures[p][1] - q.h
                assert q.pitch >= c.pictures[p][0] and q.ps == 1
            # the windows of a picture share its allocation, its first byte and its pitch
            for p in range(len(c.pictures)):
                assert len({(q.off - y0 * q.pitch - x0, q.pitch) for q, (k, x0, y0) in zip(c.recs, c.windows) if k == p}) == 1
        else:
            assert [q.alloc for q in c.recs] == list(range(c.n))
        if c.deep is not None:
            q = c.recs[c.deep]
            assert q.w % 8 == 0 and q.h % 8 == 0 and q.nb >= SH.DEEP_MIN_BLOCKS and c.kind != "windows"
        # the breaker: a case drawn for the dword mode that one allocation (one window) takes out of it
        if c.breaker is not None:
            assert c.fetch_mode == 0xFF and all(q.ps <= 4 for q in c.recs)
            if c.breaker == "address":
                assert all(q.pitch % 4 == 0 or q.h == 1 for q in c.recs)
                bad = {q.alloc for q in c.recs if q.off % 4 >= q.ps}
                assert len(bad) == 1 and (c.kind != "windows" or sum(q.off % 4 >= q.ps for q in c.recs) == 1)
            else:
                assert all(q.off % 4 < q.ps for q in c.recs)
                assert len({q.alloc for q in c.recs if q.pitch % 4 and q.h > 1}) == 1
        elif c.aligned:
            assert c.fetch_mode == c.recs[0].ps, c.describe()
        assert not (c.null_lens and c.null_status) or (c.pattern == "none" and (c.deep is None or c.limit))


def test_the_planner_follows_the_fetch_rule(mh):
    """totals.fetch_mode against the header's rule, computed here from the records (the allocations at
    256-byte aligned addresses, as the GPU test lays them out)."""
    for c in CASES:
        src = [q.record(0x7000_0000_0000 + (q.alloc << 32)) + (16,) for q in c.recs]
        assert mh.encode_set_plan(src, c.flags).totals.fetch_mode == SH.fetch_rule(src) == c.fetch_mode, c.describe()


def test_the_host_codec_gives_every_expected_status(mh, bigbridge):
    """Every case has a plan: an exact slot is accepted, a too small one is -4 unless the frame's codes
    fit 16 bytes, the deep frame is -3 without the limit flag and has 16-bit lengths with it, and no
    case that passes both optional outputs as NULL has a rejection."""
    for c in CASES:
        imgs, caps, exp = _plan(mh, bigbridge, c)
        assert len(imgs) == len(caps) == len(exp) == c.n
        assert all(im.shape == (q.h, q.w) for im, q in zip(imgs, c.recs))
        for f, ((s, ef), cap, slot) in enumerate(zip(exp, caps, c.slots)):
            assert cap % 16 == 0 and 16 <= cap <= SH.roomy_cap(c.recs[f].w, c.recs[f].h)
            assert s in (OK, TOO_LONG, CAPACITY) and (ef is not None) == (s == OK)
            if s == OK:
                assert EH.r4(ef.codes.size) <= cap and ef.canon.max() <= 16
                assert slot in ("roomy", "exact") or EH.r4(ef.codes.size) <= 16, (c.describe(), f)
                assert slot != "exact" or cap == EH.r16(EH.r4(ef.codes.size))
            if s == CAPACITY:
                assert slot in ("less16", "cap16")
            if f == c.deep:
                assert (ef is not None and ef.canon.max() == 16) or s == CAPACITY if c.limit else s == TOO_LONG, c.describe()
        if c.null_lens and c.null_status:
            assert all(s == OK for s, _ in exp), c.describe()


def test_rejections_cannot_hide_a_failure(mh, bigbridge):
    """At most one frame in three of the range is rejected, and every case of two frames or more has
    an accepted one."""
    rejected = total = 0
    for c in CASES:
        st = _statuses(mh, bigbridge, c)
        rejected += sum(s != OK for s in st)
        total += len(st)
        assert c.n < 2 or any(s == OK for s in st), c.describe()
    assert 3 * rejected <= total, (rejected, total)


def _suffix(r):
    return lambda c, st: (c.kind == "interleaved" and c.first == r and c.fetch_mode == c.K
                          and all(q.off % 4 >= r for q in c.recs) and any(q.off % 4 == r for q in c.recs))


def _multi_between_ones(c, st):
    return any(st[f] != OK and _tiles(c.recs[f]) > 1 and _tiles(c.recs[f - 1]) == 1 and _tiles(c.recs[f + 1]) == 1
               for f in range(1, c.n - 1))


CATEGORIES = {
    "fetch mode 1": lambda c, st: c.fetch_mode == 1,
    "fetch mode 2": lambda c, st: c.fetch_mode == 2,
    "fetch mode 3": lambda c, st: c.fetch_mode == 3,
    "fetch mode 4": lambda c, st: c.fetch_mode == 4,
    "fetch by bytes": lambda c, st: c.fetch_mode == 0xFF,
    "a suffix of planes, pixels % 4 from 1": _suffix(1),
    "a suffix of planes, pixels % 4 from 2": _suffix(2),
    "a suffix of planes, pixels % 4 = 3": _suffix(3),
    "the last plane alone": lambda c, st: c.kind == "interleaved" and c.first == c.K - 1 > 0 and c.fetch_mode == c.K,
    "a breaker by address": lambda c, st: c.breaker == "address",
    "a breaker by pitch": lambda c, st: c.breaker == "pitch",
    "windows of one picture": lambda c, st: c.kind == "windows" and len(c.pictures) == 1 and c.n > 1,
    "windows of two pictures": lambda c, st: c.kind == "windows" and len(c.pictures) == 2,
    "windows in the dword mode": lambda c, st: c.kind == "windows" and c.fetch_mode == 1,
    "a stride above 4": lambda c, st: c.recs[0].ps > 4,
    "a frame 256 blocks wide or wider": lambda c, st: any(EH.blocks(q.w, q.h)[0] >= 256 for q in c.recs),
    "255 blocks": lambda c, st: any(q.nb == 255 for q in c.recs),
    "256 blocks": lambda c, st: any(q.nb == 256 for q in c.recs),
    "257 blocks": lambda c, st: any(q.nb == 257 for q in c.recs),
    "1023 blocks": lambda c, st: any(q.nb == 1023 for q in c.recs),
    "1024 blocks": lambda c, st: any(q.nb == 1024 for q in c.recs),
    "1025 blocks": lambda c, st: any(q.nb == 1025 for q in c.recs),
    "a frame of 1 x 1": lambda c, st: any((q.w, q.h) == (1, 1) for q in c.recs),
    "an edge frame first": lambda c, st: c.edge_pos == 0 and c.n > 1,
    "an edge frame last": lambda c, st: c.edge_pos + (c.K - c.first) == c.n and c.n > 1,
    "a rejected first frame": lambda c, st: c.n > 1 and st[0] != OK,
    "a rejected last frame": lambda c, st: c.n > 1 and st[-1] != OK,
    "two adjacent rejected frames": lambda c, st: any(a != OK and b != OK for a, b in zip(st, st[1:])),
    "a rejected multi-tile frame between one-tile frames": _multi_between_ones,
    "an exact-fit slot": lambda c, st: any(s == OK and slot == "exact" for s, slot in zip(st, c.slots)),
    "a slot 16 bytes short": lambda c, st: any(s == CAPACITY and slot == "less16" for s, slot in zip(st, c.slots)),
    "a slot of 16 bytes": lambda c, st: any(s == CAPACITY and slot == "cap16" for s, slot in zip(st, c.slots)),
    "d_codes_len NULL": lambda c, st: c.null_lens,
    "d_status NULL": lambda c, st: c.null_status,
    "d_codes_len NULL beside a rejection": lambda c, st: c.null_lens and any(s != OK for s in st),
    "d_status NULL beside a rejection": lambda c, st: c.null_status and any(s != OK for s in st),
    "a garbage workspace": lambda c, st: c.ws_fill is not None,
    "a zeroed workspace and its flag": lambda c, st: c.ws_fill is None,
    "MH_FLAG_NO_DELTA": lambda c, st: c.no_delta,
    "init bytes": lambda c, st: c.init_zero,
    "MH_ENCODE_LIMIT_LENGTHS": lambda c, st: c.limit,
    "a deep frame with the limit flag": lambda c, st: c.deep is not None and c.limit and st[c.deep] == OK,
    "a deep frame without it": lambda c, st: c.deep is not None and not c.limit and st[c.deep] == TOO_LONG,
    "n = 1": lambda c, st: c.n == 1,
    "n >= 10": lambda c, st: c.n >= 10,
}


def hits(mh, bigbridge):
    """name -> the cases of the default range that hit the category."""
    return {name: [c.i for c in CASES if hit(c, _statuses(mh, bigbridge, c))] for name, hit in CATEGORIES.items()}


@pytest.mark.parametrize("category", list(CATEGORIES))
def test_category_is_hit_twice(mh, bigbridge, category):
    got = [c.i for c in CASES if CATEGORIES[category](c, _statuses(mh, bigbridge, c))]
    assert len(got) >= 2, (category, got)
