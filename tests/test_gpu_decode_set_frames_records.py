"""mh_decode_set_frames' device validation: ONE record corrupted per case, in a set of three small
frames (520 x 72: ten tiles and two workgroups; 264 x 40; 9 x 7). Each case is one launch. These are
validation cases, not faults: every one must end with all guard bytes intact and the other two frames
bit-exact. A rejected geometry gives MH_ERR_DIMS and a rejected raster MH_ERR_CAPACITY, with the
victim's raster untouched. A corrupt share or map word may lose tiles of its own frame only: each of the
victim's pixels is the picture's or untouched, and the status words of untouched frames keep what the
caller put there."""
from __future__ import annotations

import pytest

import decode_set_helpers as H

pytestmark = pytest.mark.gpu

SIZES = ((520, 72), (264, 40), (9, 7))
BUDGET = 3            # 14 tiles: round(3 * 10 / 14) = 2 groups, then 1 and 1 -> the map is [0, 0, 1, 2]
_SET: dict = {}


def _set(mh, oracle, device):
    if not _SET:
        fr = H.frames(mh, oracle, SIZES, ("escapes", "noesc", "flat"))
        efs = [f[0] for f in fr]
        fs = H.pack(device, efs)
        rec = H.records(mh, fs, BUDGET)
        assert rec.group_frame.tolist() == [0, 0, 1, 2] and rec.shares[:, :2].tolist() == [[0, 2], [2, 1], [3, 1]]
        _SET.update(fs=fs, tabs=H.tables(device, efs), rec=rec, wants=[f[1] for f in fr])
    return _SET["fs"], _SET["tabs"], _SET["rec"], _SET["wants"]


def _nb(f):
    return -(-SIZES[f][0] // 8) * -(-SIZES[f][1] // 8)


def _rejected(mh, oracle, device, victim, code, edit):
    fs, tabs, good, wants = _set(mh, oracle, device)
    rec = good.copy()
    edit(rec, fs)
    lay = H.run(device, fs, tabs, rec)
    assert lay.rc == 0
    # the layout the intact records describe: the victim's raster holds its fill, the others their pictures
    H.check(lay, good.rasters, fs.sizes, [None if f == victim else w for f, w in enumerate(wants)])
    assert lay.status == [code if f == victim else 0 for f in range(3)]


GEOMETRY = {
    "reserved": lambda v: lambda r, fs: r.geoms.__setitem__((v, 3), 1),
    "width_0": lambda v: lambda r, fs: r.geoms.__setitem__((v, 1), 0),
    "height_65536": lambda v: lambda r, fs: r.geoms.__setitem__((v, 2), 65536),
    "first_block_past_the_end": lambda v: lambda r, fs: r.geoms.__setitem__((v, 0), fs.total_blocks - _nb(v) + 1),
    "first_block_wraps": lambda v: lambda r, fs: r.geoms.__setitem__((v, 0), 0xFFFFFFFF),
}


@pytest.mark.parametrize("victim", [0, 1, 2])
@pytest.mark.parametrize("what", list(GEOMETRY))
def test_geometry_record(mh, oracle, device, what, victim):
    _rejected(mh, oracle, device, victim, H.MH_ERR_DIMS, GEOMETRY[what](victim))


def _offset(r, v, value):
    r.rasters[v, 0], r.rasters[v, 1] = value & 0xFFFFFFFF, value >> 32


def _last_row_overshoots(v):
    def edit(r, fs):
        w, h = SIZES[v]
        _offset(r, v, r.out_bytes - ((h - 1) * int(r.rasters[v, 2]) + H.up8(w)) + 8)
    return edit


RASTER = {
    "offset_past_out_bytes": lambda v: lambda r, fs: _offset(r, v, r.out_bytes),
    "offset_far_past": lambda v: lambda r, fs: _offset(r, v, 0xFFFFFFFFFFFFFFF8),
    "last_row_overshoots_by_8": _last_row_overshoots,
    "pitch_below_the_row": lambda v: lambda r, fs: r.rasters.__setitem__((v, 2), H.up8(SIZES[v][0]) - 8),
    "pitch_not_a_multiple_of_8": lambda v: lambda r, fs: r.rasters.__setitem__((v, 2), int(r.rasters[v, 2]) + 4),
    "offset_not_a_multiple_of_8": lambda v: lambda r, fs: _offset(r, v, int(r.rasters[v, 0]) + 4),
    "pitch_above_the_limit": lambda v: lambda r, fs: r.rasters.__setitem__((v, 2), (1 << 20) + 8),
    "reserved": lambda v: lambda r, fs: r.rasters.__setitem__((v, 3), 1),
}


@pytest.mark.parametrize("victim", [0, 1, 2])
@pytest.mark.parametrize("what", list(RASTER))
def test_raster_record(mh, oracle, device, what, victim):
    _rejected(mh, oracle, device, victim, H.MH_ERR_CAPACITY, RASTER[what](victim))


def test_the_last_row_that_just_fits_is_accepted(mh, oracle, device):
    """The bound is exact: out_bytes cut down to the last raster's last written byte passes, eight bytes
    less rejects that frame alone."""
    fs, tabs, good, wants = _set(mh, oracle, device)
    w, h = SIZES[2]
    end = (int(good.rasters[2, 0]) | int(good.rasters[2, 1]) << 32) + (h - 1) * int(good.rasters[2, 2]) + H.up8(w)
    lay = H.run(device, fs, tabs, good, out_bytes=end)
    H.check(lay, good.rasters, fs.sizes, wants)
    assert lay.status == [0, 0, 0]
    lay = H.run(device, fs, tabs, good, out_bytes=end - 8)
    H.check(lay, good.rasters, fs.sizes, [wants[0], wants[1], None])
    assert lay.status == [0, 0, H.MH_ERR_CAPACITY]


# (name, edit, the victim, may some of the victim's workgroups still serve it?)
SHARE_AND_MAP = [
    ("groups_0", lambda r: r.shares.__setitem__((0, 1), 0), 0, False),
    ("groups_0_of_one", lambda r: r.shares.__setitem__((2, 1), 0), 2, False),
    ("groups_above_the_limit", lambda r: r.shares.__setitem__((0, 1), (1 << 20) + 1), 0, False),
    ("groups_at_the_limit", lambda r: r.shares.__setitem__((0, 1), 1 << 20), 0, True),
    ("groups_too_many", lambda r: r.shares.__setitem__((0, 1), 5), 0, True),
    ("groups_too_few", lambda r: r.shares.__setitem__((0, 1), 1), 0, True),
    ("share_reserved", lambda r: r.shares.__setitem__((1, 2), 1), 1, False),
    ("share_reserved_1", lambda r: r.shares.__setitem__((1, 3), 0x80000000), 1, False),
    ("map_word_is_n_frames", lambda r: r.group_frame.__setitem__(1, 3), 0, True),
    ("map_word_is_all_ones", lambda r: r.group_frame.__setitem__(3, 0xFFFFFFFF), 2, False),
    ("map_word_names_another_frame", lambda r: r.group_frame.__setitem__(3, 1), 2, False),
    ("map_word_names_the_frame_before", lambda r: r.group_frame.__setitem__(2, 0), 1, False),
    ("map_word_of_slice_0_names_another", lambda r: r.group_frame.__setitem__(0, 2), 0, True),
    ("first_group_one_too_high", lambda r: r.shares.__setitem__((0, 0), 1), 0, True),
    ("first_group_one_too_high_of_one", lambda r: r.shares.__setitem__((1, 0), 3), 1, False),
    ("first_group_one_too_low", lambda r: r.shares.__setitem__((1, 0), 1), 1, False),
    ("first_group_wraps", lambda r: r.shares.__setitem__((2, 0), 0xFFFFFFFF), 2, False),
]


@pytest.mark.parametrize("name,edit,victim,arrives", SHARE_AND_MAP, ids=[c[0] for c in SHARE_AND_MAP])
def test_share_and_map(mh, oracle, device, name, edit, victim, arrives):
    """arrives False: none of the victim's workgroups passes its share, so its raster and its status
    word keep what they held. True: some do, and slice 0 -- the status word's writer -- may be among them."""
    fs, tabs, good, wants = _set(mh, oracle, device)
    rec = good.copy()
    edit(rec)
    lay = H.run(device, fs, tabs, rec)
    assert lay.rc == 0
    if arrives:
        # tiles may be lost or repeated, never misplaced: every pixel is the picture's or untouched
        H.check(lay, good.rasters, fs.sizes, wants, partial=(victim,))
        assert lay.status[victim] in (0, H.PRESET)
    else:
        H.check(lay, good.rasters, fs.sizes, [None if f == victim else w for f, w in enumerate(wants)])
        assert lay.status[victim] == H.PRESET
    assert [s for f, s in enumerate(lay.status) if f != victim] == [0, 0]
