"""mh_check_frame_cpu (codec.check_frame), the host twin of mh_check_headers' walk, against the oracle:
every frame of defect_helpers' seeded "frames", "headers" and "check" batches (the decode entries' defect
kinds, swapped offsets, an offset past the slot) under the frame's own header, and the header verdicts.
The only cases left out are the check cases with a truncated T2, which no header expresses."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

import check_frames_helpers as CH
import defect_helpers as DH

CLEAN = CH.CLEAN


@pytest.mark.parametrize("entry", ["frames", "headers", DH.CHECK])
def test_twin_equals_the_oracle_on_every_frame(mh, oracle, entry):
    cases = CH.cases(mh, oracle, entry)
    assert len(cases) == (30 if entry == DH.CHECK else 40)
    frames = dirty = 0
    for case in cases:
        for f, df in enumerate(case.frames):
            status, report = mh.check_frame(df.ef)
            assert status == 0 and report.dtype == np.uint32
            assert report.tolist() == df.report.tolist(), (case.describe(), f)
            assert int(report[1]) == 0
            frames += 1
            dirty += report.tolist() != CLEAN
    # the coverage the sweep is relied on for (counted with the oracle alone)
    assert (frames, dirty) == {"frames": (132, 76), "headers": (142, 83)}.get(entry, (frames, dirty))
    assert dirty >= 10 and frames - dirty >= 10


def test_check_cases_left_out_are_the_truncated_t2_ones(mh, oracle):
    every = [DH.defect_case(mh, oracle, DH.CHECK, i) for i in range(CH.N_CASES)]
    assert sum(1 for c in every if c.t2_entries) == 10
    kept = CH.cases(mh, oracle, DH.CHECK)
    kinds = [df.kind for c in kept for df in c.frames]
    assert kinds.count("past") == 8 and kinds.count("swap") == 6


def test_mixed_headers_and_defect_kinds_are_covered(mh, oracle):
    mixed = {e: sum(1 for c in CH.cases(mh, oracle, e) if len({df.header for df in c.frames}) > 1)
             for e in ("frames", "headers")}
    assert mixed == {"frames": 16, "headers": 9}
    dfs = [df for c in CH.cases(mh, oracle, "frames") for df in c.frames]
    assert sum(1 for df in dfs if int(df.report[0])) == 21 and sum(1 for df in dfs if int(df.report[2])) == 73


@pytest.mark.parametrize("name,status", [("good", 0), ("too_long", -3), ("kraft", -5), ("both", -3)])
def test_header_verdicts(mh, oracle, name, status):
    """A rejected header leaves the clean report; the verdict is the device builder's (a length over 16
    first, then a Kraft sum over 1)."""
    df = DH.made_frame(oracle, "escapes", 9, 2, 5)
    canon = CH.bad_header(df.ef.canon, name)
    got, report = mh.check_frame(dataclasses.replace(df.ef, canon=canon))
    assert got == status
    assert report.tolist() == (df.report.tolist() if status == 0 else CLEAN)


def test_offsets_past_the_slot_and_at_the_32_bit_edge(mh, oracle):
    for df in CH.far_offset_frames(oracle):
        status, report = mh.check_frame(df.ef)
        assert status == 0 and report.tolist() == df.report.tolist(), df.ef.block_offsets.tolist()


def test_null_arguments(mh):
    import ctypes
    L = mh.lib()
    rep = (ctypes.c_uint32 * 4)()
    offs = (ctypes.c_uint32 * 1)()
    buf = (ctypes.c_uint8 * 256)()
    assert L.mh_check_frame_cpu(None, 1, buf, 16, buf, rep) == -1
    assert L.mh_check_frame_cpu(offs, 0, buf, 16, buf, rep) == -1
    assert L.mh_check_frame_cpu(offs, 1, None, 16, buf, rep) == -1
    assert L.mh_check_frame_cpu(offs, 1, buf, 16, None, rep) == -1
    assert L.mh_check_frame_cpu(offs, 1, buf, 16, buf, None) == -1
