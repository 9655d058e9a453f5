"""The stream's table-per-frame mode on the CPU: metalhuffman_amd/csrc/mh_stream.cpp and
mh_stream_headers.cpp compiled unchanged with g++ against fake HIP runtime calls and fake
decode entries (tests/stream_headers_mock.cpp). Checks the slot rotation, one copy per
submit from a host buffer in slot layout and three otherwise (two and four with init
bytes), every copy and the decode on the slot's stream in that order, the slot layout the
decode is given, both mode-mismatch errors, the capacity errors, slot_status on unused and
rejected slots, and that creating a stream leaves the rasters alone -- with graph replays
(MH_STREAM_GRAPHS=1), with MH_STREAM_GRAPHS=0 and with the variable unset (direct launches)."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_headers_slots_copies_and_modes(tmp_path):
    exe = tmp_path / "stream_headers_mock"
    csrc = os.path.join(ROOT, "metalhuffman_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           os.path.join(ROOT, "tests", "stream_headers_mock.cpp"), os.path.join(csrc, "mh_stream.cpp"),
           os.path.join(csrc, "mh_stream_headers.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout
