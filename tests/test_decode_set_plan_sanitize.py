"""The planner of mh_decode_set_frames under the host compiler's AddressSanitizer and
UndefinedBehaviorSanitizer (CPU only; host code only -- the HIP kernels are not built).

host/mh_decode_set_plan_selftest.c is a stand-alone program: it links mh_host.cpp (and mh_cpu.cpp, as
the other self-tests do) and runs seeded sets -- the tile edges, the dimension limits, 1 to 300 frames,
every pitch alignment, budgets from 1 to 2^32 - 1 -- through the sizing call and mh_decode_set_plan
into arrays of exactly the reported sizes, checks every record and map word, and the refusals. Any
sanitizer report aborts the program (-fno-sanitize-recover). Nothing is preloaded and nothing of it
runs in Python."""
from __future__ import annotations

import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metalhuffman_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]


def test_decode_set_planner_under_asan_ubsan():
    if not (shutil.which("gcc") and shutil.which("g++")):
        pytest.skip("host compilers not found")
    with tempfile.TemporaryDirectory() as d:
        objs = []
        for src in ("mh_host.cpp", "mh_cpu.cpp"):
            o = os.path.join(d, src + ".o")
            subprocess.run(["g++", *SAN, "-std=c++17", "-pthread", "-c", os.path.join(CSRC, src), "-o", o], check=True)
            objs.append(o)
        st = os.path.join(d, "decode_set_plan_selftest.o")
        subprocess.run(["gcc", *SAN, "-std=c11", "-Wall", "-Wextra", "-Werror", "-c",
                        os.path.join(ROOT, "host", "mh_decode_set_plan_selftest.c"), "-o", st], check=True)
        exe = os.path.join(d, "decode_set_plan_selftest")
        subprocess.run(["g++", "-fsanitize=address,undefined", "-pthread", st, *objs, "-o", exe], check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
        for seed in ("1", "20261021"):
            r = subprocess.run([exe, seed], capture_output=True, text=True, env=env, timeout=120)
            assert r.returncode == 0 and "decode set plan selftest ok" in r.stdout and not r.stderr, \
                (r.stdout[-2000:], r.stderr[-4000:])
