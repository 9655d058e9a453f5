"""The mid-block marks' host functions under the host compiler's AddressSanitizer and
UndefinedBehaviorSanitizer (CPU only; host code only -- the HIP kernels are not built).

host/mh_mid_marks_selftest.c links mh_host.cpp and runs 120 cases: mh_encode_frame_marks writes
mh_encode_frame's bytes, its marks equal mh_mid_marks' walk and the marks computed from the
picture and the code lengths, and scrambled code bytes, offsets and short buffers are walked for
memory safety and the marks' bounds. Any sanitizer report aborts the program."""
from __future__ import annotations

import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metalhuffman_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]


def test_mid_marks_host_under_asan_ubsan():
    assert shutil.which("gcc") and shutil.which("g++"), "the host compilers that build the library are needed"
    with tempfile.TemporaryDirectory() as d:
        host = os.path.join(d, "mh_host.o")
        subprocess.run(["g++", *SAN, "-std=c++17", "-c", os.path.join(CSRC, "mh_host.cpp"), "-o", host], check=True)
        st = os.path.join(d, "selftest.o")
        subprocess.run(["gcc", *SAN, "-std=c11", "-Wall", "-Werror", "-c",
                        os.path.join(ROOT, "host", "mh_mid_marks_selftest.c"), "-o", st], check=True)
        exe = os.path.join(d, "selftest")
        subprocess.run(["g++", "-fsanitize=address,undefined", st, host, "-o", exe], check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
        for seed in ("1", "20261021"):
            r = subprocess.run([exe, seed], capture_output=True, text=True, env=env, timeout=300)
            assert r.returncode == 0 and "selftest ok 120" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
