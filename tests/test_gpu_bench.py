"""bench.py's plain run on the GPU: the headline figure only, and --dump-outputs writing
what the clocked region's last launch decoded."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_the_last_step(mh, bigbridge, tmp_path):
    from metalhuffman_amd import frames as F
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "8", "--warmup", "2",
                        "--frames", "24", "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (8, 2, 1)
    assert line["unit"] == "MB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    # value = decoded MB per step / the step's time (ms_per_step is rounded to 5 places)
    assert line["value"] == pytest.approx(bigbridge.size / 1e6 / (line["ms_per_step"] * 1e-3), rel=5e-3)
    assert line["full"] is False
    for k in ("roofline", "extras", "cpu_baseline", "frames_verified", "warm_value", "ungated_value"):
        assert k not in line, k
    d = line["dumped_outputs"]
    assert d["file"] == "decoded.npy" and d["shape"] == [1, 1536, 2048]
    assert sorted(os.listdir(out)) == ["decoded.npy"]
    got = np.load(out / "decoded.npy")
    assert got.dtype == np.float32 and got.shape == (1, 1536, 2048)
    # launch j of rank 0 decodes the block shuffle of BigBridge with seed j
    assert 0 <= d["launch"] < 24
    assert np.array_equal(got[0], F.block_shuffle(bigbridge, d["launch"]).astype(np.float32))
