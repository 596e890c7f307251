"""`bench.py --dump-outputs DIR`: the headline scan's output of its last timed step, as .npy files that two builds can be
compared by: the compacted column and its count equal the oracle's on the seeded input."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_dump_outputs_is_the_scan_result_on_the_seeded_input(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "3", "--warmup", "1", "--dwarf", "scan",
                        "--no-cpu", "--no-pjoin", "--no-sweep", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert sorted(p.name for p in out.iterdir()) == ["scan_out.npy", "scan_out_size.npy"]
    got = np.load(out / "scan_out.npy")
    size = np.load(out / "scan_out_size.npy")
    assert got.dtype == np.float32 and size.dtype == np.float64
    src = po.gen_uniform_u32(line["config"]["rows"], 42, 1, 10000).view(np.int32)  # bench_scan's input, on the host
    exp = po.copy_if_lt(src, 5)
    assert size.tolist() == [exp.size] and np.array_equal(got, exp.astype(np.float32))
    assert abs(line["config"]["selectivity"] - exp.size / src.size) < 1e-12
