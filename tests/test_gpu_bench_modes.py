"""A plain `bench.py` run measures the headline only; `--full` adds everything else (roofline, cold-source control,
oracle check, CPU baselines, the other dwarfs, the partitioned join) to the same line."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
FULL_ONLY = ("roofline", "value_cold", "cold_over_warm_time", "parity_check", "cpu_baseline", "dwarfs", "pjoin")


def _line(*extra):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "3", "--warmup", "1", *extra],
                       capture_output=True, text=True, timeout=900, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def _check_contract(line):
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config"):
        assert k in line, k
    assert line["metric"] == json.loads((ROOT / "BASELINE.json").read_text())["metric"]
    assert line["unit"] == "Mrows/s" and line["higher_is_better"] is True and line["dtype"] == "int32"
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert abs(line["value"] - line["config"]["rows"] / (line["ms_per_step"] * 1e3)) < 1e-6 * line["value"]
    assert 0 < line["config"]["selectivity"] < 1e-3  # x < 5 of uniform [1, 10000]


def test_plain_run_measures_the_headline_only():
    line = _line()
    _check_contract(line)
    assert not [k for k in FULL_ONLY if k in line], line


def test_full_run_adds_the_other_sections():
    line = _line("--full", "--dwarf", "groupby", "--no-cpu", "--no-pjoin")
    _check_contract(line)
    roof = line["roofline"]
    assert roof["bound"] == "hbm" and roof["kernel_us_avg"] > 0
    assert abs(roof["achieved"] - roof["algorithmic_bytes"] / roof["kernel_us_avg"] / 1e3) < 1e-6 * roof["achieved"]
    assert line["value_cold"] > 0 and line["cold_over_warm_time"] > 0
    assert line["parity_check"] is True and line["cpu_baseline"] is None
    assert set(line["dwarfs"]["scan"]["selectivity_sweep"]) == {"101", "1001", "5001", "10001"}
    assert line["dwarfs"]["groupby"]["kernel_us"] > 0 and "sort_8bit" not in line["dwarfs"]
