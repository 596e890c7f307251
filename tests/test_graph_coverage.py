"""tests/graph_testlib.COVERAGE names, for every entry point include/dbhip.h declares, the test that captures it into a
hipGraph or the reason why it cannot be captured.  Checked here without a GPU: the table's keys are the declared names,
and every test it names is a function of the module it names (found by reading the file: nothing is imported that
could touch a device)."""
import re
from pathlib import Path

from tests.graph_testlib import COVERAGE

ROOT = Path(__file__).resolve().parents[1]


def _declared():
    text = (ROOT / "include" / "dbhip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dbhip_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_entry_point_is_captured_or_excused():
    assert _declared() == sorted(COVERAGE)


def test_every_named_capture_test_exists():
    sources = {}
    for name, where in COVERAGE.items():
        if isinstance(where, str):
            assert where.strip() and "\n" not in where, name  # a one-line reason
            continue
        path, test = where
        if path not in sources:
            assert (ROOT / path).is_file(), (name, path)
            sources[path] = (ROOT / path).read_text()
        assert re.search(rf"^def {re.escape(test)}\(", sources[path], flags=re.M), (name, path, test)
        assert "graph_testlib" in sources[path] or "torch.cuda.graph" in sources[path], (name, path)


def test_the_excused_entry_points_are_the_ones_the_header_excuses():
    """only queries, the status read-back and the calibration call go uncaptured"""
    excused = sorted(n for n, w in COVERAGE.items() if isinstance(w, str))
    queries = sorted(n for n in _declared() if n.endswith("_workspace_bytes"))
    assert excused == sorted(queries + ["dbhip_version", "dbhip_device_info", "dbhip_radix_sort_rank_mode",
                                        "dbhip_workspace_status", "dbhip_radix_sort_prepare"])
