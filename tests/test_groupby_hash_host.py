"""The general group-by (dbhip_groupby_hash_u32) without a GPU: the C ABI declared, bound and exported, the workspace
query, the host-side argument checks (before any HIP call), the compiled code object of csrc/groupby_hash.hip and the
dwarf list of the group-by CLI."""
import re
import subprocess
from pathlib import Path

import pytest

from dwarf_bench_amd import _capi

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "dwarf_bench_amd" / "_lib"
EINVAL, EWORKSPACE = -1, -2
NEW = ("dbhip_groupby_hash_workspace_bytes", "dbhip_groupby_hash_u32", "dbhip_check_distinct_workspace_bytes",
       "dbhip_check_distinct_u32")


def test_entry_points_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dbhip.h").read_text(), flags=re.S)
    lib = _capi.lib()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name


def test_workspace_query():
    ws = _capi.lib().dbhip_groupby_hash_workspace_bytes
    assert ws(1 << 31, 0) > 0 and ws((1 << 31) + 1, 0) == 0
    for n in (0, 1, 1000, 1 << 20, 1 << 24, 1 << 26):
        for mg in (0, 1, 64, 4096, 4097, 1 << 16, 1 << 20):
            b = ws(n, mg)
            assert b % 256 == 0 and b >= 256, (n, mg)
            groups = min(mg or n, n)
            assert b >= 256 + 12 * max(64, 2 * groups), (n, mg)  # the global table: 12-byte slots, two per group
            assert b <= 65 * n + (2 << 20), (n, mg)  # dbhip.h: at most 65 bytes per row plus 2 MiB
    # grows with n and with the bound
    assert ws(1 << 20, 0) < ws(1 << 22, 0) < ws(1 << 24, 0)
    assert ws(1 << 24, 64) < ws(1 << 24, 1 << 16) < ws(1 << 24, 1 << 20) <= ws(1 << 24, 0)
    assert ws(1 << 24, 4096) <= ws(1 << 24, 4097)


def test_argument_errors_need_no_device():
    lib = _capi.lib()
    fake = 1 << 20  # 256-aligned, never dereferenced: every call below fails on the host first
    n, mg = 4096, 100
    wsb = lib.dbhip_groupby_hash_workspace_bytes(n, mg)

    def call(keys=fake, vals=fake, n=n, mg=mg, ok=fake, os_=fake, oc=fake, og=fake, w=fake, wb=wsb):
        return lib.dbhip_groupby_hash_u32(keys, vals, n, mg, ok, os_, oc, og, w, wb, None)

    assert call(keys=None) == EINVAL and call(vals=None) == EINVAL
    assert call(ok=None) == EINVAL and call(os_=None) == EINVAL and call(og=None) == EINVAL
    assert call(keys=fake + 4) == EINVAL and call(vals=fake + 8) == EINVAL  # 16-byte alignment
    assert call(n=(1 << 31) + 1, wb=1 << 40) == EINVAL
    assert call(w=None) == EWORKSPACE and call(w=fake + 64) == EWORKSPACE and call(wb=wsb - 1) == EWORKSPACE
    assert call(n=1 << 20, mg=0, wb=wsb) == EWORKSPACE  # a workspace sized for fewer groups
    dist = lib.dbhip_check_distinct_u32
    dwb = lib.dbhip_check_distinct_workspace_bytes(n)
    assert dwb >= 2 * 4 * n
    assert dist(None, n, fake, fake, dwb, None) == EINVAL and dist(fake, n, None, fake, dwb, None) == EINVAL
    assert dist(fake, n, fake, None, dwb, None) == EWORKSPACE and dist(fake, n, fake, fake, dwb - 1, None) == EWORKSPACE


def test_ops_refuses_unaligned_columns_and_large_bounds():
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    t = torch.zeros(17, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops._need16(t[1:], "keys")  # what GroupByHash.launch applies to both columns
    with pytest.raises(ValueError):
        ops.GroupByHash(16, max_groups=1 << 32, device="cpu")


def test_code_object_has_no_scratch_and_uses_lds_cas(tmp_path):
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc",
                    "--save-temps", "-c", str(ROOT / "dwarf_bench_amd" / "csrc" / "groupby_hash.hip"), "-o",
                    str(tmp_path / "gbh.o")], check=True, cwd=tmp_path, timeout=600)
    asm = (tmp_path / "groupby_hash-hip-amdgcn-amd-amdhsa-gfx950.s").read_text()
    bodies = dict(re.findall(r"^(_ZN\S*gbh_\w+):.*?\n(.*?)s_endpgm", asm, flags=re.S | re.M))
    assert len(bodies) == 6, sorted(bodies)  # lds, global, part, giant, compact, finish
    meta = re.findall(r"\.name:\s+(_ZN\S*gbh_\w+)\s*\n(?:.*\n)*?\s*\.private_segment_fixed_size:\s+(\d+)", asm)
    assert len(meta) == 6 and all(size == "0" for _, size in meta), meta
    assert "scratch_" not in "".join(bodies.values())
    lds = next(b for name, b in bodies.items() if "gbh_lds_kernel" in name)
    assert "ds_cmpst" in lds and "ds_add_u32" in lds
    assert "global_atomic_cmpswap " in lds  # the flush / overflow into the global table


def _names(exe):
    r = subprocess.run([str(exe), "list"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    return [l.strip() for l in r.stdout.splitlines() if l.startswith("\t")]


def test_groupby_hash_cli_lists_the_default_set_plus_its_dwarf():
    exe, gbh = LIB / "dwarf_bench", LIB / "dwarf_bench_groupby_hash"
    if not exe.exists() or not gbh.exists():
        from dwarf_bench_amd import build
        build.build_hip()
        build.build_host()
    default, with_gbh = _names(exe), _names(gbh)
    assert sorted(set(with_gbh) - set(default)) == ["GroupByHashHip"] and len(with_gbh) == len(default) + 1
    assert set(default) <= set(with_gbh)
    for other in ("dwarf_bench", "dwarf_bench_experimental", "dwarf_bench_slab"):
        assert "GroupByHashHip" not in _names(LIB / other)
