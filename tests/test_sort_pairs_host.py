"""The key-value radix sort / argsort (dbhip_radix_sort_pairs_*) without a GPU: the workspace query, the host-side
argument checks (all before any HIP call) and the compiled code object of the pairs kernels."""
import re
import subprocess
from pathlib import Path

import pytest

from dwarf_bench_amd import _capi
from tests.capi_testlib import EINVAL, EWORKSPACE

ROOT = Path(__file__).resolve().parents[1]


def test_workspace_query():
    lib = _capi.lib()
    ws, keys_only = lib.dbhip_radix_sort_pairs_workspace_bytes, lib.dbhip_radix_sort_workspace_bytes
    assert ws(1 << 24, 8) % 256 == 0 and ws(1 << 24, 8) > 0
    for n in (0, 1, 8192, 8193, 100003, 1 << 20, 1 << 24, (1 << 24) + 1, 1 << 26, (1 << 29) + 3):
        assert ws(n, 5) == 0 and ws(n, 7) == 0, n
        for bits in (4, 8):
            assert ws(n, bits) % 256 == 0 and ws(n, bits) >= keys_only(n, bits) > 0, (n, bits)


@pytest.mark.parametrize("entry", ["dbhip_radix_sort_pairs_u32", "dbhip_radix_sort_pairs_i32"])
def test_argument_errors_need_no_device(entry):
    lib = _capi.lib()
    fn = getattr(lib, entry)
    fake = 1 << 20  # 256-aligned, never dereferenced: every call below fails on the host first
    n = 100003

    def call(keys=fake, vals=fake, tk=fake, tv=fake, n=n, bits=8, ids=0, w=fake, wb=None):
        if wb is None:
            wb = lib.dbhip_radix_sort_pairs_workspace_bytes(n, bits if bits in (4, 8) else 8)
        return fn(keys, vals, tk, tv, n, bits, ids, w, wb, None)

    for ids in (0, 1):  # the argsort never reads vals, but vals is still written: NULL is refused in both modes
        assert call(keys=None, ids=ids) == EINVAL and call(vals=None, ids=ids) == EINVAL
        assert call(tk=None, ids=ids) == EINVAL and call(tv=None, ids=ids) == EINVAL
        assert call(bits=7, ids=ids) == EINVAL and call(bits=5, ids=ids) == EINVAL and call(bits=0, ids=ids) == EINVAL
        for arg in ("keys", "vals", "tk", "tv"):
            assert call(**{arg: fake + 4}, ids=ids) == EINVAL, arg  # 16-byte alignment of all four buffers
            assert call(**{arg: fake + 8}, ids=ids) == EINVAL, arg
        assert call(n=1 << 32, wb=1 << 40, ids=ids) == EINVAL
        for bits in (4, 8):
            wsb = lib.dbhip_radix_sort_pairs_workspace_bytes(n, bits)
            assert call(bits=bits, wb=wsb - 1, ids=ids) == EWORKSPACE
            assert call(bits=bits, w=None, ids=ids) == EWORKSPACE and call(bits=bits, w=fake + 64, ids=ids) == EWORKSPACE
        assert fn(None, None, None, None, 0, 8, ids, None, 0, None) == 0  # nothing to sort
    assert fn(None, None, None, None, 0, 7, 0, None, 0, None) == EINVAL  # bad bits come first, as in the keys-only sort


def test_validator_argument_errors_need_no_device():
    chk = _capi.lib().dbhip_check_sorted_pairs_u32
    fake = 1 << 20
    assert chk(fake, fake, fake, 10, 0, None, None) == EINVAL
    assert chk(None, fake, fake, 10, 0, fake, None) == EINVAL and chk(fake, None, fake, 10, 0, fake, None) == EINVAL
    assert chk(fake, fake, None, 10, 1, fake, None) == EINVAL
    assert chk(fake, fake, fake, 1 << 32, 0, fake, None) == EINVAL  # ids are 32 bits


def test_ops_refuses_unaligned_and_mismatched_columns():
    torch = pytest.importorskip("torch")
    from dwarf_bench_amd import ops
    for name in ("RadixSortPairs", "radix_sort_pairs_", "radix_argsort_", "check_sorted_pairs"):
        assert hasattr(ops, name), name
    t = torch.zeros(17, dtype=torch.int32)
    with pytest.raises(ValueError, match="16-byte"):
        ops._need16(t[1:], "vals")  # what RadixSortPairs.launch applies to both columns
    with pytest.raises(ValueError):
        ops.check_sorted_pairs(t, t, t)  # not on the GPU


def test_pairs_kernels_use_no_scratch_and_keep_the_occupancy(tmp_path):
    """the LDS sum of the pairs scatter (two 32 KiB tiles + counters: two workgroups per CU) assumes four waves per
    SIMD: at most 128 VGPRs and no scratch, in both rank modes and both digit widths"""
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc",
                    "--cuda-device-only", "-S", "-I", str(ROOT / "include"),
                    str(ROOT / "dwarf_bench_amd" / "csrc" / "radix.hip"), "-o", str(tmp_path / "radix.s")],
                   check=True, cwd=tmp_path, timeout=600)
    asm = (tmp_path / "radix.s").read_text()
    meta = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, flags=re.S):
        field = lambda k: int(re.search(rf"\.amdhsa_{k}\s+(\d+)", body).group(1))  # noqa: E731
        meta[name] = (field("group_segment_fixed_size"), field("private_segment_fixed_size"), field("next_free_vgpr"))
    pairs = {k: v for k, v in meta.items() if "rsp_" in k}
    assert len(pairs) == 9, sorted(pairs)  # scatter and one-workgroup sort x {8, 4} bits x {atomic, ballot}, finalize
    assert len(meta) == 18 + 9, sorted(meta)  # the keys-only kernels are all still there
    for name, (lds, scratch, vgprs) in pairs.items():
        assert scratch == 0 and vgprs <= 128, (name, scratch, vgprs)
        assert lds * 2 <= 160 * 1024, (name, lds)
    assert sum("rsp_chunk_scatter" in k for k in pairs) == 4 and sum("rsp_single_tile" in k for k in pairs) == 4
    for name, (lds, scratch, vgprs) in meta.items():  # and the keys-only kernels keep theirs
        assert scratch == 0 and vgprs <= 128, (name, scratch, vgprs)
    bodies = re.findall(r"^(_ZN\S*rsp_\w+):.*?\n(.*?)s_endpgm", asm, flags=re.S | re.M)
    assert len(bodies) == 9 and "scratch_" not in "".join(b for _, b in bodies)
