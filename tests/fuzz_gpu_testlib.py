"""Test-only GPU side of the randomised sweeps (tests/test_gpu_fuzz.py, tools/fuzz_gpu.py): runs a case of
tests/fuzz_testlib.py through its operator's raw entry point on guard_testlib.Watch buffers - every buffer at its drawn
offset, inputs frozen, the case's fill word everywhere - and returns the result fuzz_testlib.check takes.  All calls of a
Sweep share ONE guarded workspace, sized for the largest draw, that starts as random bytes and is never cleared: every
call starts on what a differently shaped call left.  Never imported by the product."""
import numpy as np
import pytest
import torch

from dwarf_bench_amd import _capi
from dwarf_bench_amd import bitpack_native as bn
from dwarf_bench_amd import dict_native as dn
from dwarf_bench_amd import merge_native as mn
from dwarf_bench_amd import ops
from dwarf_bench_amd import select_native as sn
from dwarf_bench_amd import take_native as tn
from tests import fuzz_testlib as ft
from tests import guard_testlib as gt
from tests import take_model as tm
from tests.guard_testlib import Watch, ptr

U = np.uint32
assert ft.FILLS == gt.FILLS


def stream():
    return torch.cuda.current_stream().cuda_stream


def host(t):
    return t.cpu().numpy().view(U).copy()


def dev(a):
    """an aligned device copy, as the tensor front doors take columns"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def i32(p):
    return p - (1 << 32) if p >> 31 else p


def _count(w, value):
    if value is None:
        return None
    d = w.u64(1)
    d.fill_(int(value))
    w.freeze(d)
    return d


def _p(t):
    return ptr(t) if t is not None else None


# ---- workspace bytes and raw calls, per kind of call -----------------------------------------------------------------
def ws_bytes(case):
    what = case["what"]
    if what == "select":
        return sn.workspace_bytes(case["size"])
    if what in ("setop", "merge"):
        return mn.workspace_bytes(case["a"].size, case["b"].size)
    if what == "take":
        return tn.workspace_bytes(case["size"])
    if what == "aggregate":
        return tn.workspace_bytes(case["ws_capacity"])
    if what == "bitpack select":
        return bn.workspace_bytes(case["size"])
    if what == "dict":
        return dn.workspace_bytes(case["capacity"])
    if what == "sort_pairs":
        return int(_capi.lib().dbhip_radix_sort_pairs_workspace_bytes(case["size"], case["bits"]))
    if what == "sorted_search":
        return int(_capi.lib().dbhip_sorted_index_workspace_bytes(case["size"], case["top"]))
    if what == "join_pairs":
        return int(_capi.lib().dbhip_join_pairs_workspace_bytes(case["size"]))
    if what == "topk":
        return int(_capi.lib().dbhip_topk_workspace_bytes(case["size"], case["k"]))
    if what == "reduce_by_key":
        return int(_capi.lib().dbhip_reduce_by_key_workspace_bytes(case["size"]))
    if what == "scan_by_key":
        return int(_capi.lib().dbhip_scan_by_key_workspace_bytes(case["size"]))
    return bn.workspace_bytes(0)


def _kind(name, case):
    return "bitpack select" if name == "bitpack" and case["what"] == "select" else case["what"]


def run_select(case, w, ws, nbytes):
    col, rows, cand, offs = case["col"], case["rows"], case["size"], case["offs"]
    d_col = w.col(col.size, offs["col"], data=col, freeze=True)
    d_rows = w.col(cand, offs["rows"], data=rows, freeze=True) if rows is not None else None
    d_in = _count(w, case["count"])
    d_out, d_cnt = w.col(cand, offs["out"]), w.u64(1)
    rc = sn.select_range(ptr(d_col), col.size, _p(d_rows), _p(d_in), cand if rows is not None else 0, case["lo"], case["hi"],
                         case["flags"], None if case["count_only"] else ptr(d_out), ptr(d_cnt), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    return lambda: dict(out=host(d_out), count=int(d_cnt.item()))


def run_setop(case, w, ws, nbytes):
    a, b, offs = case["a"], case["b"], case["offs"]
    d_a, d_b = w.col(a.size, offs["a"], data=a, freeze=True), w.col(b.size, offs["b"], data=b, freeze=True)
    d_out = w.col(mn.set_bound(case["op"], a.size, b.size), offs["out"])
    d_ac, d_bc, d_oc = _count(w, case["a_count"]), _count(w, case["b_count"]), w.u64(1)
    rc = mn.setop(case["op"], ptr(d_a), _p(d_ac), a.size, ptr(d_b), _p(d_bc), b.size, None if case["count_only"] else ptr(d_out),
                  ptr(d_oc), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    return lambda: dict(out=host(d_out), count=int(d_oc.item()))


def run_merge(case, w, ws, nbytes):
    a, b, offs, mode = case["a"], case["b"], case["offs"], case["mode"]
    d_a, d_b = w.col(a.size, offs["a"], data=a, freeze=True), w.col(b.size, offs["b"], data=b, freeze=True)
    d_av = d_bv = d_ov = None
    if mode == "carried":
        d_av = w.col(a.size, offs["a_vals"], data=case["a_vals"], freeze=True)
        d_bv = w.col(b.size, offs["b_vals"], data=case["b_vals"], freeze=True)
    d_ok = w.col(a.size + b.size, offs["out_keys"])
    if mode != "keys":
        d_ov = w.col(a.size + b.size, offs["out_vals"])
    d_ac, d_bc, d_oc = _count(w, case["a_count"]), _count(w, case["b_count"]), w.u64(1)
    flags = (mn.SIGNED if case["signed"] else 0) | (mn.ROW_IDS if mode == "ids" else 0)
    rc = mn.merge(ptr(d_a), _p(d_av), _p(d_ac), a.size, ptr(d_b), _p(d_bv), _p(d_bc), b.size, flags, ptr(d_ok), _p(d_ov),
                  ptr(d_oc), ptr(ws), nbytes, stream())
    assert rc == 0, rc

    def result():
        res = dict(out_keys=host(d_ok), count=int(d_oc.item()))
        if d_ov is not None:
            res["out_vals"] = host(d_ov)
        return res
    return result


def run_take(case, w, ws, nbytes):
    cols, rows, capacity, offs = case["cols"], case["rows"], case["size"], case["offs"]
    d_cols = [w.col(col.size, offs[f"col{c}"], data=col, freeze=True) for c, col in enumerate(cols)]
    d_rows, d_count = w.col(capacity, offs["rows"], data=rows, freeze=True), _count(w, case["count"])
    d_outs = [w.col(capacity, offs[f"out{c}"]) for c in range(len(cols))]
    rc = tn.take([ptr(c) for c in d_cols], len(cols), cols[0].size, ptr(d_rows), _p(d_count), capacity, case["flags"],
                 case["fill_word"], [ptr(o) for o in d_outs], ptr(ws), nbytes, stream())
    assert rc == 0, rc
    return lambda: dict(outs=[host(o) for o in d_outs])


def run_aggregate(case, w, ws, nbytes):
    col, rows, offs = case["cols"][0], case["rows"], case["offs"]
    d_col = w.col(col.size, offs["col0"], data=col, freeze=True)
    d_rows = w.col(case["size"], offs["rows"], data=rows, freeze=True) if rows is not None else None
    d_count, d_out = _count(w, case["count"]), w.u64(4)
    rc = tn.aggregate(ptr(d_col), col.size, _p(d_rows), _p(d_count), case["size"] if rows is not None else 0, case["flags"],
                      ptr(d_out), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    return lambda: dict(words=tuple(int(x) & tm.M64 for x in d_out.tolist()))


def run_pack(case, w, ws, nbytes):
    col, width = case["col"], case["width"]
    d_col = w.col(col.size, case["offs"]["col"], data=col, freeze=True)
    d_count = _count(w, case["count"])
    d_out = w.col(bn.words(col.size, width) + ft.SPARE_WORDS, 0)
    rc = bn.pack(ptr(d_col), col.size, _p(d_count), width, case["base"], ptr(d_out), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    return lambda: dict(out=host(d_out))


def _packed(case, w):
    words = bn.words(case["n_rows"], case["width"])
    return w.col(words, 0, data=case["packed"][:words], freeze=True)  # exactly its words, on a 16-byte boundary


def run_unpack(case, w, ws, nbytes):
    rows, n_rows, offs = case["rows"], case["n_rows"], case["offs"]
    d_packed = _packed(case, w)
    d_rows = w.col(case["size"], offs["rows"], data=rows, freeze=True) if rows is not None else None
    d_count, d_out = _count(w, case["count"]), w.col(case["size"], offs["out"])
    rc = bn.unpack(ptr(d_packed) if n_rows else None, n_rows, case["width"], case["base"], _p(d_rows), _p(d_count),
                   case["size"] if rows is not None else 0, case["flags"], case["fill_word"], ptr(d_out), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    return lambda: dict(out=host(d_out))


def run_bitpack_select(case, w, ws, nbytes):
    rows, n_rows, offs = case["rows"], case["n_rows"], case["offs"]
    d_packed = _packed(case, w)
    d_rows = w.col(case["size"], offs["rows"], data=rows, freeze=True) if rows is not None else None
    d_count, d_out, d_total = _count(w, case["count"]), w.col(case["size"], offs["out"]), w.u64(1)
    rc = bn.select_range(ptr(d_packed) if n_rows else None, n_rows, case["width"], case["base"], _p(d_rows), _p(d_count),
                         case["size"] if rows is not None else 0, case["lo"], case["hi"], case["flags"],
                         None if case["count_only"] else ptr(d_out), ptr(d_total), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    return lambda: dict(out=host(d_out), count=int(d_total.item()))


def run_dict(case, w, ws, nbytes):
    """the build, its status read, then the encode through the workspace the build left: it may only read it"""
    col, probe, offs = case["col"], case["probe"], case["offs"]
    d_col, d_count = w.col(col.size, offs["col"], data=col, freeze=True), _count(w, case["count"])
    d_keys, d_distinct = w.col(case["capacity"], offs["keys"]), w.u64(1)
    rc = dn.build(ptr(d_col), col.size, _p(d_count), case["capacity"], case["flags"], ptr(d_keys), ptr(d_distinct), ptr(ws),
                  nbytes, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    status, held = ops.workspace_status(ws), ws[:nbytes].clone()
    d_probe, d_pc = w.col(probe.size, offs["probe"], data=probe, freeze=True), _count(w, case["probe_count"])
    d_codes, d_miss = w.col(probe.size, offs["codes"]), (w.u64(1) if case["want_misses"] else None)
    rc = dn.encode(ptr(d_probe), probe.size, _p(d_pc), ptr(d_codes), _p(d_miss), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert torch.equal(ws[:nbytes], held), "encode wrote the dictionary's workspace"
    assert ops.workspace_status(ws) == status
    return lambda: dict(keys=host(d_keys), distinct=int(d_distinct.item()), codes=host(d_codes),
                        misses=int(d_miss.item()) if d_miss is not None else None)


def run_topk(case, w, ws, nbytes):
    keys, k = case["keys"], case["k"]
    d_keys = w.col(keys.size, data=keys, freeze=True)
    out_keys, out_rows = w.col(k), w.col(k)
    fn = _capi.lib().dbhip_topk_i32 if case["signed"] else _capi.lib().dbhip_topk_u32
    rc = fn(ptr(d_keys), keys.size, k, int(case["largest"]), int(case["sorted"]), ptr(out_keys), ptr(out_rows), ptr(ws), nbytes,
            stream())
    assert rc == 0, rc
    return lambda: dict(out_keys=host(out_keys), out_rows=host(out_rows))


def _by_key_outputs(case, w, names, entries):
    return {name: (w.u64(entries) if name == "sums" else w.col(entries)) for name in case["cols"]}


def _read_by_key(out):
    return {name: (t.cpu().numpy().view(np.uint64).copy() if name == "sums" else host(t)) for name, t in out.items()}


def run_reduce_by_key(case, w, ws, nbytes):
    n, cap = case["size"], case["capacity"]
    d_keys, d_vals = w.col(n, data=case["keys"], freeze=True), w.col(n, data=case["vals"], freeze=True)
    out, runs = _by_key_outputs(case, w, ft.RBK_NAMES, cap), w.u64(1)
    rc = _capi.lib().dbhip_reduce_by_key_u32(ptr(d_keys), ptr(d_vals) if case["with_vals"] else None, n, int(case["signed"]),
                                             *[_p(out.get(name)) for name in ft.RBK_NAMES], cap, ptr(runs), ptr(ws), nbytes,
                                             stream())
    assert rc == 0, rc
    return lambda: dict(_read_by_key(out), runs=int(runs.item()))


def run_scan_by_key(case, w, ws, nbytes):
    n = case["size"]
    d_keys, d_vals = w.col(n, data=case["keys"], freeze=True), w.col(n, data=case["vals"], freeze=True)
    out = _by_key_outputs(case, w, ft.SBK_NAMES, n)
    rc = _capi.lib().dbhip_scan_by_key_u32(ptr(d_keys), ptr(d_vals) if case["with_vals"] else None, n, int(case["signed"]),
                                           *[_p(out.get(name)) for name in ft.SBK_NAMES], ptr(ws), nbytes, stream())
    assert rc == 0, rc
    return lambda: _read_by_key(out)


def run_sort_pairs(case, w, ws, nbytes):
    """in place: the two columns are inputs and outputs, the two ping-pong buffers scratch; all four guarded"""
    n = case["size"]
    d_keys, d_vals = w.col(n, data=case["keys"]), w.col(n, data=None if case["argsort"] else case["vals"])
    tmp_keys, tmp_vals = w.col(n), w.col(n)
    fn = _capi.lib().dbhip_radix_sort_pairs_i32 if case["signed"] else _capi.lib().dbhip_radix_sort_pairs_u32
    rc = fn(ptr(d_keys), ptr(d_vals), ptr(tmp_keys), ptr(tmp_vals), n, case["bits"], int(case["argsort"]), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    return lambda: dict(keys=host(d_keys), vals=host(d_vals))


def run_sorted_search(case, w, ws, nbytes):
    """the index built into the shared workspace, then the search through it"""
    col, lo, hi, m = case["sorted"], case["lo"], case["hi"], case["size"]
    n = (lo if lo is not None else hi).size
    d_col = w.col(m, case["offs"]["sorted"], data=col, freeze=True)
    d_lo = w.col(n, data=lo, freeze=True) if lo is not None else None
    d_hi = w.col(n, data=hi, freeze=True) if hi is not None else None
    d_pos = w.col(n) if "pos" in case["outputs"] else None
    d_cnt = w.col(n) if "cnt" in case["outputs"] else None
    lib = _capi.lib()
    rc = lib.dbhip_sorted_index_build_u32(ptr(d_col), m, int(case["signed"]), case["top"], ptr(ws), nbytes, stream())
    assert rc == 0, rc
    rc = lib.dbhip_sorted_search_u32(ptr(d_col), m, _p(d_lo), _p(d_hi), n, _p(d_pos), _p(d_cnt), ptr(ws), nbytes, stream())
    assert rc == 0, rc

    def result():
        res = {}
        if d_pos is not None:
            res["pos"] = host(d_pos)
        if d_cnt is not None:
            res["cnt"] = host(d_cnt)
        return res
    return result


def run_join_pairs(case, w, ws, nbytes):
    offs, cap, n_probe = case["offs"], case["capacity"], case["size"]
    d_ids = w.col(case["ids"].size, offs["ids"], data=case["ids"], freeze=True)
    d_pos = w.col(n_probe, offs["pos"], data=case["pos"], freeze=True)
    d_cnt = w.col(n_probe, offs["cnt"], data=case["cnt"], freeze=True)
    d_rid = w.col(n_probe, offs["rid"], data=case["rid"], freeze=True) if case["rid"] is not None else None
    out_b, out_p = (w.col(cap, offs["out_build"]), w.col(cap, offs["out_probe"])) if cap else (None, None)
    total = w.u64(1)
    rc = _capi.lib().dbhip_join_pairs_u32(ptr(d_ids), case["ids"].size, _p(d_rid), ptr(d_pos), ptr(d_cnt), n_probe,
                                          int(case["left_outer"]), cap, _p(out_b), _p(out_p), ptr(total), ptr(ws), nbytes, stream())
    assert rc == 0, rc
    empty = np.zeros(0, U)
    return lambda: dict(out_build=host(out_b) if cap else empty, out_probe=host(out_p) if cap else empty,
                        total=int(total.item()) & ((1 << 64) - 1))


RAW = {"sort_pairs": run_sort_pairs, "sorted_search": run_sorted_search, "join_pairs": run_join_pairs, "topk": run_topk, "reduce_by_key": run_reduce_by_key, "scan_by_key": run_scan_by_key, "dict": run_dict, "select": run_select, "setop": run_setop, "merge": run_merge, "take": run_take, "aggregate": run_aggregate,
       "pack": run_pack, "unpack": run_unpack, "bitpack select": run_bitpack_select}


# ---- the tensor front doors: the case cut to its counts, on aligned copies -------------------------------------------
def _cut(case, field, count):
    return case[field][: ft.counted(case[count], case[field].size)]


def _raises_or(status, call):
    """a device status makes the eager front doors raise"""
    if status:
        with pytest.raises(ops._capi.DbhipError):
            call()
        return None
    return call()


def door_select(op, case):
    if not case["size"] or not case["col"].size:
        return
    cut = dict(case, rows=None if case["rows"] is None else _cut(case, "rows", "count"), count=None, count_only=False)
    cut["size"] = case["size"] if cut["rows"] is None else cut["rows"].size
    if not cut["size"]:
        return
    want = op.model(cut)
    lo, hi = (i32(case["lo"]), i32(case["hi"])) if case["signed"] else (case["lo"], case["hi"])
    got = _raises_or(want["status"], lambda: ops.select_range(dev(case["col"]), lo, hi, None if cut["rows"] is None else dev(cut["rows"]),
                                                               signed=case["signed"], negate=case["negate"]))
    if got is not None:
        assert np.array_equal(host(got), want["out"][: want["count"]])


def door_merge(op, case):
    a, b = _cut(case, "a", "a_count"), _cut(case, "b", "b_count")
    if not a.size or not b.size:
        return
    cut = dict(case, a=a, b=b, a_count=None, b_count=None, count_only=False)
    if case["what"] == "setop":
        want = op.model(cut)
        got = (ops.union_rows, ops.intersect_rows, ops.difference_rows)[case["op"]](dev(a), dev(b))
        assert np.array_equal(host(got), want["out"][: want["count"]])
        return
    cut.update(a_vals=case["a_vals"][: a.size], b_vals=case["b_vals"][: b.size])
    want = op.model(cut)
    carried = case["mode"] == "carried"
    keys, vals = ops.merge_sorted(dev(a), dev(b), dev(cut["a_vals"]) if carried else None, dev(cut["b_vals"]) if carried else None,
                                  signed=case["signed"], row_ids=case["mode"] == "ids")
    assert np.array_equal(host(keys), want["out_keys"]) and (vals is None) == (case["mode"] == "keys")
    assert vals is None or np.array_equal(host(vals), want["out_vals"])


def door_take(op, case):
    if not case["cols"][0].size or (case["rows"] is not None and not ft.counted(case["count"], case["size"])):
        return
    rows = None if case["rows"] is None else _cut(case, "rows", "count")
    cut = dict(case, rows=rows, count=None, size=case["size"] if rows is None else rows.size)
    want = op.model(cut)
    if case["what"] == "take":
        got = _raises_or(want["status"], lambda: ops.take([dev(c) for c in case["cols"]], dev(rows), outer=case["outer"],
                                                          fill=case["fill_word"]))
        if got is not None:
            assert all(np.array_equal(host(g), o) for g, o in zip(got, want["outs"]))
    else:
        got = _raises_or(want["status"], lambda: ops.aggregate_rows(dev(case["cols"][0]), None if rows is None else dev(rows),
                                                                    signed=case["signed"], outer=case["outer"]))
        if got is not None:
            assert got == tm.as_ints(want["words"], case["signed"])


def door_bitpack(op, case):
    width, base = case["width"], case["base"]
    if case["what"] == "pack":
        col = _cut(case, "col", "count")
        if not col.size:
            return
        want = op.model(dict(case, col=col, count=None))
        got = _raises_or(want["status"], lambda: ops.pack(dev(col), width, base))
        if got is not None:
            assert np.array_equal(host(got.packed), want["out"][: bn.words(col.size, width)])
        return
    if not case["n_rows"]:
        return
    rows = None if case["rows"] is None else _cut(case, "rows", "count")
    if rows is not None and not rows.size:
        return
    cut = dict(case, rows=rows, count=None, count_only=False, size=case["size"] if rows is None else rows.size)
    want = op.model(cut)
    pc = ops.PackedColumn(dev(case["packed"]), case["n_rows"], width, base)
    d_rows = None if rows is None else dev(rows)
    if case["what"] == "unpack":
        got = _raises_or(want["status"], lambda: ops.unpack(pc, d_rows, outer=case["outer"], fill=case["fill_word"]))
        if got is not None:
            assert np.array_equal(host(got), want["out"])
    else:
        lo, hi = (i32(case["lo"]), i32(case["hi"])) if case["signed"] else (case["lo"], case["hi"])
        got = _raises_or(want["status"], lambda: ops.select_range_packed(pc, lo, hi, d_rows, signed=case["signed"],
                                                                          negate=case["negate"]))
        if got is not None:
            assert np.array_equal(host(got), want["out"][: want["count"]])


def door_dict(op, case):
    col = _cut(case, "col", "count")
    probe = _cut(case, "probe", "probe_count")
    if not col.size:
        return
    want = op.model(dict(case, col=col, count=None, probe=probe, probe_count=None))
    plan = ops.Dictionary(col.size, case["capacity"])
    plan.build(dev(col), signed=case["signed"])
    assert plan.status() == want["status"]
    if want["status"]:
        with pytest.raises(ops._capi.DbhipError):
            plan.result()
    else:
        assert np.array_equal(host(plan.result()), want["keys"][: want["distinct"]])
    if probe.size:
        assert np.array_equal(host(plan.encode(dev(probe))), want["codes"])
    if not want["status"]:
        codes, uniques = ops.factorize(dev(col), signed=case["signed"], capacity=case["capacity"])
        assert np.array_equal(host(uniques), want["keys"][: want["distinct"]]) and np.array_equal(host(uniques)[host(codes)], col)


def door_topk(op, case):
    if not case["size"]:
        return
    want = op.model(case)
    m = min(case["k"], case["size"])
    keys, rows = ops.topk(dev(case["keys"]), case["k"], case["largest"], case["signed"], case["sorted"])
    assert np.array_equal(host(keys), want["out_keys"][:m]) and np.array_equal(host(rows), want["out_rows"][:m])


def door_reduce_by_key(op, case):
    if not case["size"]:
        return
    want = ft.rbm.reduce_by_key(case["keys"], case["vals"], case["signed"])
    got = ops.reduce_by_key(dev(case["keys"]), dev(case["vals"]), signed=case["signed"])
    for g, w_ in zip(got, want):
        assert np.array_equal(g.cpu().numpy().view(w_.dtype), w_)


def door_scan_by_key(op, case):
    if not case["size"]:
        return
    want = ft.sbm.scan_by_key(case["keys"], case["vals"], case["signed"])
    got = ops.scan_by_key(dev(case["keys"]), dev(case["vals"]), signed=case["signed"])
    for g, w_ in zip(got, want):
        assert np.array_equal(g.cpu().numpy().view(w_.dtype), w_)


def door_sort_pairs(op, case):
    if not case["size"]:
        return
    want = op.model(case)
    keys = dev(case["keys"])
    if case["argsort"]:
        vals = ops.radix_argsort_(keys, signed=case["signed"], radix_bits=case["bits"])
    else:
        _, vals = ops.radix_sort_pairs_(keys, dev(case["vals"]), signed=case["signed"], radix_bits=case["bits"])
    assert np.array_equal(host(keys), want["keys"]) and np.array_equal(host(vals)[: case["size"]], want["vals"])


def door_sorted_search(op, case):
    """ops.sorted_search on the column, and ops.range_join on a shuffled copy of it against the model's join"""
    lo, hi = case["lo"], case["hi"]
    n = (lo if lo is not None else hi).size
    if not case["size"] or not n:
        return
    want = ft.ssm.search(case["sorted"], lo, hi, case["signed"])
    pos, cnt = ops.sorted_search(dev(case["sorted"]), None if lo is None else dev(lo), None if hi is None else dev(hi),
                                 signed=case["signed"])
    assert np.array_equal(host(pos), want[0]) and np.array_equal(host(cnt), want[1])
    if int(want[1].astype(np.int64).sum()) > 1 << 20:
        return
    build = case["sorted"][np.random.default_rng(case["draw"]).permutation(case["size"])]
    for left_outer in (False, True):
        want_b, want_p = ft.ssm.range_join(build, lo, hi, case["signed"], left_outer)
        got_b, got_p = ops.range_join(dev(build), None if lo is None else dev(lo), None if hi is None else dev(hi),
                                      left_outer=left_outer, signed=case["signed"])
        assert np.array_equal(host(got_b), want_b) and np.array_equal(host(got_p), want_p)


def door_join_pairs(op, case):
    """ops.join_pairs on the key columns, probe rows ascending: the pairs of the model at full capacity, without rid"""
    if case["build"] is None or not case["size"] or not case["build"].size:
        return
    want = op.model(dict(case, rid=None, capacity=case["total"]))
    got_b, got_p = ops.join_pairs(dev(case["build"]), dev(case["probe"]), left_outer=case["left_outer"], ordered=True)
    pack = lambda b, p: np.sort(p.astype(np.uint64) << np.uint64(32) | b.astype(np.uint64))  # noqa: E731
    assert np.array_equal(host(got_p), want["out_probe"])
    assert np.array_equal(pack(host(got_b), host(got_p)), pack(want["out_build"], want["out_probe"]))


DOORS = {"sort_pairs": door_sort_pairs, "sorted_search": door_sorted_search, "join_pairs": door_join_pairs, "topk": door_topk, "reduce_by_key": door_reduce_by_key, "scan_by_key": door_scan_by_key, "dict": door_dict, "select": door_select, "merge": door_merge, "take": door_take, "bitpack": door_bitpack}


# ---- a sweep ---------------------------------------------------------------------------------------------------------
class Sweep:
    """the calls of one operator on one guarded workspace that is never cleared between them"""

    def __init__(self, name, ws_nbytes, seed=0):
        self.name, self.op = name, ft.OPERATORS[name]
        self.calls, self.doors = getattr(self, "calls", 0), getattr(self, "doors", 0)
        self.ws_fill = gt.FILLS[0]
        self.base, self.ws = gt.guarded_bytes(max(ws_nbytes, 256), self.ws_fill)
        gen = torch.Generator(device="cuda").manual_seed(seed)
        self.ws.copy_(torch.randint(0, 256, (self.ws.numel(),), dtype=torch.uint8, device="cuda", generator=gen))

    def run(self, case):
        """one raw call -> the result; the guards of every buffer and of the workspace, and the frozen inputs, checked"""
        nbytes = ws_bytes(dict(case, what=_kind(self.name, case)))
        if nbytes > self.ws.numel():  # (an open-ended stream of draws: a larger workspace, random bytes again)
            self.__init__(self.name, nbytes, self.calls)
        w = Watch(case["fill"])
        read = RAW[_kind(self.name, case)](case, w, self.ws, nbytes)
        torch.cuda.synchronize()
        status = ops.workspace_status(self.ws)
        w.check()
        gt.assert_byte_guards(self.base, self.ws, self.ws_fill)
        self.calls += 1
        return dict(read(), status=status)

    def step(self, case):
        """the raw call checked against the model; every fourth draw also through the tensor front door, on aligned
        copies of the inputs cut to their counts"""
        self.op.check(case, self.run(case))
        if case["draw"] % 4 == 0:
            DOORS[self.name](self.op, case)
            self.doors += 1


def sweep(name, seed=None):
    """every draw of the operator's seeded set, once -> the Sweep"""
    op = ft.OPERATORS[name]
    need = max(ws_bytes(dict(c, what=_kind(name, c))) for c in op.cases(seed))
    s = Sweep(name, need, op.seed if seed is None else seed)
    for case in op.cases(seed):
        try:
            s.step(case)
        except AssertionError as e:
            raise AssertionError(f"{name} draw {case['draw']} ({describe(case)}): {e}") from e
    return s


def describe(case):
    """a draw's parameters without its arrays"""
    return {k: (v if not isinstance(v, np.ndarray) else f"<{v.size}>") for k, v in case.items()
            if not (isinstance(v, list) and v and isinstance(v[0], np.ndarray))}


# ---- random query plans: every count stays on the device until the end ---------------------------------------------------
def run_plan(plan):
    """the steps of a plan of fuzz_testlib.plan_draws through the ops plans, nothing read back in between -> one answer
    per step, in the form of fuzz_testlib.plan_model, read after ONE synchronisation at the end"""
    n = plan["n"]
    d_cols = [dev(c) for c in plan["cols"]]
    packed = {}
    lists, readers, plans = [], [], []

    def bounds(s):
        return (i32(s["lo"]), i32(s["hi"])) if s["signed"] else (s["lo"], s["hi"])

    def listed(rows, count):
        lists.append((rows, count))
        readers.append(lambda: host(rows)[: int(count.item())])

    for s in plan["steps"]:
        c, kind = s["col"], s["step"]
        if kind in ("select", "refine", "packed"):
            rows, count = (None, None) if kind == "select" or (kind == "packed" and s["dense"]) else lists[s["list"]]
            sel = ops.SelectRows(n if rows is None else rows.numel())
            col = d_cols[c]
            if kind == "packed":
                if c not in packed:  # width and base known beforehand: the pack is one launch, nothing read back
                    host_col = plan["cols"][c]
                    base = int(host_col.min())
                    pack = ops.BitPack(n, max(1, (int(host_col.max()) - base).bit_length()), base)
                    pack.launch(col)
                    packed[c] = pack
                col = packed[c].output()
            lo, hi = bounds(s)
            sel.launch(col, lo, hi, rows=rows, count=count, signed=s["signed"], negate=s["negate"])
            plans.append(sel)
            listed(*sel.output())
        elif kind == "setop":
            (a, ca), (b, cb) = lists[s["list"]], lists[s["other"]]
            sets = ops.RowSets(a.numel(), b.numel())
            sets.launch(s["op"], a, b, ca, cb)
            plans.append(sets)
            listed(sets.rows[: a.numel() + b.numel()], sets.out_count)
        elif kind == "take":
            rows, count = lists[s["list"]]
            taker = ops.TakeRows(rows.numel(), 1)
            taker.launch(d_cols[c], rows, count)
            plans.append(taker)
            readers.append(lambda taker=taker, count=count: host(taker.output()[0][0])[: int(count.item())])
        elif kind == "aggregate":
            rows, count = lists[s["list"]]
            agg = ops.AggregateRows(rows.numel())
            agg.launch(d_cols[c], rows, count, signed=s["signed"])
            plans.append(agg)
            readers.append(lambda agg=agg: tuple(int(x) & tm.M64 for x in agg.output().tolist()))
        else:  # the values of a list, encoded through their own dictionary and decoded again
            rows, count = lists[s["list"]]
            taker, back = ops.TakeRows(rows.numel(), 1), ops.TakeRows(rows.numel(), 1)
            taker.launch(d_cols[c], rows, count)
            values = taker.output()[0][0]
            book = ops.Dictionary(rows.numel())
            book.build(values, count, signed=s["signed"])
            codes = book.encode(values, count)
            back.launch(book.keys, codes, count, outer=True)
            plans += [taker, back, book]
            readers.append(lambda codes=codes, back=back, count=count: (host(codes)[: int(count.item())],
                                                                         host(back.output()[0][0])[: int(count.item())]))
    torch.cuda.synchronize()
    assert all(p.status() == 0 for p in plans)
    return [read() for read in readers]


check_plan = ft.check_plan


def endless(name, seed):
    """the operator's draw sets under seed, seed + 1, ... one after the other, for a time-budgeted loop"""
    while True:
        yield from ft.OPERATORS[name].cases(seed)
        seed += 1
