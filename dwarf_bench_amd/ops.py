"""Tensor-level front door to the gfx950 dwarf kernels.

PyTorch is plumbing here (device memory, the current HIP stream, torch.distributed); every op is one or
more calls through a C ABI into hand-written gfx950 kernels: that of include/dbhip*.h into libdbhip.so, and for the
selection vectors (SelectRows, select_range, semi_join) that of host/select_rows.hpp into libdbench.so, where entry
points live until they are promoted to include/ (INTEGRATION.md); beside it, for the sorted merge and the set
operations on row-id lists (MergeSorted, merge_sorted, RowSets, union_rows, intersect_rows, difference_rows, select_any),
that of host/merge_sorted.hpp, and for late materialisation through a row-id list (TakeRows, take, AggregateRows,
aggregate_rows) that of host/take_rows.hpp, and for dictionary encoding (Dictionary, factorize, dict_combine,
encode_columns, and the two compositions over several key columns, groupby_columns and join_pairs_columns) that of
host/dict_encode.hpp, and for bit-packed columns (PackedColumn, BitPack, pack, unpack, select_range_packed, and SelectRows on
a PackedColumn) that of host/bitpack.hpp, and for the Bloom filter (BloomFilter, bloom_words, bloom_build, select_in_bloom,
SelectRows.launch_in and refine_in, semi_join with bloom_bits) that of host/bloom_filter.hpp, and for approximate distinct
counts (HyperLogLog, approx_count_distinct, hll_relative_error) that of host/hll_sketch.hpp, and for exact order statistics
(Quantiles, quantiles, kth_value, median, equi_depth_bounds) that of host/quantile_select.hpp.  Nothing in this module computes on the host or falls back to torch ops: without the built libraries
the first call raises.
"""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import torch

from . import (_capi, bitpack_native, bloom_native, dict_native, hll_native, merge_native, quantile_native, select_native,
               take_native)

DEV_OK, DEV_SPIN_TIMEOUT, DEV_KEY_RANGE, DEV_TABLE_FULL, DEV_RANK_ORDER = 0, 1, 2, 4, 8


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need(t: torch.Tensor, dtype: torch.dtype, name: str) -> None:
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor on the GPU, got {t.dtype} on {t.device}")


def _need16(t: torch.Tensor, name: str) -> None:
    """radix sort and group-by read their columns with 16-byte loads (include/dbhip.h): a slice like t[1:] is refused"""
    if t.numel() and t.data_ptr() % 16:
        raise ValueError(f"{name}: the column must start on a 16-byte boundary (got offset {t.data_ptr() % 16}); "
                         "copy the slice with .clone() first")


def _ws(nbytes: int, device) -> torch.Tensor:
    # torch's caching allocator hands out >= 512-byte aligned blocks; the C ABI asks for 256.  Zeroed: an entry
    # point that returns early (n == 0) must not leave an uninitialised status word behind.
    return torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def workspace_status(ws: torch.Tensor) -> int:
    """Device-side status word of a workspace (synchronises the current stream)."""
    st = C.c_uint32(0xFFFFFFFF)
    _capi.check(_capi.lib().dbhip_workspace_status(ws.data_ptr(), C.byref(st), _stream()), "workspace_status")
    return st.value


def _check_status(ws: torch.Tensor, what: str) -> None:
    st = workspace_status(ws)
    if st != DEV_OK:
        raise _capi.DbhipError(f"{what}: device status {st:#x}")


def device_info(device: int = 0):
    name = C.create_string_buffer(64)
    cus, wave = C.c_int(0), C.c_int(0)
    _capi.check(_capi.lib().dbhip_device_info(device, name, 64, C.byref(cus), C.byref(wave)), "device_info")
    return name.value.decode(), cus.value, wave.value


# ---------------------------------------------------------------------------------------------
# deterministic synthetic columns
# ---------------------------------------------------------------------------------------------
def gen_uniform_u32(n: int, seed: int, lo: int, hi: int, first_index: int = 0, device="cuda",
                    dtype: torch.dtype = torch.int32) -> torch.Tensor:
    """lo + mix64(seed, first_index + i) % (hi - lo + 1); dtype int32 reinterprets the uint32 bits."""
    out = torch.empty(n, dtype=dtype, device=device)
    _capi.check(_capi.lib().dbhip_gen_uniform_u32(out.data_ptr(), n, seed, first_index, lo, hi, _stream()),
                "gen_uniform_u32")
    return out


def gen_unique_sorted_u32(n: int, seed: int, first_index: int = 0, device="cuda") -> torch.Tensor:
    out = torch.empty(n, dtype=torch.int32, device=device)
    _capi.check(_capi.lib().dbhip_gen_unique_sorted_u32(out.data_ptr(), n, seed, first_index, _stream()),
                "gen_unique_sorted_u32")
    return out


# ---------------------------------------------------------------------------------------------
# dwarf 1: scan / compaction
# ---------------------------------------------------------------------------------------------
class CopyIfLt:
    """Reusable plan for out = [x in src : x < filter]: owns workspace + output buffers for a size."""

    def __init__(self, n: int, device="cuda"):
        self.n = n
        lib = _capi.lib()
        self.ws_bytes = lib.dbhip_copy_if_lt_i32_workspace_bytes(n)
        self.ws = _ws(self.ws_bytes, device)
        self.out = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        self.out_size = torch.zeros(1, dtype=torch.int64, device=device)
        self._seen: dict[int, float] = {}
        self._last_filter = None

    # selectivity from which the single-launch dense variant is the faster one.  2^28 rows (tools/ab.py scan), two runs:
    # s = 2.5 % two-launch 220 / dense 240 us, 5 % 242 / 240 and 218 / 242, 7.5 % 255 / 241, 10 % 265 / 242 and 241 / 246,
    # 25 % 328 / 258 and 312 / 260 — the dense variant is the same from run to run, the two-launch one is not (its staging
    # traffic), and they cross somewhere between 5 % and 10 %
    DENSE_ABOVE = 0.075

    def launch(self, src: torch.Tensor, filter_value: int, dense: bool | None = None) -> None:
        """Asynchronous on the current stream; nothing is read back.  dense: True / False pick the variant
        (dbhip_copy_if_lt_dense_i32 / dbhip_copy_if_lt_i32); None = by the selectivity the last result() saw for this
        filter value (the first call of a plan takes the two-launch path)."""
        _need(src, torch.int32, "src")
        if src.numel() != self.n:
            raise ValueError("size mismatch")
        if dense is None:
            dense = self._seen.get(filter_value, 0.0) > self.DENSE_ABOVE
        fn = _capi.lib().dbhip_copy_if_lt_dense_i32 if dense else _capi.lib().dbhip_copy_if_lt_i32
        self._last_filter = filter_value
        _capi.check(fn(src.data_ptr(), self.n, filter_value, self.out.data_ptr(), self.out_size.data_ptr(),
                       self.ws.data_ptr(), self.ws_bytes, _stream()), "copy_if_lt_i32")

    def result(self) -> torch.Tensor:
        _check_status(self.ws, "copy_if_lt_i32")
        m = int(self.out_size.item())
        if self._last_filter is not None and self.n:
            self._seen[self._last_filter] = m / self.n
        return self.out[:m]


def copy_if_lt(src: torch.Tensor, filter_value: int, dense: bool = False) -> torch.Tensor:
    plan = CopyIfLt(src.numel(), src.device)
    plan.launch(src, filter_value, dense=dense)
    return plan.result()


# ---------------------------------------------------------------------------------------------
# selection vectors: range filters that return row ids (host/select_rows.hpp, libdbench.so)
# ---------------------------------------------------------------------------------------------
def _bounds(lo: int, hi: int, signed: bool) -> tuple[int, int]:
    """Python ints in the range of the chosen signedness -> their 32-bit patterns"""
    least, most = (-(1 << 31), (1 << 31) - 1) if signed else (0, (1 << 32) - 1)
    for name, v in (("lo", lo), ("hi", hi)):
        if isinstance(v, bool) or not isinstance(v, int) or not least <= v <= most:
            raise ValueError(f"{name}: expected an int in [{least}, {most}] ({'int32' if signed else 'uint32'}), got {v!r}")
    return lo & 0xFFFFFFFF, hi & 0xFFFFFFFF


class SelectRows:
    """Reusable plan for row ids under range predicates, up to `capacity` candidates per call: owns the workspace, two
    row-id buffers (ping-pong: a call never writes the buffer it reads, and the view result() returned last stays intact
    through the next call) and their device counts.  launch() filters all rows of a column or a given row-id list;
    refine() filters the plan's own last output on another column with its count still on the device, so a conjunction
    is a chain of launches without a read-back.  Row ids come out in candidate order."""

    def __init__(self, capacity: int, device="cuda"):
        self.capacity = int(capacity)
        self.ws_bytes = select_native.workspace_bytes(self.capacity)
        if self.ws_bytes == 0:
            raise ValueError("capacity: at most 2^32 - 1 candidates")
        # one workspace for plain and packed columns: whichever query is larger
        self.ws_bytes = max(self.ws_bytes, bitpack_native.workspace_bytes(self.capacity))
        self.ws = _ws(self.ws_bytes, device)
        self.rows = [torch.empty(max(self.capacity, 1), dtype=torch.int32, device=device) for _ in range(2)]
        self.counts = torch.zeros(2, dtype=torch.int64, device=device)
        self._last = None  # index of the buffer the last launch wrote

    def launch(self, col, lo: int, hi: int, rows: torch.Tensor | None = None,
               count: torch.Tensor | None = None, signed: bool = False, negate: bool = False) -> None:
        """Asynchronous on the current stream; nothing is read back.  col: an int32 column, or a PackedColumn, which is
        filtered in its packed form (lo and hi are values, not codes).  rows: an int32 row-id list (None: all rows of
        col); count: a device int64 of one element, the number of entries of `rows` that count (None: all of them)."""
        packed = col if isinstance(col, PackedColumn) else None
        if packed is not None:
            col = _need_packed(packed, "col")  # the packed words; the row count comes from the column itself
        else:
            _need(col, torch.int32, "col")
        lo, hi = _bounds(lo, hi, signed)
        if rows is not None:
            _need(rows, torch.int32, "rows")
        elif count is not None:
            raise ValueError("count: given without rows")
        if count is not None and (not count.is_cuda or count.dtype != torch.int64 or count.numel() != 1):
            raise ValueError("count: expected one int64 on the GPU")
        n_col = col.numel() if packed is None else packed.n_rows
        candidates = n_col if rows is None else rows.numel()
        if candidates > self.capacity:
            raise ValueError(f"{candidates} candidates, the plan holds {self.capacity}")
        into = 0 if self._last is None else 1 - self._last
        if rows is not None and rows.untyped_storage().data_ptr() == self.rows[into].untyped_storage().data_ptr():
            into = 1 - into  # the list is a view of that buffer: write the other one
        col_ptr, col_n, list_ptr, count_ptr = col.data_ptr() if n_col else None, n_col, None, None
        if rows is not None and rows.numel():
            list_ptr, count_ptr = rows.data_ptr(), count.data_ptr() if count is not None else None
        elif rows is not None:  # an empty list has no address: the call over no rows at all
            col_ptr, col_n = None, 0
        if packed is not None:
            flags = (bitpack_native.SIGNED if signed else 0) | (bitpack_native.NEGATE if negate else 0)
            _capi.check(bitpack_native.select_range(
                col_ptr, col_n, packed.width, packed.base, list_ptr, count_ptr, rows.numel() if list_ptr else 0, lo, hi,
                flags, self.rows[into].data_ptr(), self.counts[into:].data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                _stream()), "bitpack_select_range_u32")
            self._last = into
            return
        flags = (select_native.SIGNED if signed else 0) | (select_native.NEGATE if negate else 0)
        _capi.check(select_native.select_range(
            col_ptr, col_n, list_ptr, count_ptr, rows.numel() if list_ptr else 0, lo, hi, flags,
            self.rows[into].data_ptr(), self.counts[into:].data_ptr(), self.ws.data_ptr(), self.ws_bytes, _stream()),
            "select_range_u32")
        self._last = into

    def refine(self, col, lo: int, hi: int, signed: bool = False, negate: bool = False) -> None:
        """the rows of the last launch that also pass this predicate on `col`: its output list and its device count are
        the candidates, nothing is read back in between"""
        if self._last is None:
            raise ValueError("refine: nothing was launched on this plan")
        at = self._last
        self.launch(col, lo, hi, rows=self.rows[at][: self.capacity], count=self.counts[at: at + 1], signed=signed,
                    negate=negate)

    def launch_in(self, bloom: "BloomFilter", col: torch.Tensor, rows: torch.Tensor | None = None,
                  count: torch.Tensor | None = None, negate: bool = False) -> None:
        """launch() with the predicate "the Bloom filter may hold col[r]" (no false negatives; negate: "it certainly does
        not"): the same candidates, buffers, device counts and workspace, so a chain may mix range, packed and Bloom
        steps.  Asynchronous on the current stream; nothing is read back."""
        if not isinstance(bloom, BloomFilter):
            raise ValueError(f"bloom: expected a BloomFilter, got {type(bloom).__name__}")
        _need(col, torch.int32, "col")
        if bloom.filter.device != col.device:
            raise ValueError(f"bloom: the filter lives on {bloom.filter.device}, col on {col.device}")
        if rows is not None:
            _need(rows, torch.int32, "rows")
        elif count is not None:
            raise ValueError("count: given without rows")
        _need_count(count, "count")
        n_col = col.numel()
        candidates = n_col if rows is None else rows.numel()
        if candidates > self.capacity:
            raise ValueError(f"{candidates} candidates, the plan holds {self.capacity}")
        into = 0 if self._last is None else 1 - self._last
        if rows is not None and rows.untyped_storage().data_ptr() == self.rows[into].untyped_storage().data_ptr():
            into = 1 - into  # the list is a view of that buffer: write the other one
        col_ptr, col_n, list_ptr, count_ptr = col.data_ptr() if n_col else None, n_col, None, None
        if rows is not None and rows.numel():
            list_ptr, count_ptr = rows.data_ptr(), count.data_ptr() if count is not None else None
        elif rows is not None:  # an empty list has no address: the call over no rows at all
            col_ptr, col_n = None, 0
        _capi.check(bloom_native.probe(
            bloom.filter.data_ptr(), bloom.n_words, bloom.seed, col_ptr, col_n, list_ptr, count_ptr,
            rows.numel() if list_ptr else 0, bloom_native.NEGATE if negate else 0, self.rows[into].data_ptr(),
            self.counts[into:].data_ptr(), self.ws.data_ptr(), self.ws_bytes, _stream()), "bloom_probe_u32")
        self._last = into

    def refine_in(self, bloom: "BloomFilter", col: torch.Tensor, negate: bool = False) -> None:
        """the rows of the last launch whose value in `col` the Bloom filter may hold (negate: certainly does not hold)"""
        if self._last is None:
            raise ValueError("refine_in: nothing was launched on this plan")
        at = self._last
        self.launch_in(bloom, col, rows=self.rows[at][: self.capacity], count=self.counts[at: at + 1], negate=negate)

    def status(self) -> int:
        return workspace_status(self.ws)

    def count(self) -> int:
        return int(self.counts[self._last].item())

    def output(self) -> tuple[torch.Tensor, torch.Tensor]:
        """(rows[:capacity], its device count as a one-element int64 view) of the last launch, without synchronising:
        what another plan (RowSets, refine's own launch) takes as a list and its count inside one captured graph"""
        if self._last is None:
            raise ValueError("output: nothing was launched on this plan")
        at = self._last
        return self.rows[at][: self.capacity], self.counts[at: at + 1]

    def result(self, strict: bool = True) -> torch.Tensor:
        """the int32 row ids of the last launch (a view of the plan's buffer; synchronises).  strict: a row id outside
        the column among the candidates (DEV_KEY_RANGE) raises; otherwise such candidates are just dropped."""
        if self._last is None:
            raise ValueError("result: nothing was launched on this plan")
        if strict:
            _check_status(self.ws, "select_range_u32")
        return self.rows[self._last][: self.count()]


def select_range(col: torch.Tensor, lo: int, hi: int, rows: torch.Tensor | None = None, signed: bool = False,
                 negate: bool = False) -> torch.Tensor:
    """Row ids r (ascending, or in the order of `rows`) with lo <= col[r] <= hi — outside [lo, hi] with negate —
    compared as uint32, or as int32 with signed.  lo > hi is the empty interval.  rows: candidates, a row id as often
    as the list holds it; a row id >= col.numel() raises."""
    _bounds(lo, hi, signed)
    _need(col, torch.int32, "col")
    if rows is not None:
        _need(rows, torch.int32, "rows")
    plan = SelectRows(col.numel() if rows is None else rows.numel(), col.device)
    plan.launch(col, lo, hi, rows=rows, signed=signed, negate=negate)
    return plan.result()


# ---------------------------------------------------------------------------------------------
# sorted merge and set operations on row-id lists: merge path (host/merge_sorted.hpp, libdbench.so)
# ---------------------------------------------------------------------------------------------
def _need_count(count: torch.Tensor | None, name: str) -> None:
    if count is not None and (not count.is_cuda or count.dtype != torch.int64 or count.numel() != 1):
        raise ValueError(f"{name}: expected one int64 on the GPU")


def _column(t: torch.Tensor | None, count: torch.Tensor | None = None):
    """-> (address or None, entries, count's address or None) as the C entry points take a column: an empty tensor has
    no address, and then no count either"""
    if t is None or t.numel() == 0:
        return None, 0, None
    return t.data_ptr(), t.numel(), count.data_ptr() if count is not None else None


class MergeSorted:
    """Reusable plan for the stable merge of two ascending int32 key columns (compared as uint32, or as int32 with
    signed) of up to a_capacity and b_capacity rows: owns the workspace, the two output columns and the device count.
    Among equal keys A's rows come before B's.  Values: none (keys only), two int32 columns carried with their keys, or
    row_ids: the position in the concatenation, r for A's row r and a_keys.numel() + r for B's row r."""

    def __init__(self, a_capacity: int, b_capacity: int, device="cuda"):
        self.a_capacity, self.b_capacity = int(a_capacity), int(b_capacity)
        self.ws_bytes = merge_native.workspace_bytes(self.a_capacity, self.b_capacity)
        if self.ws_bytes == 0:
            raise ValueError("capacity: at most 2^32 - 1 rows in all")
        self.ws = _ws(self.ws_bytes, device)
        rows = max(self.a_capacity + self.b_capacity, 1)
        self.out_keys = torch.empty(rows, dtype=torch.int32, device=device)
        self.out_vals = torch.empty(rows, dtype=torch.int32, device=device)
        self.out_count = torch.zeros(1, dtype=torch.int64, device=device)
        self._vals = None  # whether the last launch wrote out_vals

    def launch(self, a_keys: torch.Tensor, b_keys: torch.Tensor, a_vals: torch.Tensor | None = None,
               b_vals: torch.Tensor | None = None, a_count: torch.Tensor | None = None,
               b_count: torch.Tensor | None = None, signed: bool = False, row_ids: bool = False) -> None:
        """Asynchronous on the current stream; nothing is read back.  a_count, b_count: device int64 of one element, the
        rows of that side that count (None: all of them; more than the column holds: all of them)."""
        _need(a_keys, torch.int32, "a_keys")
        _need(b_keys, torch.int32, "b_keys")
        if (a_vals is None) != (b_vals is None):
            raise ValueError("a_vals, b_vals: both or neither")
        if row_ids and a_vals is not None:
            raise ValueError("row_ids: given with value columns")
        for vals, keys, name in ((a_vals, a_keys, "a_vals"), (b_vals, b_keys, "b_vals")):
            if vals is not None:
                _need(vals, torch.int32, name)
                if vals.numel() != keys.numel():
                    raise ValueError(f"{name}: {vals.numel()} values for {keys.numel()} keys")
        _need_count(a_count, "a_count")
        _need_count(b_count, "b_count")
        if a_keys.numel() > self.a_capacity or b_keys.numel() > self.b_capacity:
            raise ValueError(f"{a_keys.numel()} and {b_keys.numel()} rows, the plan holds {self.a_capacity} and "
                             f"{self.b_capacity}")
        pa, na, ca = _column(a_keys, a_count)
        pb, nb, cb = _column(b_keys, b_count)
        self._vals = row_ids or a_vals is not None
        flags = (merge_native.SIGNED if signed else 0) | (merge_native.ROW_IDS if row_ids else 0)
        _capi.check(merge_native.merge(
            pa, _column(a_vals)[0], ca, na, pb, _column(b_vals)[0], cb, nb, flags, self.out_keys.data_ptr(),
            self.out_vals.data_ptr() if self._vals else None, self.out_count.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
            _stream()), "merge_u32")

    def status(self) -> int:
        return workspace_status(self.ws)

    def count(self) -> int:
        return int(self.out_count.item())

    def result(self):
        """(keys, values or None) of the last launch: views of the plan's buffers; synchronises"""
        if self._vals is None:
            raise ValueError("result: nothing was launched on this plan")
        _check_status(self.ws, "merge_u32")
        m = self.count()
        return self.out_keys[:m], (self.out_vals[:m] if self._vals else None)


def merge_sorted(a_keys: torch.Tensor, b_keys: torch.Tensor, a_vals: torch.Tensor | None = None,
                 b_vals: torch.Tensor | None = None, signed: bool = False, row_ids: bool = False):
    """The stable merge of two ascending key columns -> (keys, values or None); see MergeSorted."""
    _need(a_keys, torch.int32, "a_keys")
    _need(b_keys, torch.int32, "b_keys")
    plan = MergeSorted(a_keys.numel(), b_keys.numel(), a_keys.device)
    plan.launch(a_keys, b_keys, a_vals, b_vals, signed=signed, row_ids=row_ids)
    return plan.result()


SET_OPS = {"union": merge_native.UNION, "intersect": merge_native.INTERSECT, "difference": merge_native.DIFFERENCE}


class RowSets:
    """Reusable plan for the union, intersection and difference (A minus B) of two STRICTLY ascending int32 row-id
    lists (uint32 order: what SelectRows over all rows of a column returns) of up to a_capacity and b_capacity entries:
    owns the workspace, the output list and its device count.  The lists' lengths may be device counts
    (SelectRows.output()), so filters and set operations chain inside one captured graph without a read-back."""

    def __init__(self, a_capacity: int, b_capacity: int, device="cuda"):
        self.a_capacity, self.b_capacity = int(a_capacity), int(b_capacity)
        self.ws_bytes = merge_native.workspace_bytes(self.a_capacity, self.b_capacity)
        if self.ws_bytes == 0:
            raise ValueError("capacity: at most 2^32 - 1 rows in all")
        self.ws = _ws(self.ws_bytes, device)
        self.rows = torch.empty(max(self.a_capacity + self.b_capacity, 1), dtype=torch.int32, device=device)
        self.out_count = torch.zeros(1, dtype=torch.int64, device=device)
        self._launched = False

    def launch(self, op, a: torch.Tensor, b: torch.Tensor, a_count: torch.Tensor | None = None,
               b_count: torch.Tensor | None = None) -> None:
        """op: "union", "intersect", "difference" or the DBENCH_SETOP_* number.  Asynchronous on the current stream;
        nothing is read back."""
        if op not in SET_OPS and op not in SET_OPS.values():
            raise ValueError(f"op: expected one of {sorted(SET_OPS)}, got {op!r}")
        _need(a, torch.int32, "a")
        _need(b, torch.int32, "b")
        _need_count(a_count, "a_count")
        _need_count(b_count, "b_count")
        if a.numel() > self.a_capacity or b.numel() > self.b_capacity:
            raise ValueError(f"{a.numel()} and {b.numel()} rows, the plan holds {self.a_capacity} and {self.b_capacity}")
        pa, na, ca = _column(a, a_count)
        pb, nb, cb = _column(b, b_count)
        _capi.check(merge_native.setop(SET_OPS.get(op, op), pa, ca, na, pb, cb, nb, self.rows.data_ptr(),
                                       self.out_count.data_ptr(), self.ws.data_ptr(), self.ws_bytes, _stream()),
                    "setop_u32")
        self._launched = True

    def status(self) -> int:
        return workspace_status(self.ws)

    def count(self) -> int:
        return int(self.out_count.item())

    def result(self) -> torch.Tensor:
        """the ascending int32 row ids of the last launch (a view of the plan's buffer; synchronises)"""
        if not self._launched:
            raise ValueError("result: nothing was launched on this plan")
        _check_status(self.ws, "setop_u32")
        return self.rows[: self.count()]


def _set_rows(op: str, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    _need(a, torch.int32, "a")
    _need(b, torch.int32, "b")
    plan = RowSets(a.numel(), b.numel(), a.device)
    plan.launch(op, a, b)
    return plan.result()


def union_rows(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The rows of either of two strictly ascending row-id lists, ascending, each once."""
    return _set_rows("union", a, b)


def intersect_rows(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The rows of both of two strictly ascending row-id lists, ascending."""
    return _set_rows("intersect", a, b)


def difference_rows(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The rows of the strictly ascending list a that the strictly ascending list b does not hold, ascending."""
    return _set_rows("difference", a, b)


def select_any(col_a: torch.Tensor, lo_a: int, hi_a: int, col_b: torch.Tensor, lo_b: int, hi_b: int,
               signed: bool = False) -> torch.Tensor:
    """Row ids r, ascending, with lo_a <= col_a[r] <= hi_a OR lo_b <= col_b[r] <= hi_b: two selections over all rows
    and their union, the two lists' lengths staying on the device in between."""
    _bounds(lo_a, hi_a, signed)
    _bounds(lo_b, hi_b, signed)
    if col_a.numel() != col_b.numel():  # one row space: the union is over row ids of the same table
        raise ValueError(f"col_a and col_b: {col_a.numel()} and {col_b.numel()} rows, expected the same number")
    _need(col_a, torch.int32, "col_a")
    _need(col_b, torch.int32, "col_b")
    first, second = SelectRows(col_a.numel(), col_a.device), SelectRows(col_b.numel(), col_b.device)
    sets = RowSets(col_a.numel(), col_b.numel(), col_a.device)
    first.launch(col_a, lo_a, hi_a, signed=signed)
    second.launch(col_b, lo_b, hi_b, signed=signed)
    (rows_a, count_a), (rows_b, count_b) = first.output(), second.output()
    sets.launch("union", rows_a, rows_b, count_a, count_b)
    return sets.result()


# ---------------------------------------------------------------------------------------------
# Bloom filter: build from keys, probe into row-id lists (host/bloom_filter.hpp, libdbench.so)
# ---------------------------------------------------------------------------------------------
def bloom_words(n_keys: int, bits_per_key: int = 16) -> int:
    """the 64-bit words of a filter for n_keys keys: max(1, ceil(n_keys * bits_per_key / 64))"""
    if isinstance(n_keys, bool) or not isinstance(n_keys, int) or n_keys < 0:
        raise ValueError(f"n_keys: expected a count, got {n_keys!r}")
    if isinstance(bits_per_key, bool) or not isinstance(bits_per_key, int) or not 1 <= bits_per_key <= 64:
        raise ValueError(f"bits_per_key: expected an int in [1, 64], got {bits_per_key!r}")
    words = bloom_native.words(n_keys, bits_per_key) if n_keys < (1 << 64) else 0
    if words == 0:
        raise ValueError(f"n_keys: {n_keys} keys at {bits_per_key} bits need 2^32 filter words or more")
    return words


class BloomFilter:
    """A Bloom filter of n_words 64-bit words over 32-bit keys (one word and up to four bits per key; the format is
    host/bloom_filter.hpp's): owns the filter (an int64 tensor) and the 256-byte workspace of build().  What
    SelectRows.launch_in and refine_in test rows against."""

    def __init__(self, n_words: int, seed: int = 0, device="cuda"):
        if isinstance(n_words, bool) or not isinstance(n_words, int) or not 1 <= n_words < (1 << 32):
            raise ValueError(f"n_words: expected an int in [1, 2^32 - 1], got {n_words!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < (1 << 32):
            raise ValueError(f"seed: expected a uint32, got {seed!r}")
        self.n_words, self.seed = n_words, seed
        self.filter = torch.zeros(n_words, dtype=torch.int64, device=device)
        self.ws_bytes = 256
        self.ws = _ws(self.ws_bytes, device)

    def build(self, col: torch.Tensor, rows: torch.Tensor | None = None, count: torch.Tensor | None = None,
              accumulate: bool = False) -> None:
        """Asynchronous on the current stream; nothing is read back.  The keys are col[0 .. count) (count None: all
        rows), or with rows col[rows[i]] for i < count; count: a device int64 of one element.  accumulate: add the keys
        to what the filter holds instead of clearing it first."""
        _need(col, torch.int32, "col")
        if rows is not None:
            _need(rows, torch.int32, "rows")
        _need_count(count, "count")
        if self.filter.device != col.device:
            raise ValueError(f"col: lives on {col.device}, the filter on {self.filter.device}")
        col_ptr, n_col, _ = _column(col)
        list_ptr, capacity, count_ptr = _column(rows, count)
        if rows is None:
            count_ptr = count.data_ptr() if count is not None and n_col else None
        elif list_ptr is None:  # an empty list has no address: the build over no keys at all
            col_ptr, n_col = None, 0
        _capi.check(bloom_native.build(col_ptr, n_col, list_ptr, count_ptr, capacity, self.seed,
                                       bloom_native.ACCUMULATE if accumulate else 0, self.filter.data_ptr(), self.n_words,
                                       self.ws.data_ptr(), self.ws_bytes, _stream()), "bloom_build_u32")

    def status(self) -> int:
        return workspace_status(self.ws)


def bloom_build(col: torch.Tensor, bits_per_key: int = 16, seed: int = 0) -> BloomFilter:
    """a filter of bloom_words(col.numel(), bits_per_key) words holding every key of col"""
    words = bloom_words(col.numel(), bits_per_key)
    _need(col, torch.int32, "col")
    bloom = BloomFilter(words, seed, col.device)
    bloom.build(col)
    return bloom


def select_in_bloom(bloom: BloomFilter, col: torch.Tensor, rows: torch.Tensor | None = None,
                    negate: bool = False) -> torch.Tensor:
    """Row ids r (ascending, or in the order of `rows`) whose key col[r] the filter may hold — with negate those it
    certainly does not hold.  A row id >= col.numel() raises."""
    if not isinstance(bloom, BloomFilter):
        raise ValueError(f"bloom: expected a BloomFilter, got {type(bloom).__name__}")
    _need(col, torch.int32, "col")
    if rows is not None:
        _need(rows, torch.int32, "rows")
    plan = SelectRows(col.numel() if rows is None else rows.numel(), col.device)
    plan.launch_in(bloom, col, rows=rows, negate=negate)
    return plan.result()


# ---------------------------------------------------------------------------------------------
# HyperLogLog: approximate COUNT(DISTINCT), mergeable sketches (host/hll_sketch.hpp, libdbench.so)
# ---------------------------------------------------------------------------------------------
def _hll_p(p) -> int:
    if isinstance(p, bool) or not isinstance(p, int) or not hll_native.MIN_P <= p <= hll_native.MAX_P:
        raise ValueError(f"p: expected an int in [{hll_native.MIN_P}, {hll_native.MAX_P}], got {p!r}")
    return p


def hll_relative_error(p: int) -> float:
    """the standard error of a sketch of 2^p registers, relative to the count: 1.04 / sqrt(2^p)"""
    return 1.04 / math.sqrt(1 << _hll_p(p))


def _hll_columns(cols):
    """one tensor or a sequence of up to four int32 columns of equal length -> the list"""
    cols = [cols] if torch.is_tensor(cols) else list(cols)
    if not 1 <= len(cols) <= hll_native.MAX_COLS:
        raise ValueError(f"cols: expected one to {hll_native.MAX_COLS} columns, got {len(cols)}")
    for i, c in enumerate(cols):
        if not torch.is_tensor(c):
            raise ValueError(f"cols[{i}]: expected a tensor, got {type(c).__name__}")
        if c.numel() != cols[0].numel():
            raise ValueError(f"cols[{i}]: {c.numel()} rows, cols[0] has {cols[0].numel()}: columns of one table")
    for i, c in enumerate(cols):
        _need(c, torch.int32, f"cols[{i}]")
    return cols


class HyperLogLog:
    """A HyperLogLog sketch of 2^p one-byte registers over the rows of one to four int32 columns (the format is
    host/hll_sketch.hpp's): owns the registers (uint8, 2^p), the histogram of their values (int32, 64) that every build and
    merge writes, and the workspace.  estimate() is the one read-back: the 256 bytes of the histogram."""

    def __init__(self, p: int = 12, seed: int = 0, device="cuda"):
        self.p = _hll_p(p)
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < (1 << 32):
            raise ValueError(f"seed: expected a uint32, got {seed!r}")
        self.seed, self.m = seed, 1 << p
        self.registers = torch.zeros(self.m, dtype=torch.uint8, device=device)
        self.hist = torch.zeros(hll_native.HIST_WORDS, dtype=torch.int32, device=device)
        self.hist[0] = self.m  # the histogram of an empty sketch
        self.ws_bytes = hll_native.workspace_bytes(p)
        self.ws = _ws(self.ws_bytes, device)

    def build(self, cols, rows: torch.Tensor | None = None, count: torch.Tensor | None = None,
              accumulate: bool = False) -> None:
        """Asynchronous on the current stream; nothing is read back.  The keys are the tuples of rows 0 .. count (count
        None: all rows), or with rows those of rows[i] for i < count; count: a device int64 of one element.  accumulate: the
        max with what the sketch holds instead of the sketch of these rows alone."""
        cols = _hll_columns(cols)
        if rows is not None:
            _need(rows, torch.int32, "rows")
        _need_count(count, "count")
        if self.registers.device != cols[0].device:
            raise ValueError(f"cols: live on {cols[0].device}, the sketch on {self.registers.device}")
        n_col = cols[0].numel()
        ptrs = [c.data_ptr() if n_col else None for c in cols]
        list_ptr, capacity, count_ptr = _column(rows, count)
        if rows is None:
            count_ptr = count.data_ptr() if count is not None and n_col else None
        elif list_ptr is None:  # an empty list has no address: the build over no rows at all
            ptrs, n_col = [None] * len(cols), 0
        _capi.check(hll_native.build(ptrs, n_col, list_ptr, count_ptr, capacity, self.seed,
                                     hll_native.ACCUMULATE if accumulate else 0, self.p, self.registers.data_ptr(),
                                     self.hist.data_ptr(), self.ws.data_ptr(), self.ws_bytes, _stream()), "hll_build_u32")

    def merge(self, other: "HyperLogLog") -> None:
        """self becomes the sketch of the union: max(self, other) register by register.  Asynchronous."""
        if not isinstance(other, HyperLogLog):
            raise ValueError(f"other: expected a HyperLogLog, got {type(other).__name__}")
        if (other.p, other.seed) != (self.p, self.seed):
            raise ValueError(f"other: a sketch of p = {other.p}, seed {other.seed} does not merge into p = {self.p}, seed {self.seed}")
        if other.registers.device != self.registers.device:
            raise ValueError(f"other: lives on {other.registers.device}, the sketch on {self.registers.device}")
        if not self.registers.is_cuda:
            raise ValueError(f"merge: expected sketches on the GPU, got {self.registers.device}")
        _capi.check(hll_native.merge(self.registers.data_ptr(), other.registers.data_ptr(), self.p, self.hist.data_ptr(),
                                     self.ws.data_ptr(), self.ws_bytes, _stream()), "hll_merge")

    def estimate(self) -> float:
        """the estimated number of distinct rows: reads the histogram back (256 bytes; synchronises) and raises on a
        flagged status word"""
        hist = self.hist.cpu().tolist()
        _check_status(self.ws, "HyperLogLog")
        e = hll_native.estimate(hist, self.p)
        if e < 0:
            raise _capi.DbhipError(f"HyperLogLog: the histogram {hist} is not one of 2^{self.p} registers")
        return e

    def status(self) -> int:
        return workspace_status(self.ws)


def approx_count_distinct(cols, rows: torch.Tensor | None = None, p: int = 12, seed: int = 0) -> float:
    """the approximate number of distinct rows (tuples) of one to four int32 columns, over all rows or those of a row-id
    list: within hll_relative_error(p) of the truth, as a standard error.  A row id >= the columns' length raises."""
    _hll_p(p)
    cols = _hll_columns(cols)
    sketch = HyperLogLog(p, seed, cols[0].device)
    sketch.build(cols, rows=rows)
    return sketch.estimate()


# ---------------------------------------------------------------------------------------------
# quantiles: exact order statistics by a multi-rank radix select (host/quantile_select.hpp, libdbench.so)
# ---------------------------------------------------------------------------------------------
QUANTILE_MAX_RANKS = quantile_native.MAX_RANKS


def _quantile_ranks(qs) -> tuple[list[int], list[int]]:
    """the ranks of a call -> (q_num, q_den) as the entry point takes them.  An int is an absolute 0-based rank (q_den = 0);
    a (num, den) pair, a Fraction or a float in [0, 1] is PERCENTILE_DISC's fraction (a float through
    Fraction(q).limit_denominator(10**9))"""
    if isinstance(qs, (int, float, Fraction)) and not isinstance(qs, bool):
        qs = [qs]  # (a tuple is a sequence of ranks: one pair is [(num, den)])
    qs = list(qs)
    if not 1 <= len(qs) <= QUANTILE_MAX_RANKS:
        raise ValueError(f"qs: expected one to {QUANTILE_MAX_RANKS} ranks, got {len(qs)}")
    nums, dens = [], []
    for i, q in enumerate(qs):
        if isinstance(q, bool):
            raise ValueError(f"qs[{i}]: expected an int, a (num, den) pair, a Fraction or a float, got {q!r}")
        if isinstance(q, int):
            if not 0 <= q < (1 << 32):
                raise ValueError(f"qs[{i}]: an absolute rank is in [0, 2^32), got {q!r}")
            nums.append(q)
            dens.append(0)
            continue
        if isinstance(q, float):
            if not 0.0 <= q <= 1.0:  # (a NaN compares false)
                raise ValueError(f"qs[{i}]: q outside [0, 1]: {q!r}")
            q = Fraction(q).limit_denominator(10 ** 9)
        if isinstance(q, Fraction):
            q = (q.numerator, q.denominator)
        if (not isinstance(q, tuple) or len(q) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in q)):
            raise ValueError(f"qs[{i}]: expected an int, a (num, den) pair, a Fraction or a float, got {q!r}")
        num, den = q
        if not 0 < den < (1 << 32):
            raise ValueError(f"qs[{i}]: a denominator is in [1, 2^32), got {den!r}")
        if not 0 <= num <= den:
            raise ValueError(f"qs[{i}]: q outside [0, 1]: {num}/{den}")
        nums.append(num)
        dens.append(den)
    return nums, dens


class Quantiles:
    """Reusable plan for the values at up to n_q ranks of an int32 column (compared as uint32, or as int32 with signed),
    over all rows or the rows of a row-id list: owns the workspace and the three output columns (values, below, equal: one
    int32 tensor of 3 x n_q words).  launch() reads nothing back and can be captured; result() is the one read-back."""

    def __init__(self, n_q: int, device="cuda"):
        if isinstance(n_q, bool) or not isinstance(n_q, int) or not 1 <= n_q <= QUANTILE_MAX_RANKS:
            raise ValueError(f"n_q: expected an int in [1, {QUANTILE_MAX_RANKS}], got {n_q!r}")
        self.n_q = n_q
        self.ws_bytes = quantile_native.workspace_bytes(n_q)
        self.ws = _ws(self.ws_bytes, device)
        self.out = torch.zeros(3, n_q, dtype=torch.int32, device=device)
        self._signed = False
        self._launched = 0  # ranks of the last launch

    def launch(self, col: torch.Tensor, qs, rows: torch.Tensor | None = None, count: torch.Tensor | None = None,
               signed: bool = False) -> None:
        """Asynchronous on the current stream; nothing is read back.  qs: up to n_q ranks, each an int (the absolute 0-based
        rank), a (num, den) pair, a Fraction or a float in [0, 1] (PERCENTILE_DISC: 1/2 is the lower median); they are host
        values, frozen into a captured graph, and resolved on the device against the number of candidates.  The candidates
        are rows 0 .. count of col (count None: all rows), or with rows those of rows[i] for i < count; count: a device
        int64 of one element."""
        nums, dens = _quantile_ranks(qs)
        if len(nums) > self.n_q:
            raise ValueError(f"qs: {len(nums)} ranks, the plan holds {self.n_q}")
        _need(col, torch.int32, "col")
        if rows is not None:
            _need(rows, torch.int32, "rows")
        _need_count(count, "count")
        if self.out.device != col.device:
            raise ValueError(f"col: lives on {col.device}, the plan on {self.out.device}")
        n_col = col.numel()
        col_ptr = col.data_ptr() if n_col else None
        list_ptr, capacity, count_ptr = _column(rows, count)
        if rows is None:
            count_ptr = count.data_ptr() if count is not None and n_col else None
        elif list_ptr is None:  # an empty list has no address: the call over no rows at all
            col_ptr, n_col = None, 0
        _capi.check(quantile_native.select(
            col_ptr, n_col, list_ptr, count_ptr, capacity, nums, dens, quantile_native.SIGNED if signed else 0,
            self.out[0].data_ptr(), self.out[1].data_ptr(), self.out[2].data_ptr(), self.ws.data_ptr(), self.ws_bytes,
            _stream()), "quantile_select_u32")
        self._signed, self._launched = bool(signed), len(nums)

    def status(self) -> int:
        return workspace_status(self.ws)

    def result(self):
        """(values, below, equal) of the last launch's ranks as int64 tensors on the host (one copy of 12 bytes per rank;
        synchronises), and raises on a flagged status word (a row id outside the column).  values: the keys in the order's
        own numbers (int32 with signed, uint32 otherwise); below: the candidates strictly before the value, equal: those
        equal to it.  A rank that names no row (no candidates, or an absolute rank beyond them) has value 0, below = the
        number of candidates and equal = 0."""
        if not self._launched:
            raise ValueError("result: nothing was launched on this plan")
        host = self.out[:, : self._launched].cpu()
        _check_status(self.ws, "quantile_select_u32")
        values, below, equal = (host[i].to(torch.int64) for i in range(3))
        if not self._signed:
            values = values & 0xFFFFFFFF
        return values, below & 0xFFFFFFFF, equal & 0xFFFFFFFF


def quantiles(col: torch.Tensor, qs, rows: torch.Tensor | None = None, signed: bool = False):
    """(values, below, equal), int64 on the host, at the ranks qs of an int32 column — compared as uint32, or as int32 with
    signed — over all rows or those of a row-id list (a row id as often as the list holds it; one >= col.numel() raises).
    Exact: PERCENTILE_DISC for a fraction, the k-th smallest for an int."""
    nums, _ = _quantile_ranks(qs)
    _need(col, torch.int32, "col")
    plan = Quantiles(len(nums), col.device)
    plan.launch(col, qs, rows=rows, signed=signed)
    return plan.result()


def kth_value(col: torch.Tensor, k: int, rows: torch.Tensor | None = None, signed: bool = False) -> int:
    """the k-th smallest value (k = 0: the minimum) among the candidates; IndexError when there are k or fewer"""
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"k: expected an int, got {k!r}")
    values, _, equal = quantiles(col, [k], rows=rows, signed=signed)
    if int(equal[0]) == 0:
        raise IndexError(f"kth_value: no row of rank {k}")
    return int(values[0])


def median(col: torch.Tensor, rows: torch.Tensor | None = None, signed: bool = False) -> int:
    """the lower median (PERCENTILE_DISC(0.5)) of the candidates; IndexError when there are none"""
    values, _, equal = quantiles(col, [(1, 2)], rows=rows, signed=signed)
    if int(equal[0]) == 0:
        raise IndexError("median: no rows")
    return int(values[0])


def equi_depth_bounds(col: torch.Tensor, parts: int, rows: torch.Tensor | None = None, signed: bool = False) -> torch.Tensor:
    """the parts - 1 values at i / parts, i = 1 .. parts - 1: the upper bounds of equi-depth buckets (deciles for
    parts = 10; the splitters of a range partition).  parts in 2 .. 17; int64 on the host; IndexError without rows"""
    if isinstance(parts, bool) or not isinstance(parts, int) or not 2 <= parts <= QUANTILE_MAX_RANKS + 1:
        raise ValueError(f"parts: expected an int in [2, {QUANTILE_MAX_RANKS + 1}], got {parts!r}")
    values, _, equal = quantiles(col, [(i, parts) for i in range(1, parts)], rows=rows, signed=signed)
    if int(equal[0]) == 0:
        raise IndexError("equi_depth_bounds: no rows")
    return values


# ---------------------------------------------------------------------------------------------
# late materialisation: take and aggregate through a row-id list (host/take_rows.hpp, libdbench.so)
# ---------------------------------------------------------------------------------------------
def _fill_word(fill: int) -> int:
    if isinstance(fill, bool) or not isinstance(fill, int) or not -(1 << 31) <= fill < (1 << 32):
        raise ValueError(f"fill: expected an int32 or uint32 value, got {fill!r}")
    return fill & 0xFFFFFFFF


def _take_columns(cols, most: int | None):
    """cols as a list of int32 GPU columns of one length -> (the list, whether a single tensor was given)"""
    single = torch.is_tensor(cols)
    cols = [cols] if single else list(cols)
    if not cols or (most is not None and len(cols) > most):
        raise ValueError(f"cols: expected 1 to {most} columns, got {len(cols)}" if most is not None else
                         "cols: expected at least one column")
    for i, c in enumerate(cols):
        if not torch.is_tensor(c):
            raise ValueError(f"cols[{i}]: expected a tensor, got {type(c).__name__}")
        if c.numel() != cols[0].numel():
            raise ValueError(f"cols[{i}]: {c.numel()} rows, cols[0] has {cols[0].numel()}: columns of one table")
    for i, c in enumerate(cols):
        _need(c, torch.int32, f"cols[{i}]")
    return cols, single


class TakeRows:
    """Reusable plan that materialises up to n_cols int32 columns through a row-id list of up to `capacity` entries:
    owns the workspace and n_cols output columns.  The list's length may be a device count (SelectRows.output(), the
    output of RowSets, JoinPairs.total), so filter -> take is one captured sequence without a read-back.  A row id outside
    the columns is filled with `fill` and raises DEV_KEY_RANGE; with outer the id 0xFFFFFFFF (-1: the build row of a
    left-outer join's miss) is filled silently."""

    def __init__(self, capacity: int, n_cols: int = 1, device="cuda"):
        self.capacity, self.n_cols = int(capacity), int(n_cols)
        if not 1 <= self.n_cols <= take_native.MAX_COLS:
            raise ValueError(f"n_cols: expected 1 to {take_native.MAX_COLS}, got {n_cols}")
        self.ws_bytes = take_native.workspace_bytes(self.capacity)
        if self.ws_bytes == 0:
            raise ValueError("capacity: at most 2^32 - 1 entries")
        self.ws = _ws(self.ws_bytes, device)
        self.outs = [torch.empty(max(self.capacity, 1), dtype=torch.int32, device=device) for _ in range(self.n_cols)]
        self._count = None  # the device count of the last launch (None: all entries of its list)
        self._used = None   # (columns, entries) of the last launch

    def launch(self, cols, rows: torch.Tensor, count: torch.Tensor | None = None, outer: bool = False, fill: int = 0) -> None:
        """Asynchronous on the current stream; nothing is read back.  cols: an int32 tensor or a sequence of 1..n_cols of
        them, all of one length; rows: the int32 row-id list; count: a device int64 of one element, the number of entries
        of `rows` that count (None: all of them; more than the list holds: all of them)."""
        fill = _fill_word(fill)
        cols, _ = _take_columns(cols, self.n_cols)
        _need(rows, torch.int32, "rows")
        _need_count(count, "count")
        if rows.numel() > self.capacity:
            raise ValueError(f"{rows.numel()} entries, the plan holds {self.capacity}")
        list_ptr, entries, count_ptr = _column(rows, count)
        n_rows = cols[0].numel()
        _capi.check(take_native.take(
            [c.data_ptr() if n_rows else None for c in cols], len(cols), n_rows, list_ptr, count_ptr, entries,
            take_native.OUTER if outer else 0, fill, [o.data_ptr() for o in self.outs[: len(cols)]], self.ws.data_ptr(),
            self.ws_bytes, _stream()), "take_u32")
        self._count = count if entries else None
        self._used = (len(cols), entries)

    def status(self) -> int:
        return workspace_status(self.ws)

    def output(self):
        """(the output columns cut to the capacity, the device count of the last launch or None) without synchronising"""
        if self._used is None:
            raise ValueError("output: nothing was launched on this plan")
        return [o[: self.capacity] for o in self.outs[: self._used[0]]], self._count

    def result(self, strict: bool = True):
        """the columns of the last launch cut to min(count, entries): views of the plan's buffers; synchronises.
        strict: a row id outside the columns (DEV_KEY_RANGE) raises; otherwise such entries hold the fill."""
        if self._used is None:
            raise ValueError("result: nothing was launched on this plan")
        if strict:
            _check_status(self.ws, "take_u32")
        used, entries = self._used
        m = entries if self._count is None else min(max(int(self._count.item()), 0), entries)
        return [o[:m] for o in self.outs[:used]]


def take(cols, rows: torch.Tensor, outer: bool = False, fill: int = 0):
    """cols[c][rows[i]] for every i: a tensor for a tensor, a list for a sequence of int32 columns of one length (more
    than four run in groups of four).  A row id outside the columns raises; with outer the id -1 gives `fill`."""
    _fill_word(fill)
    cols, single = _take_columns(cols, None)
    _need(rows, torch.int32, "rows")
    out = []
    for at in range(0, len(cols), take_native.MAX_COLS):
        group = cols[at: at + take_native.MAX_COLS]
        plan = TakeRows(rows.numel(), len(group), rows.device)
        plan.launch(group, rows, outer=outer, fill=fill)
        out += plan.result()
    return out[0] if single else out


class AggregateRows:
    """Reusable plan for COUNT, the 64-bit SUM, MIN and MAX of an int32 column (as uint32, or as int32 with signed) over
    a row-id list of up to `capacity` entries, or over all its rows (up to `capacity` of them), without materialising
    the values: owns the workspace and the four device result words."""

    def __init__(self, capacity: int, device="cuda"):
        self.capacity = int(capacity)
        self.ws_bytes = take_native.workspace_bytes(self.capacity)
        if self.ws_bytes == 0:
            raise ValueError("capacity: at most 2^32 - 1 entries")
        self.ws = _ws(self.ws_bytes, device)
        self.out = torch.zeros(4, dtype=torch.int64, device=device)
        self._signed = None  # of the last launch

    def launch(self, col: torch.Tensor, rows: torch.Tensor | None = None, count: torch.Tensor | None = None,
               signed: bool = False, outer: bool = False) -> None:
        """Asynchronous on the current stream; nothing is read back.  rows: an int32 row-id list (None: all rows of col);
        count: a device int64 of one element, the entries of `rows` that count.  Row ids outside the column are skipped
        and raise DEV_KEY_RANGE; with outer the id 0xFFFFFFFF is skipped silently."""
        if rows is None and count is not None:
            raise ValueError("count: given without rows")
        _need(col, torch.int32, "col")
        if rows is not None:
            _need(rows, torch.int32, "rows")
        _need_count(count, "count")
        candidates = col.numel() if rows is None else rows.numel()
        if candidates > self.capacity:
            raise ValueError(f"{candidates} candidates, the plan holds {self.capacity}")
        list_ptr, entries, count_ptr = _column(rows, count)
        col_ptr, n_rows = (col.data_ptr(), col.numel()) if col.numel() else (None, 0)
        if rows is not None and not entries:  # an empty list has no address: the call over no rows at all
            col_ptr, n_rows = None, 0
        flags = (take_native.SIGNED if signed else 0) | (take_native.OUTER if outer else 0)
        _capi.check(take_native.aggregate(col_ptr, n_rows, list_ptr, count_ptr, entries, flags, self.out.data_ptr(),
                                          self.ws.data_ptr(), self.ws_bytes, _stream()), "aggregate_rows_u32")
        self._signed = bool(signed)

    def status(self) -> int:
        return workspace_status(self.ws)

    def output(self) -> torch.Tensor:
        """the four device words (count, sum, min, max: int64 storage of uint64) of the last launch, without synchronising"""
        if self._signed is None:
            raise ValueError("output: nothing was launched on this plan")
        return self.out

    def result(self, strict: bool = True):
        """(count, sum, min, max) of the last launch as Python ints: the sum mod 2^64 as an unsigned number, or as a
        two's-complement one with signed; min and max are None when count is 0.  Synchronises.  strict: a row id outside
        the column among the candidates (DEV_KEY_RANGE) raises; otherwise such candidates are just skipped."""
        if self._signed is None:
            raise ValueError("result: nothing was launched on this plan")
        if strict:
            _check_status(self.ws, "aggregate_rows_u32")
        words = [int(w) for w in self.out.tolist()]  # two's complement of the uint64 words
        if not self._signed:
            words = [w & 0xFFFFFFFFFFFFFFFF for w in words]
        n = words[0] & 0xFFFFFFFFFFFFFFFF
        return n, words[1], (words[2] if n else None), (words[3] if n else None)


def aggregate_rows(col: torch.Tensor, rows: torch.Tensor | None = None, signed: bool = False, outer: bool = False):
    """(COUNT, SUM, MIN, MAX) of col over the row-id list `rows`, or over all its rows; see AggregateRows.result()."""
    _need(col, torch.int32, "col")
    if rows is not None:
        _need(rows, torch.int32, "rows")
    plan = AggregateRows(col.numel() if rows is None else rows.numel(), col.device)
    plan.launch(col, rows, signed=signed, outer=outer)
    return plan.result()


# ---------------------------------------------------------------------------------------------
# dictionary encoding: factorize, multi-column keys (host/dict_encode.hpp, libdbench.so)
# ---------------------------------------------------------------------------------------------
DICT_MISS = dict_native.MISS            # the code of a value a dictionary does not hold (-1 as int32): take's "no row" id
DICT_LDS_SLOTS = dict_native.LDS_SLOTS  # tables up to this many slots (capacities up to half of it) are encoded out of LDS
DICT_DENSE_GROUPS = 1 << 22             # groupby_columns: composite cardinalities up to this go to the dense group-by


class Dictionary:
    """Reusable order-preserving dictionary of one int32 column (values ordered as uint32, or as int32 with signed) with up
    to `capacity` distinct values (0: n, always enough for a column of n rows; the build sorts `capacity` padded entries
    whatever the column holds, so a caller who knows a bound passes it).  Owns the workspace, which holds the table value
    -> code between build and encode, the key column and the device count.  A code is the index of the value in `keys`;
    DICT_MISS stands for a value the dictionary does not hold."""

    def __init__(self, n: int, capacity: int = 0, device="cuda"):
        self.n = int(n)
        self.capacity = int(capacity) if capacity else max(self.n, 1)
        self.ws_bytes = dict_native.workspace_bytes(self.capacity)
        if self.ws_bytes == 0:
            raise ValueError("capacity: 1 to 2^31 - 1 distinct values")
        self.ws = _ws(self.ws_bytes, device)
        self.keys = torch.empty(self.capacity, dtype=torch.int32, device=device)
        self.count_dev = torch.zeros(1, dtype=torch.int64, device=device)  # the number of keys, for combine and take
        self._signed = None  # of the last build

    def build(self, col: torch.Tensor, count: torch.Tensor | None = None, signed: bool = False) -> None:
        """Asynchronous on the current stream; nothing is read back.  count: a device int64 of one element, the rows of
        `col` that count.  More than `capacity` distinct values raise DEV_TABLE_FULL in the workspace."""
        _need(col, torch.int32, "col")
        _need_count(count, "count")
        ptr, rows, count_ptr = _column(col, count)
        _capi.check(dict_native.build(ptr, rows, count_ptr, self.capacity, dict_native.SIGNED if signed else 0,
                                      self.keys.data_ptr(), self.count_dev.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                                      _stream()), "dict_build_u32")
        self._signed = bool(signed)

    def _built(self, what: str) -> None:
        if self._signed is None:
            raise ValueError(f"{what}: nothing was built on this plan")

    def encode(self, col: torch.Tensor, count: torch.Tensor | None = None, out: torch.Tensor | None = None,
               misses: torch.Tensor | None = None) -> torch.Tensor:
        """-> the codes of col's rows (a new int32 column, or `out`); asynchronous, nothing is read back, the dictionary
        is only read.  Rows behind `count` are not written.  misses: a device int64 of one element for the number of
        rows whose value the dictionary does not hold."""
        self._built("encode")
        _need(col, torch.int32, "col")
        _need_count(count, "count")
        _need_count(misses, "misses")
        if out is None:
            out = torch.empty(col.numel(), dtype=torch.int32, device=col.device)
        else:
            _need(out, torch.int32, "out")
            if out.numel() != col.numel():
                raise ValueError(f"out: {out.numel()} rows, col has {col.numel()}")
        ptr, rows, count_ptr = _column(col, count)
        _capi.check(dict_native.encode(ptr, rows, count_ptr, out.data_ptr() if rows else None,
                                       misses.data_ptr() if misses is not None else None, self.ws.data_ptr(), self.ws_bytes,
                                       _stream()), "dict_encode_u32")
        return out

    def status(self) -> int:
        return workspace_status(self.ws)

    def packed_width(self) -> int:
        """the width at which every code of this dictionary fits (codes are below the capacity), known without a
        read-back: BitPack(n, d.packed_width()) behind encode is one captured sequence.  DICT_MISS does not fit below 32
        bits: packing it raises DEV_KEY_RANGE."""
        return max(1, (self.capacity - 1).bit_length())

    def count(self) -> int:
        """the number of distinct values of the last build; synchronises and raises on a device status"""
        self._built("count")
        _check_status(self.ws, "dict_build_u32")
        return int(self.count_dev.item())

    def result(self) -> torch.Tensor:
        """the distinct values in order: a view of the plan's key column cut to their number; synchronises and raises on
        a device status (DEV_TABLE_FULL: more distinct values than the capacity)"""
        return self.keys[: self.count()]

    def decode(self, codes: torch.Tensor, fill: int = 0) -> torch.Tensor:
        """the values of `codes`: take through the keys, DICT_MISS giving `fill`"""
        self._built("decode")
        return take(self.result(), codes, outer=True, fill=fill)


def factorize(col: torch.Tensor, signed: bool = False, capacity: int | None = None):
    """-> (codes, uniques) with uniques the distinct values in order and uniques[codes] == col: the answer of
    numpy.unique(col, return_inverse=True) on the uint32 (signed: int32) view.  capacity: a bound on the number of
    distinct values (None: the number of rows); more than that raise."""
    _need(col, torch.int32, "col")
    plan = Dictionary(col.numel(), capacity or 0, col.device)
    plan.build(col, signed=signed)
    codes = plan.encode(col)
    return codes, plan.result()


def dict_combine(outer: torch.Tensor, inner: torch.Tensor, outer_card: torch.Tensor, inner_card: torch.Tensor,
                 count: torch.Tensor | None = None, out: torch.Tensor | None = None, ws: torch.Tensor | None = None):
    """-> (out, ws): out[i] = outer[i] * inner_card + inner[i], DICT_MISS where either code is; asynchronous, nothing is
    read back.  The cardinalities are device int64 of one element (Dictionary.count_dev).  out may be `outer` itself.  A
    product of the cardinalities above 0xFFFFFFFF raises DEV_KEY_RANGE in ws (256 bytes, made here when not given) and
    leaves DICT_MISS everywhere."""
    _need(outer, torch.int32, "outer")
    _need(inner, torch.int32, "inner")
    for name, t in (("outer_card", outer_card), ("inner_card", inner_card)):
        if t is None:
            raise ValueError(f"{name}: expected one int64 on the GPU")
        _need_count(t, name)
    _need_count(count, "count")
    if inner.numel() != outer.numel():
        raise ValueError(f"inner: {inner.numel()} rows, outer has {outer.numel()}")
    if out is None:
        out = torch.empty(outer.numel(), dtype=torch.int32, device=outer.device)
    else:
        _need(out, torch.int32, "out")
        if out.numel() != outer.numel():
            raise ValueError(f"out: {out.numel()} rows, outer has {outer.numel()}")
    if ws is None:
        ws = _ws(256, outer.device)
    rows = outer.numel()
    _capi.check(dict_native.combine(outer.data_ptr() if rows else None, inner.data_ptr() if rows else None, rows,
                                    count.data_ptr() if count is not None and rows else None, outer_card.data_ptr(),
                                    inner_card.data_ptr(), out.data_ptr() if rows else None, ws.data_ptr(), ws.numel(),
                                    _stream()), "dict_combine_u32")
    return out, ws


def _key_columns(cols, least: int, name: str = "cols"):
    cols = list(cols)
    if len(cols) < least:
        raise ValueError(f"{name}: expected {'two or more' if least == 2 else 'at least one'} columns, got {len(cols)}")
    for i, c in enumerate(cols):
        if not torch.is_tensor(c):
            raise ValueError(f"{name}[{i}]: expected a tensor, got {type(c).__name__}")
        if c.numel() != cols[0].numel():
            raise ValueError(f"{name}[{i}]: {c.numel()} rows, {name}[0] has {cols[0].numel()}: columns of one table")
    for i, c in enumerate(cols):
        _need(c, torch.int32, f"{name}[{i}]")
    return cols


def _combine_codes(codes, cards, device):
    """the codes of several columns folded left to right -> (composite, its cardinality); raises on overflow"""
    composite, card = codes[0], cards[0]
    for inner, inner_card in zip(codes[1:], cards[1:]):
        oc, ic = (torch.tensor([c], dtype=torch.int64, device=device) for c in (card, inner_card))
        composite, ws = dict_combine(composite, inner, oc, ic)
        if workspace_status(ws) != DEV_OK:
            raise _capi.DbhipError(f"dict_combine_u32: {card} x {inner_card} composite keys do not fit 32 bits "
                                   f"(device status {DEV_KEY_RANGE:#x})")
        card *= inner_card
    return composite, card


def _encode_columns(cols, signed: bool, least: int):
    cols = _key_columns(cols, least)
    pairs = [factorize(c, signed) for c in cols]
    uniques = [u for _, u in pairs]
    composite, card = _combine_codes([c for c, _ in pairs], [u.numel() for u in uniques], cols[0].device)
    return composite, uniques, card


def encode_columns(cols, signed: bool = False):
    """Two or more int32 columns of one table -> (codes, [uniques per column], cardinality): every column is factorized
    and the codes are combined left to right, so codes order the rows as the tuples (cols[0][i], cols[1][i], ...) do,
    equal tuples have equal codes, and all codes lie below cardinality = the product of the columns' numbers of distinct
    values.  A cardinality above 0xFFFFFFFF raises."""
    return _encode_columns(cols, signed, 2)


def groupby_columns(cols, vals: torch.Tensor, signed: bool = False, dense_groups: int | None = None):
    """GROUP BY cols[0], cols[1], ... SUM(vals), COUNT(*): -> ([key columns], sums, counts), one row per distinct tuple, in
    the tuples' lexicographic order; SUM wraps at 32 bits as in both group-bys.  The composite code of encode_columns is the
    key of the dense groupby_sum while its cardinality is at most dense_groups (None: DICT_DENSE_GROUPS), of groupby_hash
    followed by a sort of the groups otherwise; the key columns come back from the composite by divide / modulo and a
    take through each column's uniques."""
    cols = _key_columns(cols, 1)
    _need(vals, torch.int32, "vals")
    if vals.numel() != cols[0].numel():
        raise ValueError(f"vals: {vals.numel()} rows, cols[0] has {cols[0].numel()}")
    composite, uniques, card = _encode_columns(cols, signed, 1)
    limit = DICT_DENSE_GROUPS if dense_groups is None else int(dense_groups)
    if card == 0:  # no rows
        groups = sums = counts = composite
    elif card <= limit:
        all_sums = groupby_sum(composite, vals, card)
        all_counts = groupby_sum(composite, torch.ones_like(vals), card)
        groups = select_range(all_counts, 1, 0xFFFFFFFF)  # the tuples that occur, ascending
        sums, counts = take([all_sums, all_counts], groups)
    else:
        keys, sums, counts = groupby_hash(composite, vals)
        groups = keys.clone()
        order = radix_argsort_(groups)  # groups: the composites ascending
        sums, counts = take([sums, counts], order)
    rest = groups.to(torch.int64) & 0xFFFFFFFF
    key_cols = []
    for u in reversed(uniques):
        d = max(u.numel(), 1)
        key_cols.append(take(u, (rest % d).to(torch.int32)) if rest.numel() else u[:0])
        rest = rest // d
    return key_cols[::-1], sums, counts


def join_pairs_columns(build_cols, probe_cols, left_outer: bool = False):
    """The equi-join ON build.c0 = probe.c0 AND build.c1 = probe.c1 ...: -> (build_rows, probe_rows) as join_pairs gives
    them, probe rows ascending (left_outer: and one pair with build row -1 per probe row without a match).  The
    dictionaries are built on the build side's columns and the probe side is encoded through them: a probe value the build
    side does not hold becomes DICT_MISS, and so does the row's composite, which matches nothing."""
    build_cols, probe_cols = list(build_cols), list(probe_cols)
    if len(build_cols) != len(probe_cols):
        raise ValueError(f"probe_cols: {len(probe_cols)} columns, build_cols has {len(build_cols)}")
    build_cols, probe_cols = _key_columns(build_cols, 1, "build_cols"), _key_columns(probe_cols, 1, "probe_cols")
    build_codes, probe_codes, cards = [], [], []
    for b, p in zip(build_cols, probe_cols):
        plan = Dictionary(b.numel(), 0, b.device)
        plan.build(b)
        build_codes.append(plan.encode(b))
        probe_codes.append(plan.encode(p))
        cards.append(plan.count())
    device = build_cols[0].device
    build_key, _ = _combine_codes(build_codes, cards, device)
    probe_key, _ = _combine_codes(probe_codes, cards, device)
    return join_pairs(build_key, probe_key, left_outer=left_outer, ordered=True)


# ---------------------------------------------------------------------------------------------
# bit-packed columns: pack, unpack, filter on packed codes (host/bitpack.hpp, libdbench.so)
# ---------------------------------------------------------------------------------------------
def _width(width) -> int:
    if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= 32:
        raise ValueError(f"width: expected an int in 1..32, got {width!r}")
    return width


def _base_word(base) -> int:
    if isinstance(base, bool) or not isinstance(base, int) or not -(1 << 31) <= base < (1 << 32):
        raise ValueError(f"base: expected an int32 or uint32 value, got {base!r}")
    return base & 0xFFFFFFFF


class PackedColumn:
    """A column of n_rows 32-bit values held in `width` bits per row (host/bitpack.hpp): row i is base + code i mod 2^32,
    code i the bits [i * width, i * width + width) of the little-endian bit stream over the int32 words of `packed`, which
    start on a 16-byte boundary and are padded with zero bits to whole 16-byte chunks."""

    def __init__(self, packed: torch.Tensor, n_rows: int, width: int, base: int = 0):
        self.width, self.base, self.n_rows = _width(width), _base_word(base), int(n_rows)
        if not 0 <= self.n_rows < (1 << 32):
            raise ValueError("n_rows: at most 2^32 - 1 rows")
        words = bitpack_native.words(self.n_rows, self.width)
        if not torch.is_tensor(packed) or packed.dtype != torch.int32 or not packed.is_contiguous():
            raise ValueError("packed: expected a contiguous torch.int32 tensor")
        if packed.numel() < words:
            raise ValueError(f"packed: {packed.numel()} words, {self.n_rows} rows of {self.width} bits take {words}")
        if packed.numel() and packed.data_ptr() % 16:
            raise ValueError(f"packed: the words must start on a 16-byte boundary (got offset {packed.data_ptr() % 16})")
        self.packed = packed[:words]

    @property
    def nbytes(self) -> int:
        """the bytes of the packed words (a 32-bit column of as many rows takes 4 * n_rows)"""
        return 4 * self.packed.numel()

    def __len__(self) -> int:
        return self.n_rows


def _need_packed(pc, name: str) -> torch.Tensor:
    if not isinstance(pc, PackedColumn):
        raise ValueError(f"{name}: expected a PackedColumn, got {type(pc).__name__}")
    _need(pc.packed, torch.int32, f"{name}.packed")
    return pc.packed


class BitPack:
    """Reusable plan that packs int32 columns of up to `capacity` rows at `width` bits over `base`: owns the workspace and
    the packed words.  The number of rows may be a device count (the count of Dictionary.encode, SelectRows.output()), so
    encode -> pack is one captured sequence without a read-back.  A row whose code (value - base mod 2^32) does not fit
    keeps its low bits and raises DEV_KEY_RANGE."""

    def __init__(self, capacity: int, width: int, base: int = 0, device="cuda"):
        self.capacity, self.width, self.base = int(capacity), _width(width), _base_word(base)
        self.ws_bytes = bitpack_native.workspace_bytes(self.capacity)
        if self.ws_bytes == 0:
            raise ValueError("capacity: at most 2^32 - 1 rows")
        self.ws = _ws(self.ws_bytes, device)
        self.packed = torch.zeros(max(bitpack_native.words(self.capacity, self.width), 4), dtype=torch.int32, device=device)
        self._count = None  # the device count of the last launch (None: all rows of its column)
        self._rows = None   # the rows of the column of the last launch

    def launch(self, col: torch.Tensor, count: torch.Tensor | None = None) -> None:
        """Asynchronous on the current stream; nothing is read back.  count: a device int64 of one element, the rows of
        `col` that count (None: all of them); the words behind the packed form of those rows are not written."""
        _need(col, torch.int32, "col")
        _need_count(count, "count")
        if col.numel() > self.capacity:
            raise ValueError(f"{col.numel()} rows, the plan holds {self.capacity}")
        ptr, rows, count_ptr = _column(col, count)
        _capi.check(bitpack_native.pack(ptr, rows, count_ptr, self.width, self.base, self.packed.data_ptr() if rows else None,
                                        self.ws.data_ptr(), self.ws_bytes, _stream()), "bitpack_pack_u32")
        self._count = count if rows else None
        self._rows = rows

    def status(self) -> int:
        return workspace_status(self.ws)

    def output(self) -> PackedColumn:
        """the packed column of the last launch at ALL rows of its input, without synchronising: what select and unpack
        take inside one captured graph.  Rows behind a device count hold whatever the buffer held before."""
        if self._rows is None:
            raise ValueError("output: nothing was launched on this plan")
        return PackedColumn(self.packed, self._rows, self.width, self.base)

    def result(self, strict: bool = True) -> PackedColumn:
        """the packed column of the last launch cut to min(count, rows): a view of the plan's words; synchronises.
        strict: a row that did not fit (DEV_KEY_RANGE) raises; otherwise it holds its code's low bits."""
        if self._rows is None:
            raise ValueError("result: nothing was launched on this plan")
        if strict:
            _check_status(self.ws, "bitpack_pack_u32")
        m = self._rows if self._count is None else min(max(int(self._count.item()), 0), self._rows)
        return PackedColumn(self.packed, m, self.width, self.base)


def pack(col: torch.Tensor, width: int | None = None, base: int | None = None, signed: bool = False) -> PackedColumn:
    """col in `width` bits per row over `base`.  width None: the minimum and maximum come from aggregate_rows (one
    read-back; ordered as uint32, or as int32 with signed), base = the minimum unless given (it must not exceed it) and
    width = bit_length(maximum - base), at least 1.  width given: base defaults to 0.  A value that does not fit raises."""
    _need(col, torch.int32, "col")
    if base is not None:
        _base_word(base)
    if width is None:
        n, _, least, most = aggregate_rows(col, signed=signed)
        if base is None:
            base = least if n else 0
        elif n and base > least:
            raise ValueError(f"base: {base} is above the column's minimum {least}")
        width = max(1, (most - base).bit_length()) if n else 1
    plan = BitPack(col.numel(), _width(width), _base_word(0 if base is None else base), col.device)
    plan.launch(col)
    return plan.result()


def unpack(pc: PackedColumn, rows: torch.Tensor | None = None, count: torch.Tensor | None = None, outer: bool = False,
           fill: int = 0, out: torch.Tensor | None = None, ws: torch.Tensor | None = None) -> torch.Tensor:
    """The values of a packed column: all rows (rows None), or pc[rows[i]] for every entry of an int32 row-id list, with
    the rules of take: a row id outside the column gives `fill` and raises; with outer the id -1 gives `fill` silently.
    count: a device int64 of one element, the entries of `rows` that count.  Without ws the call synchronises, raises on
    a device status and returns the values cut to the count; with ws (256 bytes or more, which then holds the status
    word) it is asynchronous, nothing is read back, and `out` comes back in full."""
    if not isinstance(pc, PackedColumn):
        raise ValueError(f"pc: expected a PackedColumn, got {type(pc).__name__}")
    fill = _fill_word(fill)
    packed = _need_packed(pc, "pc")
    if rows is None and count is not None:
        raise ValueError("count: given without rows")
    if rows is not None:
        _need(rows, torch.int32, "rows")
    _need_count(count, "count")
    entries = pc.n_rows if rows is None else rows.numel()
    if out is None:
        out = torch.empty(entries, dtype=torch.int32, device=packed.device)
    else:
        _need(out, torch.int32, "out")
        if out.numel() != entries:
            raise ValueError(f"out: {out.numel()} rows, expected {entries}")
    eager = ws is None
    if eager:
        ws = _ws(bitpack_native.workspace_bytes(0), packed.device)
    list_ptr, listed, count_ptr = _column(rows, count)
    if rows is None or listed:  # (an empty list has no address: nothing to do)
        _capi.check(bitpack_native.unpack(packed.data_ptr() if pc.n_rows else None, pc.n_rows, pc.width, pc.base, list_ptr,
                                          count_ptr, listed, bitpack_native.OUTER if outer else 0, fill,
                                          out.data_ptr() if entries else None, ws.data_ptr(), ws.numel(), _stream()),
                    "bitpack_unpack_u32")
    if not eager:
        return out
    _check_status(ws, "bitpack_unpack_u32")
    return out if count is None or not listed else out[: min(max(int(count.item()), 0), entries)]


def select_range_packed(pc: PackedColumn, lo: int, hi: int, rows: torch.Tensor | None = None, signed: bool = False,
                        negate: bool = False) -> torch.Tensor:
    """select_range on a packed column, filtered in its packed form: row ids r with lo <= pc[r] <= hi (lo and hi are
    values, base + code), with the same rules for rows, signed and negate."""
    _bounds(lo, hi, signed)
    packed = _need_packed(pc, "pc")
    if rows is not None:
        _need(rows, torch.int32, "rows")
    plan = SelectRows(pc.n_rows if rows is None else rows.numel(), packed.device)
    plan.launch(pc, lo, hi, rows=rows, signed=signed, negate=negate)
    return plan.result()


# ---------------------------------------------------------------------------------------------
# dwarf 2: radix sort
# ---------------------------------------------------------------------------------------------
class RadixSort:
    def __init__(self, n: int, radix_bits: int = 8, device="cuda"):
        self.n, self.bits = n, radix_bits
        self.ws_bytes = _capi.lib().dbhip_radix_sort_workspace_bytes(n, radix_bits)
        self.ws = _ws(self.ws_bytes, device)
        self.tmp = torch.empty(max(n, 1), dtype=torch.int32, device=device)

    def launch(self, keys: torch.Tensor, signed: bool = False) -> None:
        """Sorts `keys` (int32 storage) in place; signed=False orders the bits as uint32."""
        _need(keys, torch.int32, "keys")
        _need16(keys, "keys")
        if keys.numel() != self.n:
            raise ValueError("size mismatch")
        fn = _capi.lib().dbhip_radix_sort_i32 if signed else _capi.lib().dbhip_radix_sort_u32
        _capi.check(fn(keys.data_ptr(), self.tmp.data_ptr(), self.n, self.bits, self.ws.data_ptr(), self.ws_bytes,
                       _stream()), "radix_sort")


def radix_sort_prepare() -> int:
    """optional calibration (synchronises the current stream once): device-side self-test of the LDS-atomic ranking;
    returns the rank mode the sorts of this device use from now on (1 = LDS atomics, 0 = ballots)"""
    rc = _capi.lib().dbhip_radix_sort_prepare(_stream())
    if rc < 0 or rc > 1:
        _capi.check(rc if rc else -1, "radix_sort_prepare")
    return rc


def radix_sort_(keys: torch.Tensor, signed: bool = False, radix_bits: int = 8) -> torch.Tensor:
    plan = RadixSort(keys.numel(), radix_bits, keys.device)
    plan.launch(keys, signed)
    _check_status(plan.ws, "radix_sort")
    return keys


class RadixSortPairs:
    """Stable key-value sort / argsort plan (dbhip_radix_sort_pairs_*): owns the workspace, both ping-pong buffers and
    the permutation buffer of the argsort."""

    def __init__(self, n: int, radix_bits: int = 8, device="cuda"):
        self.n, self.bits = n, radix_bits
        self.ws_bytes = _capi.lib().dbhip_radix_sort_pairs_workspace_bytes(n, radix_bits)
        self.ws = _ws(self.ws_bytes, device)
        self.tmp_keys = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        self.tmp_vals = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        self.perm = torch.empty(max(n, 1), dtype=torch.int32, device=device)

    def launch(self, keys: torch.Tensor, vals: torch.Tensor | None = None, signed: bool = False) -> torch.Tensor:
        """Asynchronous.  Sorts `keys` in place (signed=False orders the bits as uint32) and carries `vals` along, in
        place; vals=None is the argsort: the stable sort permutation goes to the plan's buffer.  Returns the value
        column (vals, or self.perm[:n]: int32 storage of uint32 ids)."""
        _need(keys, torch.int32, "keys")
        _need16(keys, "keys")
        if keys.numel() != self.n:
            raise ValueError("size mismatch")
        row_ids = vals is None
        if row_ids:
            vals = self.perm[:self.n]
        else:
            _need(vals, torch.int32, "vals")
            _need16(vals, "vals")
            if vals.numel() != self.n:
                raise ValueError("size mismatch")
        fn = _capi.lib().dbhip_radix_sort_pairs_i32 if signed else _capi.lib().dbhip_radix_sort_pairs_u32
        _capi.check(fn(keys.data_ptr(), vals.data_ptr(), self.tmp_keys.data_ptr(), self.tmp_vals.data_ptr(), self.n,
                       self.bits, int(row_ids), self.ws.data_ptr(), self.ws_bytes, _stream()), "radix_sort_pairs")
        return vals


def radix_sort_pairs_(keys: torch.Tensor, vals: torch.Tensor, signed: bool = False, radix_bits: int = 8):
    """Stable sort of (keys, vals) by key, both in place -> (keys, vals)."""
    plan = RadixSortPairs(keys.numel(), radix_bits, keys.device)
    plan.launch(keys, vals, signed)
    _check_status(plan.ws, "radix_sort_pairs")
    return keys, vals


def radix_argsort_(keys: torch.Tensor, signed: bool = False, radix_bits: int = 8) -> torch.Tensor:
    """Sorts `keys` in place and returns the stable sort permutation (int32 storage of uint32 row ids)."""
    plan = RadixSortPairs(keys.numel(), radix_bits, keys.device)
    perm = plan.launch(keys, None, signed)
    _check_status(plan.ws, "radix_sort_pairs")
    return perm


# ---------------------------------------------------------------------------------------------
# top-k: ORDER BY key LIMIT k (include/dbhip_topk.h)
# ---------------------------------------------------------------------------------------------
TOPK_SEGMENT_ROWS = 4096   # DBHIP_TOPK_SEGMENT_ROWS: one wave's rows in the count and write kernels
TOPK_CHUNK_ROWS = 32768    # DBHIP_TOPK_CHUNK_ROWS: one workgroup's rows there


class TopK:
    """Reusable plan for the first min(k, n) rows of a column by key, ties by row (dbhip_topk_*): owns the workspace and
    both output columns."""

    def __init__(self, n: int, k: int, device="cuda"):
        if n < 0 or k < 0:
            raise ValueError("n and k must not be negative")
        self.n, self.k, self.m = n, k, min(k, n)
        self.ws_bytes = _capi.lib().dbhip_topk_workspace_bytes(n, k)
        if n >= 1 << 32:
            raise ValueError("top-k takes fewer than 2^32 rows")
        self.ws = _ws(self.ws_bytes, device)
        self.ws_bytes = self.ws.numel()
        self.out_keys = torch.empty(max(self.m, 1), dtype=torch.int32, device=device)
        self.out_rows = torch.empty(max(self.m, 1), dtype=torch.int32, device=device)

    def launch(self, keys: torch.Tensor, largest: bool = False, signed: bool = False, sorted: bool = True):
        """Asynchronous on the current stream; nothing is read back.  -> (keys, rows) of the first m = min(k, n) rows,
        views of the plan's columns (int32 storage; rows are uint32 ids).  sorted: in key order, ties by row; otherwise
        in ascending row order.  signed=False orders the bits as uint32."""
        _need(keys, torch.int32, "keys")
        _need16(keys, "keys")
        if keys.numel() != self.n:
            raise ValueError("size mismatch")
        fn = _capi.lib().dbhip_topk_i32 if signed else _capi.lib().dbhip_topk_u32
        _capi.check(fn(keys.data_ptr(), self.n, self.k, int(largest), int(sorted), self.out_keys.data_ptr(),
                       self.out_rows.data_ptr(), self.ws.data_ptr(), self.ws_bytes, _stream()), "topk")
        return self.out_keys[:self.m], self.out_rows[:self.m]

    def result(self):
        """-> (keys, rows) of the last launch, after its status word was read (synchronises)"""
        _check_status(self.ws, "topk")
        return self.out_keys[:self.m], self.out_rows[:self.m]


def topk(keys: torch.Tensor, k: int, largest: bool = False, signed: bool = False, sorted: bool = True):
    """-> (keys, rows): the first min(k, n) rows by key (smallest, or largest), equal keys by ascending row"""
    plan = TopK(keys.numel(), k, keys.device)
    plan.launch(keys, largest, signed, sorted)
    return plan.result()


def check_topk(keys: torch.Tensor, out_keys: torch.Tensor, out_rows: torch.Tensor, largest: bool = False,
               signed: bool = False):
    """-> (wrong entries, input rows strictly in front of the last entry) of a SORTED top-k table of k = len(out_keys)
    entries; the table is right iff this is (0, min(k, n) - 1), or (0, 0) for an empty one"""
    for t, name in ((keys, "keys"), (out_keys, "out_keys"), (out_rows, "out_rows")):
        _need(t, torch.int32, name)
    if out_rows.numel() != out_keys.numel():
        raise ValueError("size mismatch")
    res = _result(2, keys.device)
    _capi.check(_capi.lib().dbhip_check_topk_u32(keys.data_ptr(), keys.numel(), out_keys.data_ptr(), out_rows.data_ptr(),
                                                 out_keys.numel(), int(largest), int(signed), res.data_ptr(), _stream()),
                "check_topk_u32")
    return tuple(_u64(res))


# ---------------------------------------------------------------------------------------------
# reduce by key: one row per run of equal adjacent keys; behind the pairs sort, GROUP BY key ORDER BY key
# (include/dbhip_reduce_by_key.h)
# ---------------------------------------------------------------------------------------------
REDUCE_BY_KEY_SEGMENT_ROWS = 4096   # DBHIP_REDUCE_BY_KEY_SEGMENT_ROWS: one wave's rows in the count and reduce kernels
REDUCE_BY_KEY_CHUNK_ROWS = 32768    # DBHIP_REDUCE_BY_KEY_CHUNK_ROWS: one workgroup's rows there


class ReduceByKey:
    """Reusable plan for COUNT, 64-bit SUM, MIN and MAX per run of equal adjacent keys (dbhip_reduce_by_key_u32): owns the
    workspace, the five output columns of `capacity` entries and the run counter.  capacity = 0: the count-only call."""

    def __init__(self, n: int, capacity: int, device="cuda"):
        if n < 0 or capacity < 0:
            raise ValueError("n and capacity must not be negative")
        if n >= 1 << 32:
            raise ValueError("reduce_by_key takes fewer than 2^32 rows")
        self.n, self.capacity = n, capacity
        self.ws_bytes = _capi.lib().dbhip_reduce_by_key_workspace_bytes(n)
        self.ws = _ws(self.ws_bytes, device)
        self.ws_bytes = self.ws.numel()
        cap = max(capacity, 1)
        self.keys = torch.empty(cap, dtype=torch.int32, device=device)
        self.counts = torch.empty(cap, dtype=torch.int32, device=device)
        self.sums = torch.empty(cap, dtype=torch.int64, device=device)
        self.mins = torch.empty(cap, dtype=torch.int32, device=device)
        self.maxs = torch.empty(cap, dtype=torch.int32, device=device)
        self.runs = torch.zeros(1, dtype=torch.int64, device=device)

    def launch(self, keys: torch.Tensor, vals: torch.Tensor | None, signed: bool = False) -> None:
        """Asynchronous on the current stream; nothing is read back (graph-capturable).  signed: the values are int32
        (sign-extended sums, signed min and max).  vals=None: keys and counts only."""
        _need(keys, torch.int32, "keys")
        _need16(keys, "keys")
        if vals is not None:
            _need(vals, torch.int32, "vals")
            _need16(vals, "vals")
        if keys.numel() != self.n or (vals is not None and vals.numel() != self.n):
            raise ValueError("size mismatch")
        some = self.capacity > 0
        with_vals = some and vals is not None
        _capi.check(_capi.lib().dbhip_reduce_by_key_u32(
            keys.data_ptr(), vals.data_ptr() if with_vals else None, self.n, int(signed),
            self.keys.data_ptr() if some else None, self.counts.data_ptr() if some else None,
            self.sums.data_ptr() if with_vals else None, self.mins.data_ptr() if with_vals else None,
            self.maxs.data_ptr() if with_vals else None, self.capacity, self.runs.data_ptr(), self.ws.data_ptr(),
            self.ws_bytes, _stream()), "reduce_by_key_u32")
        self._with_vals = with_vals

    def result(self):
        """-> (keys, counts, sums, mins, maxs) of the last launch, cut to the number of runs (sums: int64 bit patterns;
        the three value columns are None after a launch without vals); raises on a device status (more runs than
        capacity: DBHIP_DEV_TABLE_FULL; self.runs still holds the number)."""
        _check_status(self.ws, "reduce_by_key_u32")
        r = min(int(self.runs.item()), self.capacity)
        if not self._with_vals:
            return self.keys[:r], self.counts[:r], None, None, None
        return self.keys[:r], self.counts[:r], self.sums[:r], self.mins[:r], self.maxs[:r]


def reduce_by_key(keys: torch.Tensor, vals: torch.Tensor, signed: bool = False, capacity: int | None = None):
    """One row per run of equal adjacent keys -> (keys, counts, sums, mins, maxs), cut to the number of runs.  capacity:
    a bound on the number of runs (None: a count-only call finds it first)."""
    if capacity is None:
        count = ReduceByKey(keys.numel(), 0, keys.device)
        count.launch(keys, None)
        _check_status(count.ws, "reduce_by_key_u32")
        capacity = int(count.runs.item())
    plan = ReduceByKey(keys.numel(), capacity, keys.device)
    plan.launch(keys, vals, signed)
    return plan.result()


def groupby_sorted(keys: torch.Tensor, vals: torch.Tensor, signed: bool = False, signed_keys: bool = False):
    """GROUP BY keys ORDER BY keys: -> (distinct keys ascending, COUNT(*), SUM(vals) as int64, MIN(vals), MAX(vals)).  Copies
    both columns, sorts the copies with the stable pairs sort (the values travel with the keys) and reduces the runs.
    signed: the values are int32; signed_keys: the keys ascend as int32."""
    _need(keys, torch.int32, "keys")
    _need(vals, torch.int32, "vals")
    if keys.numel() != vals.numel():
        raise ValueError("size mismatch")
    k, v = keys.clone(), vals.clone()
    radix_sort_pairs_(k, v, signed=signed_keys)
    return reduce_by_key(k, v, signed=signed)


def check_reduce_by_key(keys: torch.Tensor, vals: torch.Tensor, out_keys: torch.Tensor, out_counts: torch.Tensor,
                        out_sums: torch.Tensor, out_mins: torch.Tensor, out_maxs: torch.Tensor, signed: bool = False):
    """-> the four words of dbhip_check_reduce_by_key_u32; the table is right iff the first two are 0 and the last two
    are equal"""
    for t, name in ((keys, "keys"), (vals, "vals"), (out_keys, "out_keys"), (out_counts, "out_counts"),
                    (out_mins, "out_mins"), (out_maxs, "out_maxs")):
        _need(t, torch.int32, name)
    _need(out_sums, torch.int64, "out_sums")
    runs = out_keys.numel()
    if keys.numel() != vals.numel() or any(t.numel() != runs for t in (out_counts, out_sums, out_mins, out_maxs)):
        raise ValueError("size mismatch")
    ws_bytes = _capi.lib().dbhip_check_reduce_by_key_workspace_bytes(keys.numel(), runs)
    ws = _ws(ws_bytes, keys.device)
    res = _result(4, keys.device)
    _capi.check(_capi.lib().dbhip_check_reduce_by_key_u32(
        keys.data_ptr(), vals.data_ptr(), keys.numel(), int(signed), out_keys.data_ptr(), out_counts.data_ptr(),
        out_sums.data_ptr(), out_mins.data_ptr(), out_maxs.data_ptr(), runs, res.data_ptr(), ws.data_ptr(), ws.numel(),
        _stream()), "check_reduce_by_key_u32")
    return tuple(_u64(res))


# ---------------------------------------------------------------------------------------------
# scan by key: one row per input row over runs of equal adjacent keys; behind the pairs sort, the window functions over
# PARTITION BY key ... UNBOUNDED PRECEDING AND CURRENT ROW (include/dbhip_scan_by_key.h)
# ---------------------------------------------------------------------------------------------
SCAN_BY_KEY_SEGMENT_ROWS = 4096   # DBHIP_SCAN_BY_KEY_SEGMENT_ROWS: one wave's rows in the two streaming kernels
SCAN_BY_KEY_CHUNK_ROWS = 32768    # DBHIP_SCAN_BY_KEY_CHUNK_ROWS: one workgroup's rows there
SCAN_BY_KEY_COLUMNS = ("run_ids", "row_numbers", "sums", "mins", "maxs")


class ScanByKey:
    """Reusable plan for the run number, the running COUNT, 64-bit SUM, MIN and MAX of every row over runs of equal adjacent
    keys (dbhip_scan_by_key_u32): owns the workspace and the five output columns of n entries."""

    def __init__(self, n: int, device="cuda"):
        if n < 0:
            raise ValueError("n must not be negative")
        if n >= 1 << 32:
            raise ValueError("scan_by_key takes fewer than 2^32 rows")
        self.n = n
        self.ws_bytes = _capi.lib().dbhip_scan_by_key_workspace_bytes(n)
        self.ws = _ws(self.ws_bytes, device)
        self.ws_bytes = self.ws.numel()
        rows = max(n, 1)
        self.run_ids = torch.empty(rows, dtype=torch.int32, device=device)
        self.row_numbers = torch.empty(rows, dtype=torch.int32, device=device)
        self.sums = torch.empty(rows, dtype=torch.int64, device=device)
        self.mins = torch.empty(rows, dtype=torch.int32, device=device)
        self.maxs = torch.empty(rows, dtype=torch.int32, device=device)
        self._columns = ()

    def launch(self, keys: torch.Tensor, vals: torch.Tensor | None, signed: bool = False,
               columns=SCAN_BY_KEY_COLUMNS) -> None:
        """Asynchronous on the current stream; nothing is read back (graph-capturable).  signed: the values are int32
        (sign-extended sums, signed min and max).  columns: the columns to compute, names of SCAN_BY_KEY_COLUMNS;
        vals=None allows run_ids and row_numbers only."""
        _need(keys, torch.int32, "keys")
        _need16(keys, "keys")
        if vals is not None:
            _need(vals, torch.int32, "vals")
            _need16(vals, "vals")
        if keys.numel() != self.n or (vals is not None and vals.numel() != self.n):
            raise ValueError("size mismatch")
        columns = tuple(columns)
        if not columns or any(c not in SCAN_BY_KEY_COLUMNS for c in columns):
            raise ValueError(f"columns: a non-empty subset of {SCAN_BY_KEY_COLUMNS}")
        if vals is None and any(c in columns for c in SCAN_BY_KEY_COLUMNS[2:]):
            raise ValueError("sums, mins and maxs need vals")
        ptrs = [getattr(self, c).data_ptr() if c in columns else None for c in SCAN_BY_KEY_COLUMNS]
        _capi.check(_capi.lib().dbhip_scan_by_key_u32(
            keys.data_ptr(), vals.data_ptr() if vals is not None else None, self.n, int(signed), *ptrs, self.ws.data_ptr(),
            self.ws_bytes, _stream()), "scan_by_key_u32")
        self._columns = columns

    def result(self):
        """-> (run_ids, row_numbers, sums, mins, maxs) of the last launch (sums: int64 bit patterns; a column that was not
        asked for is None), after the status word was read (synchronises)"""
        _check_status(self.ws, "scan_by_key_u32")
        return tuple(getattr(self, c)[:self.n] if c in self._columns else None for c in SCAN_BY_KEY_COLUMNS)


def scan_by_key(keys: torch.Tensor, vals: torch.Tensor | None, signed: bool = False):
    """One row per input row over runs of equal adjacent keys -> (run_ids, row_numbers, sums, mins, maxs); vals=None:
    (run_ids, row_numbers, None, None, None)"""
    _need(keys, torch.int32, "keys")
    plan = ScanByKey(keys.numel(), keys.device)
    plan.launch(keys, vals, signed, SCAN_BY_KEY_COLUMNS if vals is not None else SCAN_BY_KEY_COLUMNS[:2])
    return plan.result()


def check_scan_by_key(keys: torch.Tensor, vals: torch.Tensor | None, run_ids=None, row_numbers=None, sums=None, mins=None,
                      maxs=None, signed: bool = False):
    """-> the four words of dbhip_check_scan_by_key_u32: (violations, lowest violating row or 2^64 - 1, heads, 0); a column
    that is None is skipped"""
    cols = (run_ids, row_numbers, sums, mins, maxs)
    for t, name in ((keys, "keys"), (vals, "vals"), (run_ids, "run_ids"), (row_numbers, "row_numbers"), (mins, "mins"),
                    (maxs, "maxs")):
        if t is not None:
            _need(t, torch.int32, name)
    if sums is not None:
        _need(sums, torch.int64, "sums")
    n = keys.numel()
    if any(t is not None and t.numel() != n for t in (vals,) + cols):
        raise ValueError("size mismatch")
    ws = _ws(_capi.lib().dbhip_check_scan_by_key_workspace_bytes(n), keys.device)
    res = _result(4, keys.device)
    _capi.check(_capi.lib().dbhip_check_scan_by_key_u32(
        keys.data_ptr(), vals.data_ptr() if vals is not None else None, n, int(signed),
        *(t.data_ptr() if t is not None else None for t in cols), res.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
        "check_scan_by_key_u32")
    return tuple(_u64(res))


def window_sorted(keys: torch.Tensor, vals: torch.Tensor, signed: bool = False, signed_keys: bool = False):
    """The window functions over PARTITION BY keys ORDER BY <row order> ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW
    -> (sorted_keys, row_ids, run_ids, row_numbers, sums, mins, maxs), one entry per input row in (key, row) order.
    Copies the keys, argsorts the copy with the stable pairs sort on row ids, gathers the values and scans by key: the
    sort's stability makes the window order the original row order within each key.  row_ids[j] is the input row of output
    row j (scatter the results back with it); run_ids[j] is its row in groupby_sorted's result.  signed: the values are
    int32; signed_keys: the keys ascend as int32."""
    _need(keys, torch.int32, "keys")
    _need(vals, torch.int32, "vals")
    if keys.numel() != vals.numel():
        raise ValueError("size mismatch")
    k = keys.clone()
    row_ids = radix_argsort_(k, signed=signed_keys)
    v = gather_u32(vals, row_ids)
    return (k, row_ids) + scan_by_key(k, v, signed=signed)


# ---------------------------------------------------------------------------------------------
# sorted search: lower / upper bound of every probe row in a sorted column; behind the stable argsort and in front of
# JoinPairs, the range join b.key BETWEEN p.lo AND p.hi (include/dbhip_sorted_search.h)
# ---------------------------------------------------------------------------------------------
SORTED_SEARCH_FANOUT = 64    # DBHIP_SORTED_SEARCH_FANOUT: entries under one fence
SORTED_SEARCH_TOP = 16384    # DBHIP_SORTED_SEARCH_TOP: default and largest top level


class SortedSearch:
    """Reusable plan for the interval [lo, hi] of every probe row in a sorted column of m entries
    (dbhip_sorted_index_build_u32, dbhip_sorted_search_u32): owns the index workspace and both output columns of n
    entries.  top: the largest top level of the fence ladder, 0 = the default."""

    def __init__(self, m: int, n: int, device="cuda", top: int = 0):
        if m < 0 or n < 0:
            raise ValueError("m and n must not be negative")
        if m > 1 << 31 or n >= 1 << 32:
            raise ValueError("sorted_search takes at most 2^31 sorted entries and fewer than 2^32 probe rows")
        self.m, self.n, self.top = m, n, int(top)
        self.ws_bytes = _capi.lib().dbhip_sorted_index_workspace_bytes(m, self.top)
        if self.ws_bytes == 0:
            raise ValueError(f"top = {top}: 0 or a power of two from 64 to {SORTED_SEARCH_TOP}")
        self.ws = _ws(self.ws_bytes, device)
        self.ws_bytes = self.ws.numel()
        self.pos = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        self.cnt = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        self.sorted = None

    def index(self, sorted: torch.Tensor, signed: bool = False) -> None:
        """Asynchronous: builds the fence ladder over `sorted` (ascending as uint32, or as int32 when signed), which the
        plan keeps a reference to and which must not change before the last search."""
        _need(sorted, torch.int32, "sorted")
        if sorted.numel() != self.m:
            raise ValueError("size mismatch")
        _capi.check(_capi.lib().dbhip_sorted_index_build_u32(
            sorted.data_ptr(), self.m, int(signed), self.top, self.ws.data_ptr(), self.ws_bytes, _stream()),
            "sorted_index_build_u32")
        self.sorted = sorted

    def search(self, lo: torch.Tensor | None, hi: torch.Tensor | None = None) -> None:
        """Asynchronous on the current stream; nothing is read back (graph-capturable).  hi=None: hi = lo; lo=None: minus
        infinity."""
        if self.sorted is None:
            raise ValueError("index() comes first")
        for t, name in ((lo, "lo"), (hi, "hi")):
            if t is not None:
                _need(t, torch.int32, name)
                _need16(t, name)
                if t.numel() != self.n:
                    raise ValueError("size mismatch")
        if lo is None and hi is None:
            raise ValueError("lo or hi")
        _capi.check(_capi.lib().dbhip_sorted_search_u32(
            self.sorted.data_ptr(), self.m, lo.data_ptr() if lo is not None else None,
            hi.data_ptr() if hi is not None else None, self.n, self.pos.data_ptr(), self.cnt.data_ptr(), self.ws.data_ptr(),
            self.ws_bytes, _stream()), "sorted_search_u32")

    def result(self):
        """-> (pos, cnt) of the last search, int32 storage of uint32, after the status word was read (synchronises)"""
        _check_status(self.ws, "sorted_search_u32")
        return self.pos[:self.n], self.cnt[:self.n]


def sorted_search(sorted: torch.Tensor, lo: torch.Tensor | None, hi: torch.Tensor | None = None, signed: bool = False):
    """For every probe row the interval [lo, hi] of the ascending column `sorted` -> (pos, cnt): pos = the number of
    entries < lo (torch.searchsorted side="left"), pos + cnt = the number of entries <= hi (side="right"), cnt = 0 when
    hi < lo.  hi=None: hi = lo, the equality join; lo=None: minus infinity, pos = 0 and pos + cnt - 1 the ASOF row."""
    _need(sorted, torch.int32, "sorted")
    probe = lo if lo is not None else hi
    if probe is None:
        raise ValueError("lo or hi")
    _need(probe, torch.int32, "lo" if lo is not None else "hi")
    plan = SortedSearch(sorted.numel(), probe.numel(), sorted.device)
    plan.index(sorted, signed)
    plan.search(lo, hi)
    return plan.result()


def check_sorted_search(sorted: torch.Tensor, lo: torch.Tensor | None, hi: torch.Tensor | None, pos: torch.Tensor | None,
                        cnt: torch.Tensor | None, signed: bool = False):
    """-> the four words of dbhip_check_sorted_search_u32: (violations, lowest violating row or 2^64 - 1, the sum of cnt,
    0); a column that is None is not judged"""
    cols = ((sorted, "sorted"), (lo, "lo"), (hi, "hi"), (pos, "pos"), (cnt, "cnt"))
    for t, name in cols:
        if t is not None:
            _need(t, torch.int32, name)
    probe = next((t for t, _ in cols[1:] if t is not None), None)
    if probe is None:
        raise ValueError("no probe column")
    n = probe.numel()
    if any(t is not None and t.numel() != n for t, _ in cols[1:]):
        raise ValueError("size mismatch")
    ws = _ws(_capi.lib().dbhip_check_sorted_search_workspace_bytes(n), sorted.device)
    res = _result(4, sorted.device)
    _capi.check(_capi.lib().dbhip_check_sorted_search_u32(
        sorted.data_ptr(), sorted.numel(), int(signed), *(t.data_ptr() if t is not None else None for t, _ in cols[1:3]), n,
        *(t.data_ptr() if t is not None else None for t, _ in cols[3:]), res.data_ptr(), ws.data_ptr(), ws.numel(),
        _stream()), "check_sorted_search_u32")
    return tuple(_u64(res))


def range_join(build_keys: torch.Tensor, probe_lo: torch.Tensor | None, probe_hi: torch.Tensor | None = None,
               left_outer: bool = False, capacity: int | None = None, signed: bool = False):
    """The range join build.key BETWEEN probe.lo AND probe.hi -> (build_rows, probe_rows), one entry per matching pair of
    rows (left_outer: and one with build row -1 per probe row without a match).  probe_hi=None: the equality join;
    probe_lo=None: every build key <= hi.  Copies the build keys, argsorts the copy with the stable pairs sort on row
    ids, builds the fence ladder, searches, and expands with JoinPairs in probe-row order.  The pairs are grouped by probe
    row ascending; inside a row they go by ascending build key, and equal keys by ascending build row, because the sort
    is stable: the result is unique.  capacity=None: a count-only launch, one read-back, an exact allocation, the fill; a
    given capacity: one launch (more pairs than that raise DbhipError, which names the total).  signed: the keys and the
    bounds compare as int32."""
    _need(build_keys, torch.int32, "build_keys")
    probe = probe_lo if probe_lo is not None else probe_hi
    if probe is None:
        raise ValueError("probe_lo or probe_hi")
    _need(probe, torch.int32, "probe_lo" if probe_lo is not None else "probe_hi")
    nb, npr = build_keys.numel(), probe.numel()
    keys = build_keys.clone()
    ids = radix_argsort_(keys, signed=signed)[:nb]
    search = SortedSearch(nb, npr, build_keys.device)
    search.index(keys, signed)
    search.search(probe_lo, probe_hi)
    pos, cnt = search.pos[:npr], search.cnt[:npr]
    if capacity is None:
        counter = JoinPairs(npr, 0, build_keys.device)
        counter.launch(ids, pos, cnt, None, left_outer)
        capacity = counter.count()
    plan = JoinPairs(npr, capacity, build_keys.device)
    plan.launch(ids, pos, cnt, None, left_outer)
    _check_status(search.ws, "sorted_search_u32")
    return plan.result()


# ---------------------------------------------------------------------------------------------
# dwarf 3: group-by SUM
# ---------------------------------------------------------------------------------------------
class GroupBySum:
    def __init__(self, n: int, groups: int, device="cuda"):
        self.n, self.groups = n, groups
        self.ws_bytes = _capi.lib().dbhip_groupby_sum_u32_workspace_bytes(n, groups)
        self.ws = _ws(self.ws_bytes, device)
        self.out = torch.empty(max(groups, 1), dtype=torch.int32, device=device)

    def launch(self, keys: torch.Tensor, vals: torch.Tensor) -> None:
        _need(keys, torch.int32, "keys")
        _need(vals, torch.int32, "vals")
        _need16(keys, "keys")
        _need16(vals, "vals")
        if keys.numel() != self.n or vals.numel() != self.n:
            raise ValueError("size mismatch")
        _capi.check(_capi.lib().dbhip_groupby_sum_u32(keys.data_ptr(), vals.data_ptr(), self.n, self.groups,
                                                      self.out.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                                                      _stream()), "groupby_sum_u32")

    def partial(self, keys: torch.Tensor, vals: torch.Tensor, max_private_tables: int = 0) -> None:
        """phase 1 of groupby/groupby_local.cpp:52-83: privatised partial sums; 0 = let the library choose"""
        _need(keys, torch.int32, "keys")
        _need(vals, torch.int32, "vals")
        _need16(keys, "keys")
        _need16(vals, "vals")
        if keys.numel() != self.n or vals.numel() != self.n:
            raise ValueError("size mismatch")
        _capi.check(_capi.lib().dbhip_groupby_partial_u32(keys.data_ptr(), vals.data_ptr(), self.n, self.groups,
                                                          max_private_tables, self.ws.data_ptr(), self.ws_bytes,
                                                          _stream()), "groupby_partial_u32")

    def merge(self, max_private_tables: int = 0) -> None:
        """phase 2 (groupby_local.cpp:85-112): fold the private tables into the result"""
        _capi.check(_capi.lib().dbhip_groupby_merge_u32(self.groups, max_private_tables, self.out.data_ptr(),
                                                        self.ws.data_ptr(), _stream()), "groupby_merge_u32")

    def result(self) -> torch.Tensor:
        _check_status(self.ws, "groupby_sum_u32")
        return self.out[: self.groups]


def groupby_sum(keys: torch.Tensor, vals: torch.Tensor, groups: int) -> torch.Tensor:
    plan = GroupBySum(keys.numel(), groups, keys.device)
    plan.launch(keys, vals)
    return plan.result()


class GroupByHash:
    """Reusable plan for GROUP BY key SUM(val), COUNT(*) over arbitrary 32-bit keys (dbhip_groupby_hash_u32): owns the
    workspace and the three output columns for n rows and a bound on the distinct keys (max_groups, 0 = n)."""

    def __init__(self, n: int, max_groups: int = 0, device="cuda"):
        if not 0 <= max_groups < 1 << 32:
            raise ValueError("max_groups must fit 32 bits")
        self.n, self.max_groups = n, max_groups
        self.ws_bytes = _capi.lib().dbhip_groupby_hash_workspace_bytes(n, max_groups)
        if self.ws_bytes == 0:
            raise ValueError(f"n = {n} is above the group-by's 2^31 rows")
        self.ws = _ws(self.ws_bytes, device)
        cap = max(max_groups if max_groups else n, 1)
        self.keys = torch.empty(cap, dtype=torch.int32, device=device)
        self.sums = torch.empty(cap, dtype=torch.int32, device=device)
        self.counts = torch.empty(cap, dtype=torch.int32, device=device)
        self.groups = torch.zeros(1, dtype=torch.int64, device=device)
        self._counted = True

    def launch(self, keys: torch.Tensor, vals: torch.Tensor, counts: bool = True) -> None:
        """Asynchronous on the current stream; nothing is read back (graph-capturable)."""
        _need(keys, torch.int32, "keys")
        _need(vals, torch.int32, "vals")
        _need16(keys, "keys")
        _need16(vals, "vals")
        if keys.numel() != self.n or vals.numel() != self.n:
            raise ValueError("size mismatch")
        self._counted = counts
        _capi.check(_capi.lib().dbhip_groupby_hash_u32(keys.data_ptr(), vals.data_ptr(), self.n, self.max_groups,
                                                       self.keys.data_ptr(), self.sums.data_ptr(),
                                                       self.counts.data_ptr() if counts else None, self.groups.data_ptr(),
                                                       self.ws.data_ptr(), self.ws_bytes, _stream()), "groupby_hash_u32")

    def result(self):
        """-> (keys, sums, counts or None), cut to the number of groups; raises on a device status (more distinct keys
        than max_groups: DBHIP_DEV_TABLE_FULL)."""
        _check_status(self.ws, "groupby_hash_u32")
        g = int(self.groups.item())
        return self.keys[:g], self.sums[:g], (self.counts[:g] if self._counted else None)


def groupby_hash(keys: torch.Tensor, vals: torch.Tensor, max_groups: int | None = None, counts: bool = True):
    """GROUP BY keys: -> (distinct keys, SUM(vals), COUNT(*) or None), rows in no particular order, int32 tensors holding
    uint32 bits.  max_groups: a bound on the number of distinct keys (None: n, always correct; a small bound selects the
    faster LDS path)."""
    plan = GroupByHash(keys.numel(), max_groups or 0, keys.device)
    plan.launch(keys, vals, counts=counts)
    return plan.result()


# ---------------------------------------------------------------------------------------------
# dwarf 4a: one-to-many hash join (JoinOmnisci semantics)
# ---------------------------------------------------------------------------------------------
class HashJoin:
    def __init__(self, n_build: int, n_probe: int, device="cuda"):
        self.nb, self.np = n_build, n_probe
        self.ws_bytes = _capi.lib().dbhip_join_workspace_bytes(n_build)
        self.ws = _ws(self.ws_bytes, device)
        self.ids = torch.empty(max(n_build, 1), dtype=torch.int32, device=device)
        self.pos = torch.empty(max(n_probe, 1), dtype=torch.int32, device=device)
        self.cnt = torch.empty(max(n_probe, 1), dtype=torch.int32, device=device)

    def build(self, build_keys: torch.Tensor, row_ids: torch.Tensor | None = None) -> None:
        """row_ids given: the id buffer receives those values (e.g. global row ids) instead of 0..n-1"""
        _need(build_keys, torch.int32, "build_keys")
        if row_ids is None:
            _capi.check(_capi.lib().dbhip_join_build_u32(build_keys.data_ptr(), self.nb, self.ids.data_ptr(),
                                                         self.ws.data_ptr(), self.ws_bytes, _stream()), "join_build_u32")
        else:
            _need(row_ids, torch.int32, "row_ids")
            _capi.check(_capi.lib().dbhip_join_build_pairs_u32(build_keys.data_ptr(), row_ids.data_ptr(), self.nb,
                                                               self.ids.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                                                               _stream()), "join_build_pairs_u32")

    def probe(self, probe_keys: torch.Tensor) -> None:
        _need(probe_keys, torch.int32, "probe_keys")
        _capi.check(_capi.lib().dbhip_join_probe_u32(probe_keys.data_ptr(), self.np, self.ws.data_ptr(),
                                                     self.nb, self.pos.data_ptr(), self.cnt.data_ptr(), _stream()),
                    "join_probe_u32")

    def result(self):
        _check_status(self.ws, "join")
        return self.pos[: self.np], self.cnt[: self.np], self.ids[: self.nb]


class RadixJoin:
    """dwarf 4a without the probe-row-order guarantee: both sides partitioned alike, one fused LDS build + probe launch.
    Results: probe_row_ids / pos / cnt in the probe side's partition order + the id buffer (dbhip_join_radix_*)."""

    def __init__(self, n_build: int, n_probe: int, device="cuda"):
        self.nb, self.np = n_build, n_probe
        self.ws_bytes = _capi.lib().dbhip_join_radix_workspace_bytes(n_build, n_probe)
        self.ws = _ws(self.ws_bytes, device)
        self.ids = torch.empty(max(n_build, 1), dtype=torch.int32, device=device)
        self.rid = torch.empty(max(n_probe, 1), dtype=torch.int32, device=device)
        self.pos = torch.empty(max(n_probe, 1), dtype=torch.int32, device=device)
        self.cnt = torch.empty(max(n_probe, 1), dtype=torch.int32, device=device)

    def _partition(self, side: int, keys: torch.Tensor, row_ids: torch.Tensor | None) -> None:
        _need(keys, torch.int32, "keys")
        if row_ids is not None:
            _need(row_ids, torch.int32, "row_ids")
        _capi.check(_capi.lib().dbhip_join_radix_partition_u32(side, keys.data_ptr(),
                                                               row_ids.data_ptr() if row_ids is not None else None,
                                                               keys.numel(), self.nb, self.np, self.ws.data_ptr(),
                                                               self.ws_bytes, _stream()), "join_radix_partition_u32")

    def partition_build(self, keys: torch.Tensor, row_ids: torch.Tensor | None = None) -> None:
        self._partition(0, keys, row_ids)

    def partition_probe(self, keys: torch.Tensor, row_ids: torch.Tensor | None = None) -> None:
        self._partition(1, keys, row_ids)

    def match(self) -> None:
        _capi.check(_capi.lib().dbhip_join_radix_match_u32(self.nb, self.np, self.ids.data_ptr(), self.rid.data_ptr(),
                                                           self.pos.data_ptr(), self.cnt.data_ptr(), self.ws.data_ptr(),
                                                           self.ws_bytes, _stream()), "join_radix_match_u32")

    def result(self):
        """-> probe_row_ids, pos, cnt (probe partition order), ids"""
        _check_status(self.ws, "join_radix")
        return self.rid[: self.np], self.pos[: self.np], self.cnt[: self.np], self.ids[: self.nb]


def radix_join(build_keys: torch.Tensor, probe_keys: torch.Tensor, build_row_ids: torch.Tensor | None = None,
               probe_row_ids: torch.Tensor | None = None):
    plan = RadixJoin(build_keys.numel(), probe_keys.numel(), build_keys.device)
    plan.partition_build(build_keys, build_row_ids)
    plan.partition_probe(probe_keys, probe_row_ids)
    plan.match()
    return plan.result()


def join_answers(ids: torch.Tensor, pos: torch.Tensor, cnt: torch.Tensor) -> torch.Tensor:
    """(n_probe, 2) int64: the reference's JoinOneToMany records {device pointer into ids, size}
    (common/dpcpp/omnisci_hashtable.hpp:12-17)"""
    _need(ids, torch.int32, "ids")
    _need(pos, torch.int32, "pos")
    _need(cnt, torch.int32, "cnt")
    out = torch.empty((max(pos.numel(), 1), 2), dtype=torch.int64, device=pos.device)
    _capi.check(_capi.lib().dbhip_join_answers_u32(ids.data_ptr(), pos.data_ptr(), cnt.data_ptr(), pos.numel(),
                                                   out.data_ptr(), _stream()), "join_answers_u32")
    return out[: pos.numel()]


def hash_join(build_keys: torch.Tensor, probe_keys: torch.Tensor):
    plan = HashJoin(build_keys.numel(), probe_keys.numel(), build_keys.device)
    plan.build(build_keys)
    plan.probe(probe_keys)
    return plan.result()


def semi_join(build_keys: torch.Tensor, probe_keys: torch.Tensor, anti: bool = False,
              bloom_bits: int | None = None) -> torch.Tensor:
    """EXISTS / IN: the ascending probe row ids with at least one build row of the same key; anti: NOT EXISTS, the
    probe rows with none.  HashJoin.build + probe, then the rows whose match count lies in [1, 0xFFFFFFFF] (outside it
    for anti).  The join's key contract holds: 0xFFFFFFFF is the empty-slot sentinel, a build row carrying it is dropped
    and flagged (DEV_KEY_RANGE: this call raises), a probe row carrying it has no match.
    bloom_bits: a number of filter bits per build key (1 .. 64) puts a Bloom filter of the build keys in front: only
    the probe rows it lets through are joined (their count is read back once, to size the join), and for anti the rows
    it certainly rules out are united with the survivors that found no partner.  The answer is the same tensor."""
    if bloom_bits is not None:
        return _semi_join_prefiltered(build_keys, probe_keys, anti, bloom_bits)
    plan = HashJoin(build_keys.numel(), probe_keys.numel(), build_keys.device)
    plan.build(build_keys)
    plan.probe(probe_keys)
    _, cnt, _ = plan.result()
    return select_range(cnt, 1, 0xFFFFFFFF, negate=anti)


def _semi_join_prefiltered(build_keys: torch.Tensor, probe_keys: torch.Tensor, anti: bool, bloom_bits: int) -> torch.Tensor:
    n_build, n_probe = build_keys.numel(), probe_keys.numel()
    words = bloom_words(n_build, bloom_bits)
    _need(build_keys, torch.int32, "build_keys")
    _need(probe_keys, torch.int32, "probe_keys")
    device = build_keys.device
    bloom = BloomFilter(words, 0, device)
    bloom.build(build_keys)
    sel = SelectRows(n_probe, device)
    sel.launch_in(bloom, probe_keys)
    k = sel.count()  # the one read-back in front of the join: it sizes the join's probe side
    survivors = sel.rows[sel._last][:k]  # ascending probe row ids; the view stays intact through the plan's next call
    kept_keys = TakeRows(k, 1, device)
    kept_keys.launch(probe_keys, survivors)
    join = HashJoin(n_build, k, device)
    join.build(build_keys)
    join.probe(kept_keys.outs[0][:k])
    _, cnt, _ = join.result()
    at = select_range(cnt, 1, 0xFFFFFFFF, negate=anti)  # positions in `survivors`
    rows = take(survivors, at)
    if not anti:
        return rows
    sel.launch_in(bloom, probe_keys, negate=True)  # the rows the filter rules out: no partner, without the join
    certain, certain_count = sel.output()
    sets = RowSets(n_probe, rows.numel(), device)
    sets.launch("union", certain, rows, certain_count, None)
    return sets.result()


class JoinPairs:
    """Reusable plan that turns a one-to-many join answer into the table of (build row, probe row) pairs
    (dbhip_join_pairs_u32): owns the workspace, both output columns (`capacity` entries each) and the device total.
    capacity = 0: a count-only plan, no output columns."""

    def __init__(self, n_probe: int, capacity: int, device="cuda"):
        self.np, self.capacity = n_probe, int(capacity)
        self.ws_bytes = _capi.lib().dbhip_join_pairs_workspace_bytes(n_probe)
        if self.ws_bytes == 0:
            raise ValueError(f"n_probe = {n_probe} is above the join's 2^32 - 1 probe rows")
        self.ws = _ws(self.ws_bytes, device)
        self.build_rows = torch.empty(self.capacity, dtype=torch.int32, device=device) if self.capacity else None
        self.probe_rows = torch.empty(self.capacity, dtype=torch.int32, device=device) if self.capacity else None
        self.total = torch.zeros(1, dtype=torch.int64, device=device)

    def launch(self, ids: torch.Tensor, pos: torch.Tensor, cnt: torch.Tensor, probe_row_ids: torch.Tensor | None = None,
               left_outer: bool = False) -> None:
        """Asynchronous on the current stream; nothing is read back (graph-capturable).  (ids, pos, cnt) as
        HashJoin.result() returns them, or with the probe_row_ids column of RadixJoin.result()."""
        _need(ids, torch.int32, "ids")
        _need(pos, torch.int32, "pos")
        _need(cnt, torch.int32, "cnt")
        if pos.numel() != self.np or cnt.numel() != self.np:
            raise ValueError("size mismatch")
        if probe_row_ids is not None:
            _need(probe_row_ids, torch.int32, "probe_row_ids")
            if probe_row_ids.numel() != self.np:
                raise ValueError("size mismatch")
        _capi.check(_capi.lib().dbhip_join_pairs_u32(
            ids.data_ptr(), ids.numel(), probe_row_ids.data_ptr() if probe_row_ids is not None else None, pos.data_ptr(),
            cnt.data_ptr(), self.np, int(left_outer), self.capacity,
            self.build_rows.data_ptr() if self.capacity else None, self.probe_rows.data_ptr() if self.capacity else None,
            self.total.data_ptr(), self.ws.data_ptr(), self.ws_bytes, _stream()), "join_pairs_u32")

    def count(self) -> int:
        """the total number of pairs of the last launch, whatever the capacity (synchronises)"""
        return int(self.total.item())

    def result(self):
        """-> (build_rows, probe_rows) cut to the total, int32 storage of uint32 row ids (a left-outer miss: -1 as the
        build row); raises on a device status (more pairs than the capacity: DBHIP_DEV_TABLE_FULL)"""
        st = workspace_status(self.ws)
        total = self.count()
        if st & DEV_TABLE_FULL:
            raise _capi.DbhipError(f"join_pairs_u32: device status {st:#x}: {total} pairs are needed, the capacity is "
                                   f"{self.capacity}")
        if st != DEV_OK:
            raise _capi.DbhipError(f"join_pairs_u32: device status {st:#x}")
        if not self.capacity:
            empty = torch.empty(0, dtype=torch.int32, device=self.ws.device)
            return empty, empty.clone()
        return self.build_rows[:total], self.probe_rows[:total]


def join_pairs(build_keys: torch.Tensor, probe_keys: torch.Tensor, left_outer: bool = False, capacity: int | None = None,
               ordered: bool = False):
    """The whole join: -> (build_rows, probe_rows), one entry per matching pair of rows (left_outer: and one with build
    row -1 per probe row without a match).  ordered=False runs RadixJoin: the pairs are grouped by probe row, the probe
    rows stand in partition order; ordered=True runs HashJoin: probe rows ascending.  capacity=None: a count-only launch,
    one read-back, an exact allocation, the fill; a given capacity: one launch and no read-back before the result (more
    pairs than that raise DbhipError, which names the total)."""
    nb, npr = build_keys.numel(), probe_keys.numel()
    if ordered:
        join = HashJoin(nb, npr, build_keys.device)
        join.build(build_keys)
        join.probe(probe_keys)
        rid = None
    else:
        join = RadixJoin(nb, npr, build_keys.device)
        join.partition_build(build_keys)
        join.partition_probe(probe_keys)
        join.match()
        rid = join.rid[:npr]
    ids, pos, cnt = join.ids[:nb], join.pos[:npr], join.cnt[:npr]
    if capacity is None:
        counter = JoinPairs(npr, 0, build_keys.device)
        counter.launch(ids, pos, cnt, rid, left_outer)
        capacity = counter.count()
    plan = JoinPairs(npr, capacity, build_keys.device)
    plan.launch(ids, pos, cnt, rid, left_outer)
    _check_status(join.ws, "join")  # the first read-back when a capacity was given
    return plan.result()


# ---------------------------------------------------------------------------------------------
# dwarf 4b: unique-key payload join (Join semantics)
# ---------------------------------------------------------------------------------------------
class UniqueJoin:
    def __init__(self, n_build: int, n_probe: int, device="cuda"):
        self.nb, self.np = n_build, n_probe
        self.ws_bytes = _capi.lib().dbhip_ujoin_workspace_bytes(n_build)
        self.ws = _ws(self.ws_bytes, device)
        self.out_key = torch.empty(max(n_probe, 1), dtype=torch.int32, device=device)
        self.out_bval = torch.empty_like(self.out_key)
        self.out_pval = torch.empty_like(self.out_key)

    def build(self, keys: torch.Tensor, vals: torch.Tensor) -> None:
        _need(keys, torch.int32, "build_keys")
        _need(vals, torch.int32, "build_vals")
        _capi.check(_capi.lib().dbhip_ujoin_build_u32(keys.data_ptr(), vals.data_ptr(), self.nb, self.ws.data_ptr(),
                                                      self.ws_bytes, _stream()), "ujoin_build_u32")

    def probe(self, keys: torch.Tensor, vals: torch.Tensor) -> None:
        _need(keys, torch.int32, "probe_keys")
        _need(vals, torch.int32, "probe_vals")
        _capi.check(_capi.lib().dbhip_ujoin_probe_u32(keys.data_ptr(), vals.data_ptr(), self.np, self.ws.data_ptr(),
                                                      self.nb, self.out_key.data_ptr(), self.out_bval.data_ptr(),
                                                      self.out_pval.data_ptr(), _stream()), "ujoin_probe_u32")

    def result(self):
        _check_status(self.ws, "ujoin")
        return self.out_key[: self.np], self.out_bval[: self.np], self.out_pval[: self.np]


# ---------------------------------------------------------------------------------------------
# multi-GPU partitioned join: device pieces (the exchange lives in pjoin.py)
# ---------------------------------------------------------------------------------------------
def partition_by_hash(keys: torch.Tensor, first_row_id: int, parts: int):
    """-> (keys bucket-major, global row ids bucket-major, counts[parts] int64 on the device)"""
    _need(keys, torch.int32, "keys")
    n = keys.numel()
    lib = _capi.lib()
    ws_bytes = lib.dbhip_pjoin_partition_workspace_bytes(n, parts)
    ws = _ws(ws_bytes, keys.device)
    out_keys = torch.empty(max(n, 1), dtype=torch.int32, device=keys.device)
    out_rids = torch.empty(max(n, 1), dtype=torch.int32, device=keys.device)
    counts = torch.zeros(parts, dtype=torch.int64, device=keys.device)
    _capi.check(lib.dbhip_pjoin_partition_u32(keys.data_ptr(), n, first_row_id, parts, out_keys.data_ptr(),
                                              out_rids.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws_bytes,
                                              _stream()), "pjoin_partition_u32")
    return out_keys[:n], out_rids[:n], counts


def gather_u32(table: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    _need(table, torch.int32, "table")
    _need(idx, torch.int32, "idx")
    out = torch.empty(max(idx.numel(), 1), dtype=torch.int32, device=idx.device)
    _capi.check(_capi.lib().dbhip_gather_u32(table.data_ptr(), idx.data_ptr(), idx.numel(), out.data_ptr(), _stream()),
                "gather_u32")
    return out[: idx.numel()]


# ---------------------------------------------------------------------------------------------
# reduce and nested-loop join (reduce/reduce.cpp, join/nested_join.cpp)
# ---------------------------------------------------------------------------------------------
def reduce_sum(src: torch.Tensor) -> torch.Tensor:
    """one-element int32 tensor: the wrap-around sum of src"""
    _need(src, torch.int32, "src")
    out = torch.empty(1, dtype=torch.int32, device=src.device)
    _capi.check(_capi.lib().dbhip_reduce_sum_i32(src.data_ptr(), src.numel(), out.data_ptr(), _stream()), "reduce_sum_i32")
    return out


def nested_join(a_keys: torch.Tensor, a_vals: torch.Tensor, b_keys: torch.Tensor, b_vals: torch.Tensor):
    """dense (n_a x n_b) cell matrices (key, a_val, b_val); empty cells are (0, -1, -1)"""
    for t, name in ((a_keys, "a_keys"), (a_vals, "a_vals"), (b_keys, "b_keys"), (b_vals, "b_vals")):
        _need(t, torch.int32, name)
    na, nb = a_keys.numel(), b_keys.numel()
    if a_vals.numel() != na or b_vals.numel() != nb:
        raise ValueError("size mismatch")
    outs = [torch.empty(max(na * nb, 1), dtype=torch.int32, device=a_keys.device) for _ in range(3)]
    _capi.check(_capi.lib().dbhip_nested_join_u32(a_keys.data_ptr(), a_vals.data_ptr(), b_keys.data_ptr(),
                                                  b_vals.data_ptr(), na, nb, outs[0].data_ptr(), outs[1].data_ptr(),
                                                  outs[2].data_ptr(), _stream()), "nested_join_u32")
    return tuple(o[: na * nb].view(na, nb) if na and nb else o[:0] for o in outs)


# ---------------------------------------------------------------------------------------------
# bitmask-claimed table (SimpleNonOwningHashTable counterpart)
# ---------------------------------------------------------------------------------------------
class BitmaskTable:
    def __init__(self, table_size: int, hash_kind: int = 1, seed: int = 0, device="cuda"):
        self.size, self.kind, self.seed = table_size, hash_kind, seed
        self.ws_bytes = _capi.lib().dbhip_bitmask_table_workspace_bytes(table_size)
        self.ws = _ws(self.ws_bytes, device)
        self.reset()

    def reset(self) -> None:
        _capi.check(_capi.lib().dbhip_bitmask_table_reset(self.ws.data_ptr(), self.ws_bytes, self.size, _stream()),
                    "bitmask_table_reset")

    def insert(self, keys: torch.Tensor, vals: torch.Tensor, serial: bool = False) -> None:
        _need(keys, torch.int32, "keys")
        _need(vals, torch.int32, "vals")
        _capi.check(_capi.lib().dbhip_bitmask_table_insert_u32(keys.data_ptr(), vals.data_ptr(), keys.numel(),
                                                               self.ws.data_ptr(), self.ws_bytes, self.size, self.kind,
                                                               self.seed, int(serial), _stream()), "bitmask_table_insert")

    def lookup(self, keys: torch.Tensor):
        _need(keys, torch.int32, "keys")
        n = keys.numel()
        vals = torch.empty(max(n, 1), dtype=torch.int32, device=keys.device)
        found = torch.empty(max(n, 1), dtype=torch.int32, device=keys.device)
        _capi.check(_capi.lib().dbhip_bitmask_table_lookup_u32(keys.data_ptr(), n, self.ws.data_ptr(), self.size,
                                                               self.kind, self.seed, vals.data_ptr(), found.data_ptr(),
                                                               _stream()), "bitmask_table_lookup")
        return vals[:n], found[:n]

    def check(self) -> None:
        """raise if an insert found the table full (DEV_TABLE_FULL)"""
        _check_status(self.ws, "bitmask_table")

    def slot_values(self) -> torch.Tensor:
        """the payload array of the table (for slot-level known-answer tests)"""
        off = 256 + 4 * self.size
        return self.ws[off: off + 4 * self.size].view(torch.int32)


# ---------------------------------------------------------------------------------------------
# cuckoo table (CuckooHashtable counterpart, common/dpcpp/cuckoo_hashtable.hpp)
# ---------------------------------------------------------------------------------------------
def cuckoo_seed_pair(seed: int, attempt: int) -> tuple[int, int]:
    """The (seed1, seed2) of build attempt `attempt`: the low words of splitmix64(seed, 2a) and (seed, 2a + 1), seed2
    nudged off seed1.  The reference draws them at random (helpers::make_random); a fixed sequence makes a failing build
    reproducible.  CuckooHashBuildHip (host/hip_dwarfs.cpp) uses the same sequence."""
    m = (1 << 64) - 1

    def mix(i: int) -> int:
        z = ((i + 1) * 0x9E3779B97F4A7C15 + seed * 0xD1B54A32D192ED03) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return (z ^ (z >> 31)) & 0xFFFFFFFF

    s1, s2 = mix(2 * attempt), mix(2 * attempt + 1)
    return s1, (s2 ^ 1 if s2 == s1 else s2)


class CuckooTable:
    """Two-choice cuckoo table of `table_size` 8-byte slots.  hash_kind 0: (k % size + seed) % size, 1: Murmur3(k, seed)
    % size (the reference's hasher), 2: (mix64(seed, k) >> 32) % size (include/dbhip.h: kind 1 cannot hold millions of
    keys); seeds = (seed1, seed2) make h1 and h2.  insert() is asynchronous; failed() / status() synchronise."""

    def __init__(self, table_size: int, hash_kind: int = 1, seeds: tuple[int, int] = (0, 1), device="cuda"):
        self.size, self.kind = table_size, hash_kind
        self.seeds = (seeds[0] & 0xFFFFFFFF, seeds[1] & 0xFFFFFFFF)
        self.ws_bytes = _capi.lib().dbhip_cuckoo_table_workspace_bytes(table_size)
        self.ws = _ws(self.ws_bytes, device)
        self.reset()

    def reset(self) -> None:
        """empty every slot and clear the status word"""
        _capi.check(_capi.lib().dbhip_cuckoo_table_reset(self.ws.data_ptr(), self.ws_bytes, self.size, _stream()),
                    "cuckoo_table_reset")

    def insert(self, keys: torch.Tensor, vals: torch.Tensor, serial: bool = False, max_iter: int = 0,
               want_results: bool = False):
        """insert (keys[i], vals[i]); max_iter = exchanges per row before it gives up (0: min(n, 100000)).
        want_results: returns an int32 tensor, 1 where the row was stored."""
        _need(keys, torch.int32, "keys")
        _need(vals, torch.int32, "vals")
        n = keys.numel()
        if vals.numel() != n:
            raise ValueError("keys and vals differ in length")
        res = torch.empty(max(n, 1), dtype=torch.int32, device=keys.device) if want_results else None
        _capi.check(_capi.lib().dbhip_cuckoo_table_insert_u32(
            keys.data_ptr(), vals.data_ptr(), n, self.ws.data_ptr(), self.ws_bytes, self.size, self.kind, self.seeds[0],
            self.seeds[1], max_iter, int(serial), res.data_ptr() if want_results else None, _stream()),
            "cuckoo_table_insert")
        return res[:n] if want_results else None

    def status(self) -> int:
        """the device status word since the last reset (synchronises): DEV_TABLE_FULL, DEV_KEY_RANGE"""
        return workspace_status(self.ws)

    def failed(self) -> bool:
        """True if a row since the last reset gave up (its eviction chain reached max_iter, a pair was dropped)"""
        return bool(self.status() & DEV_TABLE_FULL)

    def lookup(self, keys: torch.Tensor):
        """(vals, found): the value stored with each key (0 when missing) and 1 / 0"""
        _need(keys, torch.int32, "keys")
        n = keys.numel()
        vals = torch.empty(max(n, 1), dtype=torch.int32, device=keys.device)
        found = torch.empty(max(n, 1), dtype=torch.int32, device=keys.device)
        _capi.check(_capi.lib().dbhip_cuckoo_table_lookup_u32(keys.data_ptr(), n, self.ws.data_ptr(), self.size, self.kind,
                                                              self.seeds[0], self.seeds[1], vals.data_ptr(),
                                                              found.data_ptr(), _stream()), "cuckoo_table_lookup")
        return vals[:n], found[:n]

    def slots(self):
        """(keys, vals) of every slot; an empty slot is (-1, 0) (key 0xFFFFFFFF)"""
        keys = torch.empty(self.size, dtype=torch.int32, device=self.ws.device)
        vals = torch.empty(self.size, dtype=torch.int32, device=self.ws.device)
        _capi.check(_capi.lib().dbhip_cuckoo_table_export_u32(self.ws.data_ptr(), self.size, keys.data_ptr(),
                                                              vals.data_ptr(), _stream()), "cuckoo_table_export")
        return keys, vals


def cuckoo_build(keys: torch.Tensor, vals: torch.Tensor, table_size: int | None = None, max_attempts: int = 16,
                 seed: int = 0, hash_kind: int = 2):
    """Build a cuckoo table over (keys, vals), rebuilding with the next seed pair (cuckoo_seed_pair(seed, attempt))
    while an insert reports a dropped pair, as hash/cuckoo_hash_build.cpp:43-92 does.  table_size defaults to 4 * n
    (:14).  hash_kind defaults to 2: with the reference's Murmur3 pair (1) large builds fail for every seed pair.
    Returns (table, attempts); raises after max_attempts failed builds, and at once on any other device status."""
    n = keys.numel()
    size = table_size if table_size is not None else max(4 * n, 1)
    table = None
    for attempt in range(max_attempts):
        seeds = cuckoo_seed_pair(seed, attempt)
        if table is None:
            table = CuckooTable(size, hash_kind, seeds, device=keys.device)
        else:
            table.seeds = seeds
            table.reset()
        table.insert(keys, vals)
        st = table.status()
        if st == DEV_OK:
            return table, attempt + 1
        if st != DEV_TABLE_FULL:
            raise _capi.DbhipError(f"cuckoo_build: device status {st:#x}")
    raise _capi.DbhipError(f"cuckoo_build: {max_attempts} attempts failed at {n} keys in {size} slots")


# ---------------------------------------------------------------------------------------------
# slab table (SlabHashTable counterpart, common/dpcpp/slab_hash.hpp)
# ---------------------------------------------------------------------------------------------
SLAB_HASHER_BUILD = (242792921, 653019598, 2147483647)  # DefaultHasher of SlabHashBuild / SlabProbe
SLAB_HASHER_JOIN = (32, 48, 1031)                       # join/slab_join.cpp:72, :100
SLAB_HASHER_TESTS = (13, 24, 343)                       # tests/slab_tests.cpp
SLAB_MAX_GROUPS = 1 << 14  # DBHIP_SLAB_INSERT_GROUPS: the most pool nodes one concurrent insert leaves unlinked


def slab_buckets(n: int) -> int:
    """calculate_buckets_count(n, 60) = n / (32 * 0.625) = n // 20 (slab_hash.hpp:30-58), but at least 1: the reference
    takes % 0 below 20 rows"""
    return max(1, n // 20)


class SlabTable:
    """Slab hash table: `buckets` chains of 32-slot slabs, nodes [buckets, buckets + pool_nodes) the overflow pool.
    hasher = (A, B, P): bucket = ((A*k + B) % P) % buckets.  A multimap; insert() is asynchronous, status() / failed()
    synchronise.  A concurrent insert may leave one pool node per group unlinked: a pool of ceil(rows / 32) +
    SLAB_MAX_GROUPS nodes holds any input."""

    def __init__(self, buckets: int, pool_nodes: int, hasher=SLAB_HASHER_BUILD, device="cuda"):
        self.buckets, self.pool = int(buckets), int(pool_nodes)
        self.hasher = tuple(int(x) for x in hasher)
        self.ws_bytes = _capi.lib().dbhip_slab_table_workspace_bytes(self.buckets, self.pool)
        if self.ws_bytes == 0:
            raise ValueError(f"SlabTable: bad geometry ({buckets} buckets, {pool_nodes} pool nodes)")
        self.ws = _ws(self.ws_bytes, device)
        self.reset()

    @property
    def nodes(self) -> int:
        return self.buckets + self.pool

    def reset(self) -> None:
        """empty every slab, unlink every node, clear the pool cursor and the status word"""
        _capi.check(_capi.lib().dbhip_slab_table_reset(self.ws.data_ptr(), self.ws_bytes, self.buckets, self.pool,
                                                       _stream()), "slab_table_reset")

    def insert(self, keys: torch.Tensor, vals: torch.Tensor, serial: bool = False, want_results: bool = False):
        """insert (keys[i], vals[i]); serial: one group in input order (the reference's sequential layout).
        want_results: returns an int32 tensor, 1 where the row was stored."""
        _need(keys, torch.int32, "keys")
        _need(vals, torch.int32, "vals")
        n = keys.numel()
        if vals.numel() != n:
            raise ValueError("keys and vals differ in length")
        res = torch.empty(max(n, 1), dtype=torch.int32, device=keys.device) if want_results else None
        a, b, p = self.hasher
        _capi.check(_capi.lib().dbhip_slab_table_insert_u32(
            keys.data_ptr(), vals.data_ptr(), n, self.ws.data_ptr(), self.ws_bytes, self.buckets, self.pool, a, b, p,
            int(serial), res.data_ptr() if want_results else None, _stream()), "slab_table_insert")
        return res[:n] if want_results else None

    def status(self) -> int:
        """the device status word since the last reset (synchronises): DEV_TABLE_FULL, DEV_KEY_RANGE, DEV_SPIN_TIMEOUT"""
        return workspace_status(self.ws)

    def failed(self) -> bool:
        """True if a row since the last reset was not stored for want of pool nodes"""
        return bool(self.status() & DEV_TABLE_FULL)

    def lookup(self, keys: torch.Tensor):
        """(vals, found): the value of the first slot in chain order holding each key (0 when missing) and 1 / 0"""
        _need(keys, torch.int32, "keys")
        n = keys.numel()
        vals = torch.empty(max(n, 1), dtype=torch.int32, device=keys.device)
        found = torch.empty(max(n, 1), dtype=torch.int32, device=keys.device)
        a, b, p = self.hasher
        _capi.check(_capi.lib().dbhip_slab_table_lookup_u32(keys.data_ptr(), n, self.ws.data_ptr(), self.buckets,
                                                            self.pool, a, b, p, vals.data_ptr(), found.data_ptr(),
                                                            _stream()), "slab_table_lookup")
        return vals[:n], found[:n]

    def join_probe(self, keys: torch.Tensor, vals: torch.Tensor):
        """(key, build value, probe value) per probe row, all -1 (0xFFFFFFFF) on a miss"""
        _need(keys, torch.int32, "keys")
        _need(vals, torch.int32, "vals")
        n = keys.numel()
        if vals.numel() != n:
            raise ValueError("keys and vals differ in length")
        out = torch.empty((3, max(n, 1)), dtype=torch.int32, device=keys.device)
        a, b, p = self.hasher
        _capi.check(_capi.lib().dbhip_slab_table_join_probe_u32(
            keys.data_ptr(), vals.data_ptr(), n, self.ws.data_ptr(), self.buckets, self.pool, a, b, p,
            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _stream()), "slab_table_join_probe")
        return out[0, :n], out[1, :n], out[2, :n]

    def slabs(self):
        """(keys [nodes, 32], vals [nodes, 32], next [nodes], pool_used): the layout; an empty slot is (-1, 0), a
        missing link -1"""
        dev = self.ws.device
        keys = torch.empty((self.nodes, 32), dtype=torch.int32, device=dev)
        vals = torch.empty((self.nodes, 32), dtype=torch.int32, device=dev)
        nxt = torch.empty(self.nodes, dtype=torch.int32, device=dev)
        used = torch.empty(1, dtype=torch.int32, device=dev)
        _capi.check(_capi.lib().dbhip_slab_table_export_u32(self.ws.data_ptr(), self.buckets, self.pool,
                                                            keys.data_ptr(), vals.data_ptr(), nxt.data_ptr(),
                                                            used.data_ptr(), _stream()), "slab_table_export")
        return keys, vals, nxt, int(used.cpu()[0])


def slab_join(build_keys: torch.Tensor, build_vals: torch.Tensor, probe_keys: torch.Tensor,
              probe_vals: torch.Tensor, hasher=SLAB_HASHER_BUILD):
    """SlabJoin (join/slab_join.cpp:10-144): build a slab table over (build_keys, build_vals), probe it with every probe
    row, and return (keys, build_vals, probe_vals) of the hit rows in probe-row order.  A probe key that occurs more than
    once in the build side meets the first of its rows in chain order (find()).  Key 0 is a key like any other; key
    0xFFFFFFFF (-1) cannot be stored.  Sized by slab_buckets with a pool that holds any input, not the reference's fixed
    1024 buckets and 20000-node heap."""
    n = build_keys.numel()
    table = SlabTable(slab_buckets(n), -(-n // 32) + SLAB_MAX_GROUPS, hasher, device=build_keys.device)
    table.insert(build_keys, build_vals)
    _check_status(table.ws, "slab_join build")
    k, bv, pv = table.join_probe(probe_keys, probe_vals)
    hit = k != -1
    return k[hit], bv[hit], pv[hit]


# ---------------------------------------------------------------------------------------------
# exclusive prefix sum (scan/scan.cl:44-66, tests/scan_tests.cpp:14-21, dpl_wrapper.hpp:18-25)
# ---------------------------------------------------------------------------------------------
class ExclusiveScan:
    """launch() is asynchronous; result() synchronises and raises on a device-side status (the single-launch path waits
    on other workgroups with a bounded spin: DBHIP_DEV_SPIN_TIMEOUT means the prefix that was written is wrong)"""

    def __init__(self, n: int, device="cuda"):
        self.n = n
        self.ws_bytes = _capi.lib().dbhip_exclusive_scan_u32_workspace_bytes(n)
        self.ws = _ws(self.ws_bytes, device)
        self.out = None

    def launch(self, src: torch.Tensor, init: int = 0, out: torch.Tensor | None = None) -> None:
        _need(src, torch.int32, "src")
        assert src.numel() == self.n
        if out is None:
            out = torch.empty(max(self.n, 1), dtype=torch.int32, device=src.device)[: self.n]
        _need(out, torch.int32, "out")
        self.out = out
        _capi.check(_capi.lib().dbhip_exclusive_scan_u32(src.data_ptr(), self.n, init & 0xFFFFFFFF, out.data_ptr(),
                                                         self.ws.data_ptr(), self.ws_bytes, _stream()), "exclusive_scan_u32")

    def result(self) -> torch.Tensor:
        _check_status(self.ws, "exclusive_scan_u32")
        return self.out


def exclusive_scan(src: torch.Tensor, init: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """out[0] = init, out[i] = init + src[0] + ... + src[i-1] (uint32 wrap-around); out may be src.  Checked: reads the
    workspace's status word back (one synchronisation); use ExclusiveScan for asynchronous launches."""
    plan = ExclusiveScan(src.numel(), src.device)
    plan.launch(src, init, out)
    return plan.result()


# ---------------------------------------------------------------------------------------------
# device-side validators (what the ...Hip dwarfs use for Result::valid at large sizes)
# ---------------------------------------------------------------------------------------------
def _result(words: int, device) -> torch.Tensor:
    return torch.empty(words, dtype=torch.int64, device=device)


def _u64(t: torch.Tensor):
    return [int(x) & 0xFFFFFFFFFFFFFFFF for x in t.cpu().tolist()]


def check_fingerprint_lt(src: torch.Tensor, filter_value: int):
    """-> (fingerprint, length) of the subsequence of src with x < filter_value, order-sensitive"""
    _need(src, torch.int32, "src")
    lib = _capi.lib()
    ws_bytes = lib.dbhip_check_fingerprint_workspace_bytes(src.numel())
    ws = _ws(ws_bytes, src.device)
    res = _result(2, src.device)
    _capi.check(lib.dbhip_check_fingerprint_lt_i32(src.data_ptr(), src.numel(), filter_value, res.data_ptr(), ws.data_ptr(),
                                                   ws_bytes, _stream()), "check_fingerprint_lt_i32")
    return tuple(_u64(res))


def check_sorted(keys: torch.Tensor, signed: bool = False):
    """-> (descents, multiset fingerprint, key sum)"""
    _need(keys, torch.int32, "keys")
    res = _result(3, keys.device)
    _capi.check(_capi.lib().dbhip_check_sorted_u32(keys.data_ptr(), keys.numel(), int(signed), res.data_ptr(), _stream()),
                "check_sorted_u32")
    return tuple(_u64(res))


def check_sorted_pairs(keys_in: torch.Tensor, keys_out: torch.Tensor, ids_out: torch.Tensor, signed: bool = False):
    """-> (descents of the (key, id) pairs, ids out of range or naming a row with another key); (0, 0) iff ids_out is
    the stable sort permutation of keys_in and keys_out the sorted column"""
    for t, name in ((keys_in, "keys_in"), (keys_out, "keys_out"), (ids_out, "ids_out")):
        _need(t, torch.int32, name)
    if keys_out.numel() != keys_in.numel() or ids_out.numel() != keys_in.numel():
        raise ValueError("size mismatch")
    res = _result(2, keys_in.device)
    _capi.check(_capi.lib().dbhip_check_sorted_pairs_u32(keys_in.data_ptr(), keys_out.data_ptr(), ids_out.data_ptr(),
                                                         keys_in.numel(), int(signed), res.data_ptr(), _stream()),
                "check_sorted_pairs_u32")
    return tuple(_u64(res))


def check_weighted_sum(keys: torch.Tensor | None, vals: torch.Tensor):
    """-> two 32-bit weighted sums of vals, weights drawn from keys (None: the index)"""
    _need(vals, torch.int32, "vals")
    if keys is not None:
        _need(keys, torch.int32, "keys")
    res = _result(2, vals.device)
    _capi.check(_capi.lib().dbhip_check_weighted_sum_u32(keys.data_ptr() if keys is not None else None, vals.data_ptr(),
                                                         vals.numel(), res.data_ptr(), _stream()), "check_weighted_sum_u32")
    return tuple(_u64(res))


def check_distinct(keys: torch.Tensor) -> int:
    """-> number of i with s[i] >= s[i+1] over a sorted copy s of keys (0 iff the keys are distinct)"""
    _need(keys, torch.int32, "keys")
    lib = _capi.lib()
    ws_bytes = lib.dbhip_check_distinct_workspace_bytes(keys.numel())
    ws = _ws(ws_bytes, keys.device)
    res = _result(1, keys.device)
    _capi.check(lib.dbhip_check_distinct_u32(keys.data_ptr(), keys.numel(), res.data_ptr(), ws.data_ptr(), ws_bytes,
                                             _stream()), "check_distinct_u32")
    return _u64(res)[0]


def check_permutation(ids: torch.Tensor) -> int:
    """-> number of entries that are out of range or repeated (0 iff ids is a permutation of 0..n-1)"""
    _need(ids, torch.int32, "ids")
    lib = _capi.lib()
    ws_bytes = lib.dbhip_check_permutation_workspace_bytes(ids.numel())
    ws = _ws(ws_bytes, ids.device)
    res = _result(1, ids.device)
    _capi.check(lib.dbhip_check_permutation_u32(ids.data_ptr(), ids.numel(), res.data_ptr(), ws.data_ptr(), ws_bytes,
                                                _stream()), "check_permutation_u32")
    return _u64(res)[0]


def check_join(sorted_build: torch.Tensor, probe: torch.Tensor, pos: torch.Tensor, cnt: torch.Tensor, ids: torch.Tensor,
               build_keys: torch.Tensor | None = None, gen=(0, 0, 0)):
    """-> (bad probe rows, sum of counts); build_keys None: ids are global row ids of gen = (seed, lo, hi)"""
    for t, name in ((sorted_build, "sorted_build"), (probe, "probe"), (pos, "pos"), (cnt, "cnt"), (ids, "ids")):
        _need(t, torch.int32, name)
    res = _result(2, probe.device)
    _capi.check(_capi.lib().dbhip_check_join_u32(sorted_build.data_ptr(), sorted_build.numel(), probe.data_ptr(),
                                                 probe.numel(), pos.data_ptr(), cnt.data_ptr(), ids.data_ptr(),
                                                 build_keys.data_ptr() if build_keys is not None else None,
                                                 gen[0], gen[1], gen[2], res.data_ptr(), _stream()), "check_join_u32")
    return tuple(_u64(res))


def check_join_pairs(build_keys: torch.Tensor, probe_keys: torch.Tensor, ids: torch.Tensor, pos: torch.Tensor,
                     cnt: torch.Tensor, build_rows: torch.Tensor, probe_rows: torch.Tensor,
                     probe_row_ids: torch.Tensor | None = None, left_outer: bool = False):
    """-> (bad pairs, pairs expected, fingerprint of the pairs given, fingerprint expected); the pair table is right iff
    the first is 0, the second equals build_rows.numel() and the last two are equal.  Row ids are row indices into the
    key columns."""
    for t, name in ((build_keys, "build_keys"), (probe_keys, "probe_keys"), (ids, "ids"), (pos, "pos"), (cnt, "cnt"),
                    (build_rows, "build_rows"), (probe_rows, "probe_rows")):
        _need(t, torch.int32, name)
    if probe_row_ids is not None:
        _need(probe_row_ids, torch.int32, "probe_row_ids")
    if probe_rows.numel() != build_rows.numel() or pos.numel() != probe_keys.numel() or cnt.numel() != probe_keys.numel():
        raise ValueError("size mismatch")
    res = _result(4, probe_keys.device)
    _capi.check(_capi.lib().dbhip_check_join_pairs_u32(
        build_keys.data_ptr(), build_keys.numel(), probe_keys.data_ptr(), probe_keys.numel(), ids.data_ptr(),
        probe_row_ids.data_ptr() if probe_row_ids is not None else None, pos.data_ptr(), cnt.data_ptr(), int(left_outer),
        build_rows.data_ptr(), probe_rows.data_ptr(), build_rows.numel(), res.data_ptr(), _stream()),
        "check_join_pairs_u32")
    return tuple(_u64(res))


def check_ujoin(sorted_build: torch.Tensor, build_vals: torch.Tensor, probe: torch.Tensor, probe_vals: torch.Tensor,
                out_key: torch.Tensor, out_bval: torch.Tensor, out_pval: torch.Tensor):
    """-> (bad probe rows, hits)"""
    res = _result(2, probe.device)
    _capi.check(_capi.lib().dbhip_check_ujoin_u32(sorted_build.data_ptr(), build_vals.data_ptr(), sorted_build.numel(),
                                                  probe.data_ptr(), probe_vals.data_ptr(), probe.numel(),
                                                  out_key.data_ptr(), out_bval.data_ptr(), out_pval.data_ptr(),
                                                  res.data_ptr(), _stream()), "check_ujoin_u32")
    return tuple(_u64(res))


def check_gen_uniform(values: torch.Tensor, seed: int, lo: int, hi: int, first_index: int = 0,
                      indices: torch.Tensor | None = None) -> int:
    """-> number of values that differ from lo + mix64(seed, index) % (hi - lo + 1)"""
    _need(values, torch.int32, "values")
    res = _result(1, values.device)
    _capi.check(_capi.lib().dbhip_check_gen_uniform_u32(values.data_ptr(), indices.data_ptr() if indices is not None else None,
                                                        values.numel(), seed, first_index, lo, hi, res.data_ptr(),
                                                        _stream()), "check_gen_uniform_u32")
    return _u64(res)[0]
