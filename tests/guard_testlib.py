"""Test-only helpers that see where a kernel writes: buffers of exactly the size a call is entitled to, with guard bytes
directly in front of them and directly behind them in the same allocation, and frozen copies of input columns.  The
int32 columns are join_testlib.guarded / assert_guards; this module adds byte workspaces, uint64 result words and a
collector that checks all buffers of one call.  Never imported by the product.

Guards around an INPUT column serve a second purpose: a kernel that reads past the end of its input and uses what it
read gives different answers under the two FILLS, so every test runs under both and wants the oracle's answer twice."""
import numpy as np
import torch

from tests import join_testlib as jt

FILLS = (0x5A5A5A5A, 0xA5A5A5A5)
GUARD_BYTES = 4096  # in front of and behind a byte workspace or a run of uint64 words
COL_GUARD_WORDS = 1024  # around an int32 column, on top of join_testlib.GUARD_WORDS
WS_ALIGN = 256      # include/dbhip.h: a workspace starts on a 256-byte boundary


def i32(word):
    """a 32-bit pattern as the int32 value torch wants (0xA5A5A5A5 is negative)"""
    word &= 0xFFFFFFFF
    return word - (1 << 32) if word >> 31 else word


def i64(word):
    """the 32-bit pattern twice, as the int64 value torch wants"""
    both = (word & 0xFFFFFFFF) * 0x100000001
    return both - (1 << 64) if both >> 63 else both


def ptr(t):
    """the address of a tensor's first element, also for an empty view (whose data_ptr() torch reports as 0): a call
    at n = 0 still gets a pointer into its guarded allocation"""
    return t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()


def _pattern(fill, first, count, device):
    """bytes [first, first + count) of the little-endian fill word repeated from byte 0 of an allocation"""
    four = torch.tensor([(fill >> (8 * b)) & 0xFF for b in range(4)], dtype=torch.uint8, device=device)
    return four[(torch.arange(first, first + count, device=device) & 3)]


def guarded_bytes(nbytes, fill, device="cuda"):
    """-> (base, view): a uint8 workspace view of exactly `nbytes` bytes that starts on a 256-byte boundary, inside a
    fresh allocation whose other bytes — at least GUARD_BYTES on each side — repeat the fill word.  The guard behind
    starts at byte `nbytes` of the view, whatever nbytes is."""
    words = (2 * GUARD_BYTES + WS_ALIGN + int(nbytes) + 3) // 4
    base = torch.full((words,), i32(fill), dtype=torch.int32, device=device).view(torch.uint8)
    at = GUARD_BYTES + (-(base.data_ptr() + GUARD_BYTES)) % WS_ALIGN
    view = base[at: at + int(nbytes)]
    assert ptr(view) % WS_ALIGN == 0 and view.numel() == nbytes
    return base, view


def assert_byte_guards(base, view, fill):
    """every byte of `base` outside `view` still holds its byte of the fill word"""
    at = ptr(view) - ptr(base)
    behind = at + view.numel()
    assert at >= GUARD_BYTES and base.numel() - behind >= GUARD_BYTES
    for lo, hi, where in ((0, at, "in front of"), (behind, base.numel(), "behind")):
        bad = torch.nonzero(base[lo:hi] != _pattern(fill, lo, hi - lo, base.device))
        assert bad.numel() == 0, (f"{bad.numel()} guard bytes {where} the workspace overwritten, the first at byte "
                                  f"{int(bad[0]) + lo - (at if lo == 0 else behind)} from that edge")


GUARD_U64 = GUARD_BYTES // 8


def guarded_u64(words, fill, device="cuda"):
    """-> (base, view): `words` device uint64 words (int64 storage, 8-byte aligned), GUARD_BYTES of the fill word on
    each side; the view itself starts out holding the fill too"""
    base = torch.full((2 * GUARD_U64 + int(words),), i64(fill), dtype=torch.int64, device=device)
    view = base[GUARD_U64: GUARD_U64 + int(words)]
    assert ptr(view) % 8 == 0
    return base, view


def assert_u64_guards(base, view, fill):
    """every word of `base` outside `view` still holds the fill"""
    at = (ptr(view) - ptr(base)) // 8
    assert at >= GUARD_U64 and base.numel() - at - view.numel() >= GUARD_U64
    for part, where in ((base[:at], "in front of"), (base[at + view.numel():], "behind")):
        bad = torch.nonzero(part != i64(fill))
        assert bad.numel() == 0, f"{bad.numel()} guard words {where} the uint64 result overwritten"


class Frozen:
    """a device clone of an input column, taken now; assert_unchanged() compares all of it"""

    def __init__(self, tensor):
        self.tensor, self.copy = tensor, tensor.clone()

    def assert_unchanged(self):
        bad = torch.nonzero(self.tensor != self.copy)
        assert bad.numel() == 0, f"{bad.numel()} words of an input column changed, the first at {int(bad[0])}"


class Watch:
    """the buffers of one call: hands out guarded buffers filled with one fill word, freezes inputs, and check() looks at
    every guard and every frozen input"""

    def __init__(self, fill, device="cuda"):
        self.fill, self.device = fill, device
        self._cols, self._bytes, self._u64, self._frozen = [], [], [], []

    def col(self, n, offset_words=0, data=None, freeze=False):
        """an int32 column of n words, offset_words past a 16-byte boundary (join_testlib.guarded); data: a host
        array (any 4-byte dtype) or a tensor copied into it; freeze: an input, compared by check()"""
        # join_testlib.guarded leaves 16 guard words on each side; COL_GUARD_WORDS more of the same allocation (a multiple
        # of 4: the offset from the 16-byte boundary stays) see a whole stray wave row of 16-byte vectors too
        base, outer = jt.guarded(int(n) + 2 * COL_GUARD_WORDS, offset_words, i32(self.fill), device=self.device)
        view = outer[COL_GUARD_WORDS: COL_GUARD_WORDS + int(n)]
        assert ptr(view) % 16 == 4 * (offset_words % 4)  # (ptr: torch gives an empty view, n = 0, no data_ptr)
        self._cols.append((base, view))
        if data is not None:
            if not torch.is_tensor(data):
                data = torch.from_numpy(np.ascontiguousarray(data).view(np.int32))
            view.copy_(data)
        if freeze:
            self._frozen.append(Frozen(view))
        return view

    def ws(self, nbytes):
        base, view = guarded_bytes(nbytes, self.fill, device=self.device)
        self._bytes.append((base, view))
        return view

    def u64(self, words):
        base, view = guarded_u64(words, self.fill, device=self.device)
        self._u64.append((base, view))
        return view

    def freeze(self, tensor):
        self._frozen.append(Frozen(tensor))

    def check(self):
        for base, view in self._cols:
            if view.numel():
                jt.assert_guards(base, view, i32(self.fill))
            else:  # an empty column (n = 0): all of the allocation is guard
                assert bool((base == i32(self.fill)).all()), "guard words around an empty column overwritten"
        for base, view in self._bytes:
            assert_byte_guards(base, view, self.fill)
        for base, view in self._u64:
            assert_u64_guards(base, view, self.fill)
        for f in self._frozen:
            f.assert_unchanged()
