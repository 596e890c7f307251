"""tests/guard_testlib.py on the host: every helper accepts an untouched buffer and raises when one guard byte directly
in front of the view, one directly behind it, or one word of a frozen input is edited (with torch, on the CPU)."""
import pytest
import torch

from tests import guard_testlib as gt
from tests import join_testlib as jt


def test_the_fill_words_as_torch_wants_them():
    assert gt.FILLS == (0x5A5A5A5A, 0xA5A5A5A5)
    assert gt.i32(0x5A5A5A5A) == 0x5A5A5A5A and gt.i32(0xA5A5A5A5) == 0xA5A5A5A5 - (1 << 32) < 0
    for fill in gt.FILLS:
        assert torch.tensor([gt.i64(fill)], dtype=torch.int64).view(torch.int32).tolist() == [gt.i32(fill)] * 2


@pytest.mark.parametrize("fill", gt.FILLS)
@pytest.mark.parametrize("nbytes", [0, 1, 5, 256, 768, 4099, 100001])
def test_guarded_bytes_end_where_they_say(nbytes, fill):
    base, view = gt.guarded_bytes(nbytes, fill, device="cpu")
    at = gt.ptr(view) - gt.ptr(base)
    assert view.dtype == torch.uint8 and view.numel() == nbytes and gt.ptr(view) % 256 == 0
    assert at >= 4096 and base.numel() - at - nbytes >= 4096
    gt.assert_byte_guards(base, view, fill)
    view.fill_(0x33)  # the view is the caller's, all of it
    gt.assert_byte_guards(base, view, fill)
    for edit in (at - 1, at + nbytes, 0, base.numel() - 1):  # directly in front, directly behind, the far ends
        was = int(base[edit])
        base[edit] = was ^ 0x01
        with pytest.raises(AssertionError):
            gt.assert_byte_guards(base, view, fill)
        base[edit] = was
    gt.assert_byte_guards(base, view, fill)
    assert bool((view == 0x33).all())


@pytest.mark.parametrize("fill", gt.FILLS)
@pytest.mark.parametrize("words", [0, 1, 2, 3, 1024])
def test_guarded_u64_words(words, fill):
    base, view = gt.guarded_u64(words, fill, device="cpu")
    at = (gt.ptr(view) - gt.ptr(base)) // 8
    assert view.dtype == torch.int64 and view.numel() == words and gt.ptr(view) % 8 == 0 and at * 8 >= 4096
    gt.assert_u64_guards(base, view, fill)
    view.zero_()
    gt.assert_u64_guards(base, view, fill)
    for edit in (at - 1, at + words):
        base[edit] ^= 1 << 40  # one byte of one guard word
        with pytest.raises(AssertionError):
            gt.assert_u64_guards(base, view, fill)
        base[edit] ^= 1 << 40
    gt.assert_u64_guards(base, view, fill)


def test_frozen_sees_one_changed_word():
    col = torch.arange(1000, dtype=torch.int32)
    frozen = gt.Frozen(col)
    frozen.assert_unchanged()
    for at in (0, 517, 999):
        col[at] += 1
        with pytest.raises(AssertionError):
            frozen.assert_unchanged()
        col[at] -= 1
    frozen.assert_unchanged()
    empty = gt.Frozen(col[:0])
    empty.assert_unchanged()


def test_an_empty_column_still_has_an_address_and_guards():
    w = gt.Watch(gt.FILLS[0], device="cpu")
    view = w.col(0, 2)
    base = w._cols[0][0]
    assert view.numel() == 0 and gt.ptr(view) == base.data_ptr() + 4 * (jt.GUARD_WORDS + gt.COL_GUARD_WORDS + 2)
    w.check()
    base[jt.GUARD_WORDS + gt.COL_GUARD_WORDS + 2] = 0
    with pytest.raises(AssertionError):
        w.check()


@pytest.mark.parametrize("fill", gt.FILLS)
def test_watch_checks_every_buffer_it_handed_out(fill):
    w = gt.Watch(fill, device="cpu")
    src = w.col(37, 3, data=torch.arange(37, dtype=torch.int32), freeze=True)
    out = w.col(37, 1)
    ws = w.ws(768)
    size = w.u64(1)
    assert src.data_ptr() % 16 == 12 and out.data_ptr() % 16 == 4 and src.tolist() == list(range(37))
    assert out.tolist() == [gt.i32(fill)] * 37  # an output starts out holding the fill
    w.check()
    out.fill_(1), ws.fill_(2), size.fill_(3)
    w.check()
    edits = []
    for view in (src, out):  # the int32 columns: join_testlib.guarded's bases
        base = next(b for b, v in w._cols if v is view)
        at = (view.data_ptr() - base.data_ptr()) // 4
        assert at == jt.GUARD_WORDS + gt.COL_GUARD_WORDS + (3 if view is src else 1)
        edits += [(base, at - 1), (base, at + 37), (base, 0), (base, base.numel() - 1)]
    base = w._bytes[0][0]
    at = ws.data_ptr() - base.data_ptr()
    edits += [(base, at - 1), (base, at + 768)]
    base = w._u64[0][0]
    edits += [(base, gt.GUARD_U64 - 1), (base, gt.GUARD_U64 + 1)]
    edits += [(src, 0), (src, 36)]  # a frozen input
    for tensor, at in edits:
        was = tensor[at].clone()
        tensor[at] = was ^ 1
        with pytest.raises(AssertionError):
            w.check()
        tensor[at] = was
    w.check()
