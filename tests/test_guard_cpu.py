"""Mutation tests of tests/guard.py on CPU tensors: what a stray kernel write would do to a guarded buffer is done here by
hand, one word at a time, and check_guard must fail and name the place. This is the proof that a GPU test built on the
helper fails when a kernel strays; no faulty kernel is planted on the device for it."""
import pytest
import torch

from tests import guard

DTYPES = [torch.float32, torch.int32, torch.float64]
R, C, LD, OFF = 5, 6, 12, 4


def _view(dtype):
    return guard.guarded((R, C), dtype, ld=LD, col_off=OFF, lead=8, tail=8)


def _write_all(v):
    v.copy_(torch.arange(R * C, dtype=torch.float64).view(R, C).to(v.dtype))


def _elem_word(v, e, half=0):
    """Index into the buffer's int32 words of element offset e (in the view's dtype) of the flat buffer."""
    return e * v._guard.wpe + half


@pytest.mark.parametrize("dtype", DTYPES)
def test_untouched_buffer_passes(dtype):
    v = _view(dtype)
    guard.check_guard(v, all_written=False)
    _write_all(v)
    guard.check_guard(v)
    assert int((v._guard.words == guard.SENTINEL).sum()) == v._guard.words.numel() - R * C * v._guard.wpe


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where,elem,expect", [
    ("lead", 3, "before the rows (5 elements"),
    ("gap left of a middle row", 8 + 2 * LD + 1, "between the rows (row 2, column -3)"),
    ("gap right of a middle row", 8 + 2 * LD + OFF + C, "between the rows (row 2, column %d)" % C),
    ("gap of the last row", 8 + (R - 1) * LD + LD - 1, "between the rows (row %d, column %d)" % (R - 1, LD - 1 - OFF)),
    ("tail", 8 + R * LD + 2, "behind the rows (2 elements"),
])
def test_one_changed_word_is_found_and_named(dtype, where, elem, expect):
    for half in range(guard._WORDS[dtype]):
        v = _view(dtype)
        _write_all(v)
        v._guard.words[_elem_word(v, elem, half)] = 1
        with pytest.raises(guard.GuardError) as ei:
            guard.check_guard(v)
        assert expect in str(ei.value), (where, str(ei.value))


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_unwritten_element_fails_under_all_written(dtype):
    v = _view(dtype)
    _write_all(v)
    wpe = v._guard.wpe
    e = 8 + 3 * LD + OFF + 2
    v._guard.words[e * wpe:(e + 1) * wpe] = guard.SENTINEL
    guard.check_guard(v, all_written=False)
    with pytest.raises(guard.GuardError) as ei:
        guard.check_guard(v)
    assert "(3, 2)" in str(ei.value) and "never written" in str(ei.value)


@pytest.mark.parametrize("value", [0.0, -0.0, float("nan"), float(guard.SENTINEL)])
def test_float_writes_that_a_float_comparison_would_miss(value):
    """A gap word overwritten with +0.0 / -0.0, with the canonical NaN (NaN != NaN, so `x != x` style checks see "still a
    NaN") or with the float whose VALUE is the sentinel's integer: none has the sentinel's bits, each must fail."""
    v = _view(torch.float32)
    _write_all(v)
    flat = v._guard.words.view(torch.float32)
    flat[8 + LD + 1] = value
    with pytest.raises(guard.GuardError) as ei:
        guard.check_guard(v)
    assert "between the rows (row 1, column -3)" in str(ei.value)


def test_sentinel_is_a_nan_as_float_and_no_index():
    assert guard.SENTINEL_F32 != guard.SENTINEL_F32                                  # NaN
    v = guard.guarded((2, 3), torch.float32, ld=4)
    assert bool(torch.isnan(v).all())
    assert guard.SENTINEL > 1 << 30 and guard.INDEX_FILL == 2 ** 31 - 1
    d = guard.guarded((2, 3), torch.float64, ld=4)
    assert bool((d._guard.words == guard.SENTINEL).all())                            # both halves


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ld,col_off,aligned", [(None, 0, None), (12, 4, True), (12, 1, False), (11, 0, False), (13, 4, False)])
def test_embed_round_trips_and_aligns(dtype, ld, col_off, aligned):
    t = (torch.arange(3 * 7, dtype=torch.float64).view(3, 7) - 5).to(dtype)
    if ld is None:
        aligned = False                                         # 7 elements a row: neither 28-byte nor 56-byte rows are aligned
    v = guard.embed(t, ld=ld, col_off=col_off, aligned=aligned)
    assert v.shape == t.shape and v.stride() == ((ld or 7), 1)
    assert torch.equal(v, t)
    assert guard.rows_aligned(v) == bool(aligned)
    assert (v.data_ptr() % 16 == 0) == (col_off % (16 // t.element_size()) == 0)
    guard.check_guard(v, all_written=False)
    words = v._guard.words
    n_fill = words.numel() - t.numel() * v._guard.wpe
    if dtype == torch.float32:
        assert int(torch.isnan(words.view(torch.float32)).sum()) == n_fill           # NaN everywhere around
    elif dtype == torch.float64:
        assert int(torch.isnan(words.view(torch.float64)).sum()) == n_fill // 2
    else:
        assert int((words == guard.INDEX_FILL).sum()) == n_fill
    # and a changed surrounding of an INPUT is seen as well (a kernel that writes through a const pointer)
    words[0] = 7
    with pytest.raises(guard.GuardError):
        guard.check_guard(v, all_written=False)


def test_embed_refuses_an_alignment_it_cannot_give():
    t = torch.zeros((3, 8))
    with pytest.raises(ValueError):
        guard.embed(t, ld=12, col_off=1, aligned=True)
    with pytest.raises(ValueError):
        guard.embed(t, ld=12, col_off=4, aligned=False)
    with pytest.raises(ValueError):
        guard.embed(t, ld=9, col_off=4)                         # 4 + 8 > 9


def test_embed_3d_batch_stride():
    t = torch.arange(2 * 3 * 4, dtype=torch.float32).view(2, 3, 4)
    v = guard.embed(t, ld=8, col_off=4, batch_stride=3 * 8 + 5, aligned=False)
    assert v.stride() == (29, 8, 1) and torch.equal(v, t)
    v._guard.words[guard.LEAD + 3 * 8 + 2] = 0                  # between the two batches
    with pytest.raises(guard.GuardError) as ei:
        guard.check_guard(v, all_written=False)
    assert "between the rows (batch 0, 2 elements past its last row)" in str(ei.value)


def test_workspace_is_exact_and_aligned():
    ws = guard.workspace(40)
    assert ws.numel() * 4 == 40 and ws.data_ptr() % 16 == 0
    guard.check_guard(ws, all_written=False)
    ws._guard.words[guard.LEAD + 10] = 0                        # the first word behind the 40 bytes
    with pytest.raises(guard.GuardError) as ei:
        guard.check_guard(ws, all_written=False)
    assert "behind the rows (0 elements" in str(ei.value)
    with pytest.raises(ValueError):
        guard.workspace(6)
    empty = guard.workspace(0)                                  # a zero-byte query owns no word at all
    assert empty.numel() == 0 and empty.data_ptr() % 16 == 0
    guard.check_guard(empty)
    empty._guard.words[guard.LEAD] = 0                          # where its first word would be
    with pytest.raises(guard.GuardError):
        guard.check_guard(empty)
    with pytest.raises(TypeError, match="ORIGINAL"):
        guard.check_guard(ws[2:])                               # a slice does not carry the bookkeeping


@pytest.mark.parametrize("dtype", DTYPES)
def test_assert_untouched_sees_a_write_inside_the_view_too(dtype):
    """What a refused launch must leave behind: not one word written, the output's own elements included."""
    v = _view(dtype)
    guard.assert_untouched(v)
    v[2, 3] = 1
    guard.check_guard(v, all_written=False)                     # a write inside the view is no guard violation ...
    with pytest.raises(guard.GuardError, match="inside the view"):
        guard.assert_untouched(v)                               # ... but it is a launch
    t = guard.embed(torch.ones((3, 4), dtype=dtype), ld=6, col_off=1)
    guard.assert_untouched(t)                                   # an input's own elements are data
    t._guard.words[0] = 5
    with pytest.raises(guard.GuardError, match="before the rows"):
        guard.assert_untouched(t)
