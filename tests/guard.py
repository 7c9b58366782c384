"""Guard bands for kernel tests: strided, offset views inside buffers whose every other word holds a known bit pattern.

A plain module (no fixtures, no pytest settings) that works on CPU and device tensors alike.

    embed(t, ...)      a dense operand copied into the middle of a larger buffer: row stride ld >= C, a column offset, spare
                       elements in front and behind, everything outside the view = `fill` (a quiet NaN for float inputs,
                       0x7fffffff for int32 index inputs);
    guarded(shape,...) an output view inside a buffer in which EVERY 32-bit word, the view's own included, holds SENTINEL;
    workspace(nbytes)  a guarded region of exactly the size a ptt_*_workspace query returned, 16-byte aligned;
    check_guard(view)  every word outside the view's own elements still holds its fill, and (all_written) no element inside
                       still holds the sentinel — compared as int32 bit patterns, never as floats: +0.0 == -0.0 and NaN != NaN
                       would both let a stray write through;
    launch(name, ...)  the C ABI directly, for entry points whose wrapper in ops.py allocates its own outputs.

What this proves and what it does not: a WRITE outside an output or workspace changes a guard word and is caught wherever it
lands inside the buffer (the lead, the tail, the ld - C gap of every row). A READ outside an input is caught only if it reaches
the result — NaN surroundings turn a leak (a staged row too many, multiplied by a zero weight: NaN * 0 = NaN) into a wrong
value; a stray load whose value is discarded goes unseen.
"""
import struct

import torch

SENTINEL = 0x7fc0beef                   # int32; a quiet NaN read as float32, an impossible index / arg-max otherwise
INDEX_FILL = 0x7fffffff                 # around int32 index inputs: an index no cloud has
SENTINEL_F32 = struct.unpack("<f", struct.pack("<i", SENTINEL))[0]
_F64_NAN_WORDS = (0, 0x7ff80000)        # little-endian words of the float64 quiet NaN
_WORDS = {torch.float32: 1, torch.int32: 1, torch.float64: 2, torch.int64: 2}
LEAD = TAIL = 64                        # spare elements in front / behind by default (a multiple of 4: alignment kept)


class _Info(object):
    """Where a view lies inside its buffer (all in ELEMENTS of the view's dtype) and what surrounds it."""

    def __init__(self, words, wpe, shape3, ld, col_off, lead, tail, bstride, fill_words, ndim):
        self.words, self.wpe, self.shape3, self.ld, self.col_off = words, wpe, shape3, ld, col_off
        self.lead, self.tail, self.bstride, self.fill_words, self.ndim = lead, tail, bstride, fill_words, ndim

    @property
    def span(self):
        B, R, _ = self.shape3
        return (B - 1) * self.bstride + R * self.ld


def rows_aligned(view):
    """True when every row of the view starts on a 16-byte boundary (what the float4 forms of the kernels need)."""
    item = view.element_size()
    return view.data_ptr() % 16 == 0 and all((s * item) % 16 == 0 for s in view.stride()[:-1])


def _shape3(shape):
    shape = tuple(int(s) for s in shape)
    if len(shape) == 1:
        return (1, 1, shape[0])
    if len(shape) == 2:
        return (1,) + shape
    if len(shape) == 3:
        return shape
    raise ValueError("1-D, 2-D or 3-D shapes only, got %s" % (shape,))


def _fill_buffer(words, wpe, fill_words):
    for k in range(wpe):
        words[k::wpe] = fill_words[k]


def _make(shape, dtype, device, ld, col_off, lead, tail, batch_stride, fill_words, aligned, is_output):
    wpe = _WORDS[dtype]
    B, R, C = s3 = _shape3(shape)
    ld = C if ld is None else int(ld)
    if col_off < 0 or col_off + C > ld:
        raise ValueError("col_off=%d + C=%d does not fit ld=%d" % (col_off, C, ld))
    bstride = R * ld if batch_stride is None else int(batch_stride)
    if bstride < R * ld:
        raise ValueError("batch_stride=%d < rows * ld=%d" % (bstride, R * ld))
    n = lead + (B - 1) * bstride + R * ld + tail
    words = torch.empty((n * wpe,), dtype=torch.int32, device=device)
    assert words.data_ptr() % 16 == 0, "the allocator returned a buffer that is not 16-byte aligned"
    _fill_buffer(words, wpe, fill_words)
    elems = words.view(dtype)
    view = elems.as_strided((B, R, C), (bstride, ld, 1), lead + col_off)
    if len(shape) == 2:
        view = view[0]
    elif len(shape) == 1:
        view = view[0, 0]
    view._guard = _Info(words, wpe, s3, ld, col_off, lead, tail, bstride, fill_words, len(shape))
    view._guard.is_output = is_output
    per16 = 16 // (4 * wpe)
    want = (lead + col_off) % per16 == 0 and (R == 1 or ld % per16 == 0) and (B == 1 or bstride % per16 == 0)
    if aligned is not None and bool(aligned) != want:
        raise ValueError("aligned=%s cannot be had with lead=%d col_off=%d ld=%d batch_stride=%d" % (aligned, lead, col_off, ld, bstride))
    # the alignment that was asked for is the alignment the device sees
    got = view.data_ptr() % 16 == 0 and (R == 1 or (ld * 4 * wpe) % 16 == 0) and (B == 1 or (bstride * 4 * wpe) % 16 == 0)
    assert got == want, "asked for %s rows, data_ptr() %% 16 = %d" % ("aligned" if want else "unaligned", view.data_ptr() % 16)
    return view


def _default_fill(dtype):
    if dtype == torch.float32:
        return (SENTINEL,)
    if dtype == torch.float64:
        return _F64_NAN_WORDS
    if dtype == torch.int32:
        return (INDEX_FILL,)
    return (INDEX_FILL, INDEX_FILL)


def embed(t, ld=None, col_off=0, lead=LEAD, tail=TAIL, fill=None, batch_stride=None, aligned=None):
    """The dense 1-, 2- or 3-D tensor `t` copied into the middle of a larger flat buffer -> the view of it: row stride ld >= C,
    column offset col_off inside the row, `lead` / `tail` spare elements in front and behind, batch stride >= rows * ld.
    Everything outside the view holds `fill`, given as the int32 bit pattern of every 32-bit word (default: a quiet NaN for
    float tensors, INDEX_FILL for integer ones). col_off % 4 == 0 with ld % 4 == 0 keeps float32 rows 16-byte aligned,
    col_off = 1 or an odd ld does not; `aligned` (optional) states which one the caller means, and the helper asserts from
    data_ptr() % 16 that the view has the alignment its layout implies."""
    if not t.is_contiguous():
        raise ValueError("embed() takes a dense tensor")
    fill_words = _default_fill(t.dtype) if fill is None else (int(fill),) * _WORDS[t.dtype]
    view = _make(tuple(t.shape), t.dtype, t.device, ld, col_off, lead, tail, batch_stride, fill_words, aligned, False)
    view.copy_(t)
    return view


def guarded(shape, dtype, ld=None, col_off=0, lead=LEAD, tail=TAIL, device="cpu", batch_stride=None, aligned=None):
    """An output view of `shape` inside a buffer in which every 32-bit word — inside the view too — holds SENTINEL (both halves
    of a 64-bit element)."""
    return _make(shape, dtype, device, ld, col_off, lead, tail, batch_stride, (SENTINEL,) * _WORDS[dtype], aligned, True)


def workspace(nbytes, device="cpu", lead=LEAD, tail=TAIL):
    """A guarded region of exactly `nbytes` bytes (what a ptt_*_workspace query returned; a multiple of 4), 16-byte aligned:
    an int32 view; pass data_ptr() and nbytes to the launch, then check_guard(ws, all_written=False). A query that returned 0
    gets a view that owns no word: any write through its pointer is a guard violation."""
    nbytes = int(nbytes)
    if nbytes % 4:
        raise ValueError("workspace sizes are whole 32-bit words, got %d bytes" % nbytes)
    return guarded((nbytes // 4,), torch.int32, lead=lead, tail=tail, device=device, aligned=True)


class GuardError(AssertionError):
    pass


def _owned_word_index(info, device):
    B, R, C = info.shape3
    ar = lambda n: torch.arange(n, dtype=torch.int64, device=device)
    e = (info.lead + info.col_off + ar(B).view(B, 1, 1) * info.bstride + ar(R).view(1, R, 1) * info.ld + ar(C).view(1, 1, C))
    return (e.reshape(-1, 1) * info.wpe + ar(info.wpe).view(1, -1)).reshape(-1)


def _place(info, e):
    """Element offset e inside the buffer -> a description of where that is relative to the view."""
    B, R, C = info.shape3
    if e < info.lead:
        return "before the rows (%d elements in front of the view's first row)" % (info.lead - e)
    rel = e - info.lead
    if rel >= info.span:
        return "behind the rows (%d elements past the end of the last row)" % (rel - info.span)
    b, in_b = divmod(rel, info.bstride)
    r, c = divmod(in_b, info.ld)
    if r >= R:
        return "between the rows (batch %d, %d elements past its last row)" % (b, in_b - R * info.ld)
    where = "(row %d, column %d)" % (r, c - info.col_off) if B == 1 else "(batch %d, row %d, column %d)" % (b, r, c - info.col_off)
    return "between the rows %s" % where


def _info(view):
    info = getattr(view, "_guard", None)
    if info is None:
        raise TypeError("a view made by embed(), guarded() or workspace() is expected — the ORIGINAL one: a slice, reshape or copy "
                        "of it does not carry the buffer's bookkeeping")
    return info


def _changed(info):
    """-> (own, bad): the word indices the view owns, and per word of the buffer whether it no longer holds its fill."""
    own = _owned_word_index(info, info.words.device)
    expect = torch.empty_like(info.words)
    _fill_buffer(expect, info.wpe, info.fill_words)
    return own, info.words != expect


def check_guard(view, all_written=True):
    """Raises GuardError unless every word of the buffer outside the view's own elements still holds its fill — the lead, the
    tail and the ld - C gap of every row — and, with all_written, no element inside the view still holds the sentinel. Bit
    patterns are compared as int32. The message names the first offending place. `view` is the tensor embed() / guarded() /
    workspace() returned, not a slice or reshape of it (the bookkeeping is an attribute of that tensor object)."""
    info = _info(view)
    words, wpe = info.words, info.wpe
    own, bad = _changed(info)
    bad[own] = False
    if bool(bad.any()):
        w = int(torch.nonzero(bad)[0, 0])
        raise GuardError("guard word changed %s: 0x%08x instead of 0x%08x" % (_place(info, w // wpe), int(words[w]) & 0xffffffff,
                                                                              info.fill_words[w % wpe] & 0xffffffff))
    if all_written:
        still = (words[own] == SENTINEL).view(-1, wpe).all(dim=1)
        if bool(still.any()):
            k = int(torch.nonzero(still)[0, 0])
            B, R, C = info.shape3
            b, rc = divmod(k, R * C)
            r, c = divmod(rc, C)
            raise GuardError("element (%s%d, %d) inside the view still holds the sentinel: never written" % ("%d, " % b if B > 1 else "", r, c))


def assert_untouched(*views):
    """Every word of each view's buffer — inside the view too — still holds its fill: what a refused launch must leave behind."""
    for v in views:
        info = _info(v)
        own, bad = _changed(info)
        inside = torch.zeros_like(bad)
        inside[own] = True
        if not info.is_output:                                          # an embed()-ded input: its own elements are data
            bad &= ~inside
        if bool(bad.any()):
            w = int(torch.nonzero(bad)[0, 0])
            raise GuardError("a word was written %s" % ("inside the view" if bool(inside[w]) else _place(info, w // info.wpe)))


def launch(name, device, *args):
    """Pass-through to ptt_amd.ops._launch: the entry point `name` of the C ABI on the current stream; a non-zero status
    raises RuntimeError."""
    from ptt_amd import ops
    return ops._launch(name, device, *args)


def ptr(t):
    """A tensor's device pointer as the C ABI takes it (None -> NULL)."""
    import ctypes
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
