"""Two tokenizations of a batch compared word by word on the device (include/dpt.h dpt_word_compare_sizes,
dpt_word_compare_write): which words have fewer (or more) tokens on side a than on side b, and where their tokens lie.

A side is what the producing calls leave on the device: ``tok_word`` (and ``tok_end``) of ``dpt_token_spans`` next to
the CSR ``id_off`` of ``dpt_encode``, or ``tok_word`` of ``dpt_bpe_encode`` next to its string offsets and ``counts``.
``compare_device`` makes the two calls on torch's current stream; ``selected_ids`` gathers the ids of the selected
words of one side."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

from . import _lib
from ._lib import WORDS_GREATER, WORDS_LESS, DptError, WordSide, check

__all__ = ["WORDS_LESS", "WORDS_GREATER", "Side", "WordCompare", "sizes_device", "write_device", "compare_device", "selected_ids"]


class Side(NamedTuple):
    """One tokenization by word, torch device tensors: ``off`` int64[n_str + 1], ``tok_word`` int32 (uint32 bits), and
    optionally ``counts`` int64[n_str] (given: ``off`` are string offsets, the padded layout), ``status`` int32[n_str]
    and ``tok_end`` int32 -- side a's gives the selected words' byte spans."""
    off: object
    tok_word: object
    counts: Optional[object] = None
    status: Optional[object] = None
    tok_end: Optional[object] = None


class WordCompare(NamedTuple):
    """``compare_device``'s result, all device tensors.  Per string: ``status`` (0, a side's status, or 4 for streams
    that are not two numberings of the same words), ``n_words``, ``n_sel``, ``len_a``, ``len_b``, and the prefix sums
    ``word_off`` / ``sel_off`` (int64[n_str + 1]).  Per word at ``word_off[s] + w``: ``cnt_a``, ``cnt_b``.  Per selected
    word at ``sel_off[s] + d``, ascending: ``sel_str``, ``sel_word``, the token ranges ``sel_a_first`` / ``sel_a_count`` /
    ``sel_b_first`` / ``sel_b_count`` within the string, and ``sel_begin`` / ``sel_end``, the word's bytes (None when
    side a came without ``tok_end``)."""
    status: object
    n_words: object
    n_sel: object
    len_a: object
    len_b: object
    word_off: object
    sel_off: object
    cnt_a: object
    cnt_b: object
    sel_str: object
    sel_word: object
    sel_begin: Optional[object]
    sel_end: Optional[object]
    sel_a_first: object
    sel_a_count: object
    sel_b_first: object
    sel_b_count: object


def _side(ptrs) -> WordSide:
    """``(off, counts, status, tok_word, tok_end)`` device addresses (0 = NULL) as a dpt_word_side."""
    return WordSide(*(int(x) or None for x in ptrs))


def _need():
    if not _lib.has_words():
        raise DptError(f"{_lib.LIB_PATH} was built before the word-compare calls (no dpt_word_compare_sizes): rebuild it")


def sizes_device(a, b, n_str: int, flags: int, n_words_ptr: int, n_sel_ptr: int, wc_status_ptr: int, len_a_ptr: int = 0,
                 len_b_ptr: int = 0, stream: int = 0) -> None:
    """dpt_word_compare_sizes over device addresses (0 = NULL): stream-ordered, no sync.  ``a`` / ``b``: each side as
    ``(off_ptr, counts_ptr, status_ptr, tok_word_ptr, tok_end_ptr)``."""
    _need()
    sa, sb = _side(a), _side(b)
    check(_lib.lib().dpt_word_compare_sizes(ctypes.byref(sa), ctypes.byref(sb), n_str, flags, n_words_ptr, n_sel_ptr, len_a_ptr,
                                            len_b_ptr, wc_status_ptr, stream), "dpt_word_compare_sizes")


def write_device(a, b, n_str: int, flags: int, wc_status_ptr: int, *, word_off_ptr: int = 0, cnt_a_ptr: int = 0, cnt_b_ptr: int = 0,
                 sel_off_ptr: int = 0, sel_str_ptr: int = 0, sel_word_ptr: int = 0, sel_begin_ptr: int = 0, sel_end_ptr: int = 0,
                 sel_a_first_ptr: int = 0, sel_a_count_ptr: int = 0, sel_b_first_ptr: int = 0, sel_b_count_ptr: int = 0,
                 stream: int = 0) -> None:
    """dpt_word_compare_write over device addresses (0 = NULL): stream-ordered, no sync.  Sides as ``sizes_device``'s;
    ``word_off`` / ``sel_off`` are the prefix sums of the sizes pass's ``n_words`` / ``n_sel`` (uint64[n_str + 1])."""
    _need()
    sa, sb = _side(a), _side(b)
    check(_lib.lib().dpt_word_compare_write(ctypes.byref(sa), ctypes.byref(sb), n_str, flags, word_off_ptr, cnt_a_ptr, cnt_b_ptr,
                                            sel_off_ptr, sel_str_ptr, sel_word_ptr, sel_begin_ptr, sel_end_ptr, sel_a_first_ptr,
                                            sel_a_count_ptr, sel_b_first_ptr, sel_b_count_ptr, wc_status_ptr, stream),
          "dpt_word_compare_write")


def _check_side(torch, side, name: str) -> Side:
    side = Side(*side)
    for field, dtype in (("off", torch.int64), ("tok_word", torch.int32), ("counts", torch.int64), ("status", torch.int32),
                         ("tok_end", torch.int32)):
        t = getattr(side, field)
        if t is None and field in ("counts", "status", "tok_end"):
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"side {name}: {field} must be a contiguous {dtype} device tensor")
    n = side.off.numel() - 1
    if n < 0 or any(t is not None and t.numel() != n for t in (side.counts, side.status)):
        raise ValueError(f"side {name}: off needs n_str + 1 entries, counts and status n_str")
    return side


def _ptrs(torch, side: Side, anchor):
    """The side's addresses; an empty tok_word / tok_end (a batch without tokens) still gives an address."""
    def ptr(t):
        return 0 if t is None else t.data_ptr() if t.numel() else anchor.data_ptr()
    return ptr(side.off), ptr(side.counts), ptr(side.status), ptr(side.tok_word), ptr(side.tok_end)


def compare_device(side_a, side_b, flags: int = WORDS_LESS) -> WordCompare:
    """``side_a`` against ``side_b`` (each a ``Side`` or a tuple in its field order) on torch's current stream: the sizes
    pass, one ``torch.cumsum`` pair, the write pass.  The two totals that size the outputs are the only host reads."""
    import torch
    a, b = _check_side(torch, side_a, "a"), _check_side(torch, side_b, "b")
    n = a.off.numel() - 1
    if b.off.numel() - 1 != n:
        raise ValueError("both off tensors need the same n_str + 1 entries")
    dev = a.off.device
    if any(t is not None and t.device != dev for t in tuple(a) + tuple(b)):
        raise ValueError("both sides must be on one device")
    if flags not in (WORDS_LESS, WORDS_GREATER, WORDS_LESS | WORDS_GREATER):
        raise ValueError("flags: WORDS_LESS and / or WORDS_GREATER")
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        per_str = torch.zeros((5, max(n, 1)), dtype=torch.int32, device=dev)   # n_words, n_sel, len_a, len_b, status
        offs = torch.zeros((2, n + 1), dtype=torch.int64, device=dev)          # word_off, sel_off
        pa, pb = _ptrs(torch, a, per_str), _ptrs(torch, b, per_str)
        if n > 0:
            sizes_device(pa, pb, n, flags, per_str[0].data_ptr(), per_str[1].data_ptr(), per_str[4].data_ptr(),
                         len_a_ptr=per_str[2].data_ptr(), len_b_ptr=per_str[3].data_ptr(), stream=stream)
            torch.cumsum(per_str[:2, :n], dim=1, out=offs[:, 1:])
        n_words, n_sel = (int(x) for x in offs[:, -1].tolist())
        per_word = torch.empty((2, max(n_words, 1)), dtype=torch.int32, device=dev)
        want_spans = a.tok_end is not None
        per_sel = torch.empty((8, max(n_sel, 1)), dtype=torch.int32, device=dev)
        if n > 0:
            sel = [per_sel[k].data_ptr() for k in range(8)]
            write_device(pa, pb, n, flags, per_str[4].data_ptr(), word_off_ptr=offs[0].data_ptr(), cnt_a_ptr=per_word[0].data_ptr(),
                         cnt_b_ptr=per_word[1].data_ptr(), sel_off_ptr=offs[1].data_ptr(), sel_str_ptr=sel[0], sel_word_ptr=sel[1],
                         sel_begin_ptr=sel[2] if want_spans else 0, sel_end_ptr=sel[3] if want_spans else 0, sel_a_first_ptr=sel[4],
                         sel_a_count_ptr=sel[5], sel_b_first_ptr=sel[6], sel_b_count_ptr=sel[7], stream=stream)
    s = per_sel[:, :n_sel]
    return WordCompare(per_str[4, :n], per_str[0, :n], per_str[1, :n], per_str[2, :n], per_str[3, :n], offs[0], offs[1],
                       per_word[0, :n_words], per_word[1, :n_words], s[0], s[1], s[2] if want_spans else None,
                       s[3] if want_spans else None, s[4], s[5], s[6], s[7])


def selected_ids(ids, off, counts, sel_str, sel_first, sel_count):
    """The ids of the selected words of one side, gathered on the device: ``ids`` int32 with string s's at
    ``off[s] - off[0]`` (``counts``, the padded layout's, is not needed to find them and may be None), the records
    ``sel_str`` / ``sel_first`` / ``sel_count`` of that side -> (flat int32 ids, int64 offsets[n_sel + 1]): word d's ids
    are ``flat[offsets[d]:offsets[d + 1]]``.  One host read, the total."""
    import torch
    n_sel, dev = sel_str.numel(), ids.device
    out_off = torch.zeros(n_sel + 1, dtype=torch.int64, device=dev)
    if n_sel == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), out_off
    torch.cumsum(sel_count.to(torch.int64), dim=0, out=out_off[1:])
    total = int(out_off[-1])
    start = off[sel_str.to(torch.int64)] - off[0] + sel_first.to(torch.int64)
    at = torch.repeat_interleave(start - out_off[:-1], sel_count.to(torch.int64), output_size=total)
    return ids[at + torch.arange(total, dtype=torch.int64, device=dev)], out_off
