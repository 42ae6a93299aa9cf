"""Model-input batches on the device (dpt_collate, include/dpt.h): the ids of an encoded batch as padded
``input_ids`` / ``attention_mask`` / ``labels`` rows -- what the reference's ``llama_preprocessing_function``
(main_analyze_s2orc.py:61-93) and the Trainer's collator produce on the host.

``collate_device`` is the raw call over device addresses; ``model_inputs`` the same over torch tensors.

``collate_pair_device`` / ``pair_model_inputs`` are the two-segment form (dpt_collate_pair): each row is a source
followed by a target -- what the reference's translation driver builds with ``apply_tokenizer`` and
``ShortcutDataCollatorForSeq2Seq`` (main_biomed_translation.py:138-145, :104-124)."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

from . import _lib
from ._lib import (COLLATE_BOS, COLLATE_EOS, COLLATE_I64, COLLATE_MASK_A, COLLATE_PAD_LEFT, COLLATE_SEP, COLLATE_TRIM_A_FIRST,
                   COLLATE_TRUNC_LEFT, CollateOpts, CollatePairOpts, CollateSide, DptError, check)


def collate_flags(bos_id=None, eos_id=None, pad_left=False, trunc_left=False, int64=True) -> int:
    return ((COLLATE_BOS if bos_id is not None else 0) | (COLLATE_EOS if eos_id is not None else 0)
            | (COLLATE_PAD_LEFT if pad_left else 0) | (COLLATE_TRUNC_LEFT if trunc_left else 0)
            | (COLLATE_I64 if int64 else 0))


def collate_device(ids_ptr: int, off_ptr: int, n_str: int, input_ids_ptr: int, row_len: int, *, counts_ptr: int = 0,
                   status_ptr: int = 0, mask_ptr: int = 0, labels_ptr: int = 0, lengths_ptr: int = 0, row_stride: int = 0,
                   pad_id: int = 0, bos_id: Optional[int] = None, eos_id: Optional[int] = None, ignore_id: int = -100,
                   pad_left: bool = False, trunc_left: bool = False, int64: bool = True, stream: int = 0) -> None:
    """dpt_collate over device addresses (e.g. ``torch.Tensor.data_ptr()``; 0 = NULL): stream-ordered, no sync.
    ``counts_ptr`` 0: ``off`` is dpt_encode's id_off; else dpt_encode_padded's str_off and counts.  ``bos_id`` /
    ``eos_id`` None: no such special.  Rows are int64, or int32 with ``int64=False``; ``lengths`` is uint32."""
    if not _lib.has_collate():
        raise DptError("this libdpt.so has no dpt_collate")
    opts = CollateOpts(row_len, row_stride, pad_id, bos_id or 0, eos_id or 0, ignore_id,
                       collate_flags(bos_id, eos_id, pad_left, trunc_left, int64))
    check(_lib.lib().dpt_collate(ids_ptr, off_ptr, counts_ptr, status_ptr, n_str, ctypes.byref(opts), input_ids_ptr,
                                 mask_ptr, labels_ptr, lengths_ptr, stream), "dpt_collate")


def _check_padding(padding, padding_side, truncation_side):
    if padding not in ("longest", "max_length"):
        raise ValueError("padding must be 'longest' or 'max_length'")
    if padding_side not in ("left", "right") or truncation_side not in ("left", "right"):
        raise ValueError("padding_side / truncation_side must be 'left' or 'right'")


def _check_side(torch, side, name=""):
    """One source as (ids, off, status, counts) tensors, validated (``name``: the side, for the messages) -> the four
    and n_str (-1: ``off`` is empty, which the caller reports)."""
    ids, off, status, counts = (tuple(side) + (None, None))[:4]
    name = name and name + ": "
    for t in (ids, off, status, counts):
        if t is not None and (not t.is_contiguous() or t.device != ids.device):
            raise ValueError(name + "ids, off, status and counts must be contiguous tensors on one device")
    if ids.dtype != torch.int32 or off.element_size() != 8 or (counts is not None and counts.element_size() != 8) \
            or (status is not None and status.dtype != torch.int32):
        raise ValueError(name + "ids / status must be int32, off / counts 8-byte integers")
    n_str = off.numel() - 1
    if (status is not None and status.numel() < n_str) or (counts is not None and counts.numel() < n_str):
        raise ValueError("status / counts need n_str entries")
    return (ids, off, status, counts), n_str


def _row_len(torch, sides, caps, n_str, n_special, padding, max_length, pad_to_multiple_of):
    """The row length of both calls: ``max_length``, or (``padding="longest"``) the longest row's kept tokens -- each
    side's count under its cap (0: none), summed -- plus the specials, capped by ``max_length``; then at least
    max(the specials, 1) and rounded up to ``pad_to_multiple_of``.  A failed string's row is all pad: it adds nothing."""
    if padding == "max_length":
        if max_length is None:
            raise ValueError("padding='max_length' needs max_length")
        row_len = int(max_length)
    else:
        row_len = 0
        if n_str:
            total = 0
            for (_, off, status, counts), cap in zip(sides, caps):
                n = counts.view(torch.int64)[:n_str] if counts is not None else off.view(torch.int64).diff()
                if status is not None:
                    n = n.masked_fill(status[:n_str] != 0, -(1 << 40))
                total = total + (n.clamp(max=cap) if cap else n)
            row_len = max(int(total.max()), 0) + n_special
        if max_length is not None:
            row_len = min(row_len, int(max_length))
    row_len = max(row_len, n_special, 1)
    if pad_to_multiple_of:
        row_len = -(-row_len // pad_to_multiple_of) * pad_to_multiple_of
    return row_len


def _alloc(torch, rows, per_row, n_str, row_len, int64, dev):
    """the [n_str, row_len] tensors named in ``rows`` and the int32 per-string ones named in ``per_row``"""
    out = {k: torch.empty((n_str, row_len), dtype=torch.int64 if int64 else torch.int32, device=dev) for k in rows}
    out.update((k, torch.empty(n_str, dtype=torch.int32, device=dev)) for k in per_row)
    return out


def _side_ptrs(torch, side):
    """(ids, off, counts, status) device addresses of a validated side, 0 for None, and the tensor that keeps the ids'
    address alive"""
    ids, off, status, counts = side
    if ids.numel() == 0:   # (an empty tensor has no address; no id is read)
        ids = torch.zeros(1, dtype=torch.int32, device=off.device)
    return (ids.data_ptr(), off.data_ptr(), counts.data_ptr() if counts is not None else 0,
            status.data_ptr() if status is not None else 0), ids


def model_inputs(ids, off, status=None, counts=None, *, padding: str = "longest", max_length: Optional[int] = None,
                 pad_to_multiple_of: Optional[int] = None, labels: bool = False, pad_id: int = 0,
                 bos_id: Optional[int] = None, eos_id: Optional[int] = None, ignore_id: int = -100,
                 padding_side: str = "right", truncation_side: str = "right", int64: bool = True) -> Dict[str, object]:
    """Torch device tensors of an encoded batch -> ``{"input_ids", "attention_mask", "lengths"[, "labels"]}``,
    allocated on the inputs' device and filled on torch's current stream by one dpt_collate launch.

    ``ids`` int32, ``off`` (int64 / uint64 bit patterns, n_str + 1 entries), ``status`` int32 or None and
    ``counts`` or None are what ``Encoder.encode_device`` (off = id_off) or ``encode_device_padded``
    (off = str_off, counts) wrote.  ``padding="longest"``: the row length is the longest kept sequence, read
    back from the offsets or counts (that one scalar is the only synchronisation), capped by ``max_length``;
    ``"max_length"``: the row length is ``max_length`` and nothing synchronises.  Either is then rounded up to
    ``pad_to_multiple_of`` and is at least max(the specials, 1).  Rows are int64 (``int64=False``: int32),
    ``lengths`` int32 per string."""
    import torch
    _check_padding(padding, padding_side, truncation_side)
    side, n_str = _check_side(torch, (ids, off, status, counts))
    if n_str < 0:
        raise ValueError("off needs n_str + 1 entries")
    n_special = (bos_id is not None) + (eos_id is not None)
    row_len = _row_len(torch, [side], [0], n_str, n_special, padding, max_length, pad_to_multiple_of)
    dev = ids.device
    out = _alloc(torch, ["input_ids", "attention_mask"] + (["labels"] if labels else []), ["lengths"], n_str, row_len, int64, dev)
    if n_str == 0:
        return out
    (ids_ptr, off_ptr, counts_ptr, status_ptr), _keep = _side_ptrs(torch, side)
    with torch.cuda.device(dev):
        collate_device(ids_ptr, off_ptr, n_str, out["input_ids"].data_ptr(), row_len, counts_ptr=counts_ptr,
                       status_ptr=status_ptr, mask_ptr=out["attention_mask"].data_ptr(),
                       labels_ptr=out["labels"].data_ptr() if labels else 0, lengths_ptr=out["lengths"].data_ptr(),
                       pad_id=pad_id, bos_id=bos_id, eos_id=eos_id, ignore_id=ignore_id,
                       pad_left=padding_side == "left", trunc_left=truncation_side == "left", int64=int64,
                       stream=torch.cuda.current_stream(dev).cuda_stream)
    return out


def collate_pair_flags(bos_id=None, sep_id=None, eos_id=None, pad_left=False, trunc_left=False, int64=True, mask_a=False,
                       trim_a_first=False) -> int:
    return (collate_flags(bos_id, eos_id, pad_left, trunc_left, int64) | (COLLATE_SEP if sep_id is not None else 0)
            | (COLLATE_MASK_A if mask_a else 0) | (COLLATE_TRIM_A_FIRST if trim_a_first else 0))


def collate_pair_device(a, b, n_str: int, input_ids_ptr: int, row_len: int, *, mask_ptr: int = 0, labels_ptr: int = 0,
                        token_type_ptr: int = 0, lengths_ptr: int = 0, b_start_ptr: int = 0, row_stride: int = 0,
                        pad_id: int = 0, bos_id: Optional[int] = None, sep_id: Optional[int] = None,
                        eos_id: Optional[int] = None, ignore_id: int = -100, max_a: int = 0, max_b: int = 0,
                        pad_left: bool = False, trunc_left: bool = False, int64: bool = True, mask_a: bool = False,
                        trim_a_first: bool = False, stream: int = 0) -> None:
    """dpt_collate_pair over device addresses (0 = NULL): stream-ordered, no sync.  ``a`` / ``b``: each side as
    ``(ids_ptr, off_ptr, counts_ptr, status_ptr)`` -- ``counts_ptr`` 0: ``off`` is dpt_encode's id_off, else
    dpt_encode_padded's str_off and counts; ``status_ptr`` 0: all 0.  ``bos_id`` / ``sep_id`` / ``eos_id`` None: no such
    special.  Rows are int64, or int32 with ``int64=False``; ``lengths`` and ``b_start`` are uint32."""
    if not _lib.has_collate_pair():
        raise DptError("this libdpt.so has no dpt_collate_pair")
    sides = [CollateSide(*(int(x) or None for x in side)) for side in (a, b)]
    opts = CollatePairOpts(row_len, row_stride, pad_id, bos_id or 0, sep_id or 0, eos_id or 0, ignore_id, max_a, max_b,
                           collate_pair_flags(bos_id, sep_id, eos_id, pad_left, trunc_left, int64, mask_a, trim_a_first))
    check(_lib.lib().dpt_collate_pair(ctypes.byref(sides[0]), ctypes.byref(sides[1]), n_str, ctypes.byref(opts), input_ids_ptr,
                                      mask_ptr, labels_ptr, token_type_ptr, lengths_ptr, b_start_ptr, stream),
          "dpt_collate_pair")


def pair_model_inputs(a, b, *, padding: str = "longest", max_length: Optional[int] = None,
                      pad_to_multiple_of: Optional[int] = None, max_source: Optional[int] = None,
                      max_target: Optional[int] = None, labels: bool = False, mask_source: bool = False,
                      token_type_ids: bool = False, trim: str = "target", pad_id: int = 0, bos_id: Optional[int] = None,
                      sep_id: Optional[int] = None, eos_id: Optional[int] = None, ignore_id: int = -100,
                      padding_side: str = "right", truncation_side: str = "right", int64: bool = True) -> Dict[str, object]:
    """Two encoded batches of the same n_str strings -> ``{"input_ids", "attention_mask", "lengths", "b_start"[,
    "labels"][, "token_type_ids"]}``: row s is ``[bos] + a's string s + [sep] + b's string s + [eos]``, filled on torch's
    current stream by one dpt_collate_pair launch (include/dpt.h has the rule).

    Each side is ``(ids, off[, status[, counts]])`` as ``model_inputs`` takes them, in either layout independently (the
    two may be views of one encode's buffers).  ``max_source`` / ``max_target`` cap a side's tokens; a row longer than the
    row length loses tokens of ``trim`` ("target" or "source") first.  ``mask_source``: the labels are ``ignore_id`` on
    the bos, the source and the sep.  ``padding="longest"``: the row length is the longest capped pair plus the
    specials, read back from the counts or offsets (that one scalar is the only synchronisation), capped by
    ``max_length``; ``"max_length"`` synchronises nothing.  ``b_start`` (int32 per row) is the column of the target's
    first position."""
    import torch
    _check_padding(padding, padding_side, truncation_side)
    if trim not in ("target", "source"):
        raise ValueError("trim must be 'target' or 'source'")
    (side_a, n_str), (side_b, n_b) = _check_side(torch, a, "a"), _check_side(torch, b, "b")
    if n_str < 0 or n_b != n_str:
        raise ValueError("both off tensors need the same n_str + 1 entries")
    dev = side_a[0].device
    if side_b[0].device != dev:
        raise ValueError("both sides must be on one device")
    caps = [int(max_source or 0), int(max_target or 0)]
    n_special = (bos_id is not None) + (sep_id is not None) + (eos_id is not None)
    row_len = _row_len(torch, [side_a, side_b], caps, n_str, n_special, padding, max_length, pad_to_multiple_of)
    rows = ["input_ids", "attention_mask"] + (["labels"] if labels else []) + (["token_type_ids"] if token_type_ids else [])
    out = _alloc(torch, rows, ["lengths", "b_start"], n_str, row_len, int64, dev)
    if n_str == 0:
        return out
    (ptrs_a, _keep_a), (ptrs_b, _keep_b) = _side_ptrs(torch, side_a), _side_ptrs(torch, side_b)
    with torch.cuda.device(dev):
        collate_pair_device(ptrs_a, ptrs_b, n_str, out["input_ids"].data_ptr(), row_len,
                            mask_ptr=out["attention_mask"].data_ptr(), labels_ptr=out["labels"].data_ptr() if labels else 0,
                            token_type_ptr=out["token_type_ids"].data_ptr() if token_type_ids else 0,
                            lengths_ptr=out["lengths"].data_ptr(), b_start_ptr=out["b_start"].data_ptr(), pad_id=pad_id,
                            bos_id=bos_id, sep_id=sep_id, eos_id=eos_id, ignore_id=ignore_id, max_a=caps[0], max_b=caps[1],
                            pad_left=padding_side == "left", trunc_left=truncation_side == "left", int64=int64,
                            mask_a=mask_source, trim_a_first=trim == "source",
                            stream=torch.cuda.current_stream(dev).cuda_stream)
    return out
