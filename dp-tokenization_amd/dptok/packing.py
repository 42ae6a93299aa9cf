"""Sequence packing on the device (dpt_pack_sizes, dpt_pack_plan, dpt_pack_write; include/dpt.h has the rule):
consecutive strings of an encoded batch packed in order into rows of ``row_len`` tokens, no sequence split, with
``position_ids`` / ``segment_ids`` per token and the placement of every string.

``pack_sizes_device`` / ``pack_plan_device`` / ``pack_write_device`` are the raw calls over device addresses;
``plan_lengths`` plans any lengths tensor; ``packed_inputs`` is the whole route over the torch tensors of an encode."""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

from . import _lib
from ._lib import (COLLATE_BOS, COLLATE_EOS, COLLATE_I64, COLLATE_TRUNC_LEFT, PACK_MASK_FIRST, CollateOpts, CollateSide,
                   DptError, check)
from .collate import _check_side, _side_ptrs


def pack_flags(bos_id=None, eos_id=None, trunc_left=False, int64=True, mask_first=False) -> int:
    return ((COLLATE_BOS if bos_id is not None else 0) | (COLLATE_EOS if eos_id is not None else 0)
            | (COLLATE_TRUNC_LEFT if trunc_left else 0) | (COLLATE_I64 if int64 else 0) | (PACK_MASK_FIRST if mask_first else 0))


def _need():
    if not _lib.has_packing():
        raise DptError("this libdpt.so has no packing calls")
    return _lib.lib()


def pack_geometry():
    """dpt_debug_pack_geometry: (the strings one plan block takes, the plan's grid cap); needs no device."""
    b, cap = _lib.U32(), _lib.U32()
    check(_need().dpt_debug_pack_geometry(ctypes.byref(b), ctypes.byref(cap)), "dpt_debug_pack_geometry")
    return b.value, cap.value


def plan_workspace_bytes(n_str: int) -> int:
    n = _lib.U64()
    check(_need().dpt_pack_plan_workspace(n_str, ctypes.byref(n)), "dpt_pack_plan_workspace")
    return n.value


def pack_sizes_device(off_ptr: int, n_str: int, lengths_ptr: int, row_len: int, *, counts_ptr: int = 0, status_ptr: int = 0,
                      bos_id: Optional[int] = None, eos_id: Optional[int] = None, stream: int = 0) -> None:
    """dpt_pack_sizes over device addresses (0 = NULL): ``lengths`` (uint32 per string) as dpt_collate gives them."""
    opts = CollateOpts(row_len, 0, 0, bos_id or 0, eos_id or 0, 0, pack_flags(bos_id, eos_id, int64=False))
    check(_need().dpt_pack_sizes(off_ptr, counts_ptr, status_ptr, n_str, ctypes.byref(opts), lengths_ptr, stream), "dpt_pack_sizes")


def pack_plan_device(tok_off_ptr: int, n_str: int, row_len: int, row_cap: int, n_rows_ptr: int, ws_ptr: int, ws_bytes: int, *,
                     str_row_ptr: int = 0, str_col_ptr: int = 0, row_first_ptr: int = 0, row_fill_ptr: int = 0, stream: int = 0) -> None:
    """dpt_pack_plan over device addresses (0 = NULL): ``tok_off`` the exclusive prefix sum of the lengths (uint64,
    n_str + 1), ``n_rows`` a device uint64, ``row_first`` of row_cap + 1 and ``row_fill`` of row_cap uint32."""
    check(_need().dpt_pack_plan(tok_off_ptr, n_str, row_len, row_cap, str_row_ptr, str_col_ptr, row_first_ptr, row_fill_ptr,
                                n_rows_ptr, ws_ptr, ws_bytes, stream), "dpt_pack_plan")


def pack_write_device(side, n_str: int, tok_off_ptr: int, row_first_ptr: int, n_rows_ptr: int, row_cap: int, input_ids_ptr: int,
                      row_len: int, *, position_ids_ptr: int = 0, segment_ids_ptr: int = 0, labels_ptr: int = 0, row_stride: int = 0,
                      pad_id: int = 0, bos_id: Optional[int] = None, eos_id: Optional[int] = None, ignore_id: int = -100,
                      trunc_left: bool = False, int64: bool = True, mask_first: bool = False, stream: int = 0) -> None:
    """dpt_pack_write over device addresses (0 = NULL); ``side``: the source as ``(ids_ptr, off_ptr, counts_ptr,
    status_ptr)``.  Rows are int64, or int32 with ``int64=False``."""
    cside = CollateSide(*(int(x) or None for x in side))
    opts = CollateOpts(row_len, row_stride, pad_id, bos_id or 0, eos_id or 0, ignore_id,
                       pack_flags(bos_id, eos_id, trunc_left, int64, mask_first))
    check(_need().dpt_pack_write(ctypes.byref(cside), n_str, tok_off_ptr, row_first_ptr, n_rows_ptr, row_cap, ctypes.byref(opts),
                                 input_ids_ptr, position_ids_ptr, segment_ids_ptr, labels_ptr, stream), "dpt_pack_write")


def _tok_off(torch, lengths):
    """the exclusive prefix sum of int32 lengths as n + 1 int64 entries (uint64 bit patterns)"""
    tok_off = torch.zeros(lengths.numel() + 1, dtype=torch.int64, device=lengths.device)
    torch.cumsum(lengths, 0, dtype=torch.int64, out=tok_off[1:])
    return tok_off


def _plan(torch, tok_off, n_str, row_len, rows):
    """One dpt_pack_plan on torch's current stream over ``tok_off`` -> (placement dict, the rows, n_rows on the
    device).  ``rows`` None: the row arrays are sized for the bound n_rows <= n_str, n_rows is read back and they are
    cut to it."""
    dev = tok_off.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws_bytes = plan_workspace_bytes(n_str)
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.int32, device=dev)
    n_rows = torch.empty(1, dtype=torch.int64, device=dev)
    cap = n_str if rows is None else int(rows)
    # (one spare entry each, so that every tensor has an address)
    str_row, str_col, row_fill = (torch.empty(n + 1, dtype=torch.int32, device=dev) for n in (n_str, n_str, cap))
    row_first = torch.empty(cap + 1, dtype=torch.int32, device=dev)
    pack_plan_device(tok_off.data_ptr(), n_str, row_len, cap, n_rows.data_ptr(), ws.data_ptr(), ws_bytes, str_row_ptr=str_row.data_ptr(),
                     str_col_ptr=str_col.data_ptr(), row_first_ptr=row_first.data_ptr(), row_fill_ptr=row_fill.data_ptr(), stream=stream)
    if rows is None:
        cap = int(n_rows.item())
    return {"str_row": str_row[:n_str], "str_col": str_col[:n_str], "row_first": row_first[:cap + 1], "row_fill": row_fill[:cap],
            "n_rows": cap if rows is None else n_rows[0]}, cap, n_rows


def plan_lengths(lengths, row_len: int, rows: Optional[int] = None) -> Dict[str, object]:
    """A device tensor of per-string lengths (any integer dtype, each <= ``row_len``; 0: the string is not placed)
    -> ``{"str_row", "str_col", "row_first", "row_fill", "n_rows"}`` of the in-order greedy packing into rows of
    ``row_len`` (include/dpt.h dpt_pack_plan), on torch's current stream.  ``str_row`` / ``str_col`` are int32 per
    string (-1 = DPT_PACK_NONE: not placed), ``row_first`` int32 of rows + 1, ``row_fill`` int32 of rows.  ``rows``
    None: ``n_rows`` is read back (the only synchronisation), the arrays hold exactly that many rows and ``n_rows`` is
    an int; ``rows=R``: nothing synchronises, R is the row capacity and ``n_rows`` a device scalar (the need, also
    above R)."""
    import torch
    if not lengths.is_cuda or lengths.dim() != 1:
        raise ValueError("lengths must be a 1-d device tensor")
    with torch.cuda.device(lengths.device):
        out, _, _ = _plan(torch, _tok_off(torch, lengths), lengths.numel(), int(row_len), rows)
    return out


def packed_inputs(ids, off, status=None, counts=None, *, max_length: int, rows: Optional[int] = None, position_ids: bool = True,
                  segment_ids: bool = True, labels: bool = False, mask_first: bool = False, pad_id: int = 0,
                  bos_id: Optional[int] = None, eos_id: Optional[int] = None, ignore_id: int = -100,
                  truncation_side: str = "right", int64: bool = True) -> Dict[str, object]:
    """Torch device tensors of an encoded batch (as ``collate.model_inputs`` takes them) -> packed rows of
    ``max_length`` tokens: ``{"input_ids"[, "position_ids"][, "segment_ids"][, "labels"], "lengths", "str_row",
    "str_col", "row_first", "row_fill", "n_rows"}``, made on torch's current stream by dpt_pack_sizes, a cumsum,
    dpt_pack_plan and dpt_pack_write.  The attention mask is ``segment_ids != 0``; ``mask_first``: the labels are
    ``ignore_id`` on the first position of every sequence.  ``rows`` None: ``n_rows`` is read back -- that one scalar is
    the only synchronisation -- and the rows are allocated exactly; ``rows=R``: nothing synchronises, the tensors have R
    rows (those past the need are pad, the sequences past R rows are dropped) and ``n_rows`` is a device scalar."""
    import torch
    if truncation_side not in ("left", "right"):
        raise ValueError("truncation_side must be 'left' or 'right'")
    side, n_str = _check_side(torch, (ids, off, status, counts))
    if n_str < 0:
        raise ValueError("off needs n_str + 1 entries")
    row_len = int(max_length)
    if row_len < max((bos_id is not None) + (eos_id is not None), 1):
        raise ValueError("max_length holds fewer elements than the specials asked for")
    dev = ids.device
    dtype = torch.int64 if int64 else torch.int32
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        (ids_ptr, off_ptr, counts_ptr, status_ptr), _keep = _side_ptrs(torch, side)
        lengths = torch.empty(n_str, dtype=torch.int32, device=dev)
        if n_str:
            pack_sizes_device(off_ptr, n_str, lengths.data_ptr(), row_len, counts_ptr=counts_ptr, status_ptr=status_ptr,
                              bos_id=bos_id, eos_id=eos_id, stream=stream)
        tok_off = _tok_off(torch, lengths)
        out, cap, n_rows = _plan(torch, tok_off, n_str, row_len, rows)
        want = ["input_ids"] + [k for k, on in (("position_ids", position_ids), ("segment_ids", segment_ids), ("labels", labels)) if on]
        fill = {"input_ids": pad_id, "position_ids": 0, "segment_ids": 0, "labels": ignore_id}
        for k in want:   # (no string: no launch, the rows are all pad)
            out[k] = torch.empty((cap, row_len), dtype=dtype, device=dev) if n_str else torch.full((cap, row_len), fill[k], dtype=dtype, device=dev)
        if n_str and cap:
            pack_write_device((ids_ptr, off_ptr, counts_ptr, status_ptr), n_str, tok_off.data_ptr(), out["row_first"].data_ptr(),
                              n_rows.data_ptr(), cap, out["input_ids"].data_ptr(), row_len,
                              position_ids_ptr=out["position_ids"].data_ptr() if position_ids else 0,
                              segment_ids_ptr=out["segment_ids"].data_ptr() if segment_ids else 0,
                              labels_ptr=out["labels"].data_ptr() if labels else 0, pad_id=pad_id, bos_id=bos_id, eos_id=eos_id,
                              ignore_id=ignore_id, trunc_left=truncation_side == "left", int64=int64, mask_first=mask_first, stream=stream)
        out["lengths"] = lengths
    return out
