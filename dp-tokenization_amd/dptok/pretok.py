"""Llama mode's pre-tokenization on the device: text in, DPT_MODE_PRESPLIT input (text + cut mask) out."""
from __future__ import annotations

from typing import Dict, Iterable, Sequence

import numpy as np

from . import _lib
from ._lib import DptError, check, destroy_handle, new_handle
from .pack import _csr_bytes, _ptr, encode_utf8

NEEDS_HOST = _lib.PRETOK_NEEDS_HOST


def pack_literals(literals: Iterable[str]):
    """Literal strings -> (blob u8, off u64[n+1], n): each once, in their first order."""
    enc = list(dict.fromkeys(encode_utf8(x) for x in literals))
    blob, off = _csr_bytes(enc)
    return blob, off, len(enc)


def two_pass_split(sizes_device, write_device, text_t, offs_t):
    """The two passes of a device splitter (``Pretok.presplit``, ``ByteLevelSplit.split``) over torch device tensors
    (text uint8, offsets int64[n + 1]) -> (text2 uint8, offs2 int64[n + 1] from 0, cut uint8, pre_status int32[n]) on
    the same device: ``sizes_device``, a cumsum, ``write_device``.  One host read (the total)."""
    import torch
    n = offs_t.numel() - 1
    dev = text_t.device
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if text_t.numel() == 0:   # (a batch of empty strings: the call still wants an address)
            text_t = torch.zeros(1, dtype=torch.uint8, device=dev)
        out_len = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        pre_status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        offs2 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if n > 0:
            sizes_device(text_t.data_ptr(), offs_t.data_ptr(), n, out_len.data_ptr(), pre_status.data_ptr(), stream)
            torch.cumsum(out_len[:n], 0, out=offs2[1:])
        total = int(offs2[-1]) if n > 0 else 0
        text2 = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        cut = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        if n > 0:
            write_device(text_t.data_ptr(), offs_t.data_ptr(), n, pre_status.data_ptr(), text2.data_ptr(),
                         offs2.data_ptr(), cut.data_ptr(), stream)
    return text2[:total], offs2, cut[:total], pre_status[:n]


class Pretok:
    """Device-resident pre-tokenization table of ``t2i`` (include/dpt.h dpt_pretok_create): the words that
    ``pretokenize_with_llama`` + ``merge_tokens`` (reference packages/tokenizer_utils.py:7-31) build from a
    Llama-style SentencePiece model's pieces, written by two kernels for every string whose words are a
    per-character function of its text.  The other strings get ``pre_status`` NEEDS_HOST (6) and no output: a
    leading space, U+2581, one of ``literals`` (the tokenizer's special and added tokens), two spaces in a row
    when the vocabulary has a multi-U+2581 piece, malformed UTF-8.  ``bos_piece``: the piece in front of every
    string ("" or None: none)."""

    def __init__(self, t2i: Dict[str, int], bos_piece: str = "<s>", literals: Sequence[str] = (), device: int = 0):
        if not _lib.has_pretok():   # (loads the library)
            raise DptError(f"{_lib.LIB_PATH} was built before the pre-tokenization calls (no dpt_pretok_create): rebuild it")
        blob, off = _csr_bytes([encode_utf8(t) for t in t2i])
        bos = np.frombuffer(encode_utf8(bos_piece or "") + b"\0", dtype=np.uint8)
        lit, lit_off, n_lit = pack_literals(literals)
        self.handle = new_handle("dpt_pretok_create", _ptr(blob), _ptr(off), len(t2i), _ptr(bos), len(bos) - 1, _ptr(lit),
                                  _ptr(lit_off), n_lit, device)
        self.device = device

    def __del__(self):
        destroy_handle(self, "handle", "dpt_pretok_destroy")

    # (the argument types are void*: a plain int passes as that address, 0 as NULL)
    def sizes_device(self, text_ptr: int, off_ptr: int, n_str: int, out_len_ptr: int, pre_status_ptr: int, stream: int = 0) -> None:
        """dpt_pretok_sizes: out_len (uint64 per string) = the bytes of each string's pre-split form, pre_status
        (int32 per string) = 0 or NEEDS_HOST.  Device addresses, stream-ordered, no sync, no workspace."""
        check(_lib.lib().dpt_pretok_sizes(self.handle, text_ptr, off_ptr, n_str, out_len_ptr, pre_status_ptr, stream),
              "dpt_pretok_sizes")

    def write_device(self, text_ptr: int, off_ptr: int, n_str: int, pre_status_ptr: int, out_text_ptr: int, out_off_ptr: int,
                     cut_ptr: int, stream: int = 0, atoms: bool = False) -> None:
        """dpt_pretok_write: string s's pre-split form at out_text + out_off[s] - out_off[0] and its cut mask at
        the same index of cut (out_off: uint64[n_str + 1], the prefix sum of ``sizes_device``'s lengths from any
        start; pre_status: what it wrote).  ``atoms``: dpt_pretok_write_atoms -- the same text under a
        DPT_MODE_ATOMS mask (3 where a word opens, 2 at every other atom's first byte), ``Bpe``'s input."""
        call = "dpt_pretok_write_atoms" if atoms else "dpt_pretok_write"
        check(getattr(_lib.lib(), call)(self.handle, text_ptr, off_ptr, n_str, pre_status_ptr, out_text_ptr, out_off_ptr,
                                        cut_ptr, stream), call)

    def presplit(self, text_t, offs_t, atoms: bool = False):
        """torch device tensors in (text uint8, offsets int64[n + 1]) -> (text2 uint8, offs2 int64[n + 1] from 0,
        cut uint8, pre_status int32[n]) on the same device: sizes, a cumsum, write.  One host read (the total)."""
        write = (lambda *a: self.write_device(*a, atoms=True)) if atoms else self.write_device
        return two_pass_split(self.sizes_device, write, text_t, offs_t)
