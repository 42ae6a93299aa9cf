"""Decode side of the engine: ids back to bytes and the round-trip check of an encoded batch."""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import numpy as np

from . import _lib
from ._lib import DptError, check, destroy_handle, new_handle
from .pack import _host_batch, _ptr, pack_vocab

DETOK_RULES = {"pieces": _lib.DPT_DETOK_PIECES, "sp": _lib.DPT_DETOK_SP, "bytelevel": _lib.DPT_DETOK_BYTELEVEL}


def _decode_flags(strip_space: bool) -> int:
    return _lib.DPT_DECODE_STRIP_SPACE if strip_space else 0


class Detok:
    """Device-resident decode table of ``t2i`` under one rule (include/dpt.h dpt_detok_create): ids back to
    bytes, and the round-trip check of an encoded batch -- the tokenizer's own ``decode`` of the reference's
    second closure (packages/tokenizer_utils.py:82-84, :176-179) and its caller's assert
    (main_analyze_s2orc.py:84-87) for a whole batch in one launch.

    ``rule``: "pieces" (the tokens' bytes), "sp" (SentencePiece: U+2581 -> ' ', ``<0xNN>`` -> the byte) or
    "bytelevel" (the GPT-2 / ByteLevel alphabet back to bytes); ``skip_ids`` decode to nothing (BOS).
    ``strip_space`` drops a string's first decoded byte when it is ' '.  The output is bytes: nothing is
    validated or repaired as UTF-8."""

    def __init__(self, t2i: Dict[str, int], rule: str = "sp", skip_ids: Iterable[int] = (), device: int = 0):
        if not _lib.has_decode():   # (loads the library)
            raise DptError(f"{_lib.LIB_PATH} was built before the decode calls (no dpt_detok_create): rebuild it")
        blob, off, ids, n = pack_vocab(t2i)
        skip = np.array(list(skip_ids), dtype=np.int32)
        self.handle = new_handle("dpt_detok_create", _ptr(blob), _ptr(off), _ptr(ids), n, DETOK_RULES[rule],
                                  _ptr(skip) if len(skip) else None, len(skip), device)
        self.device = device
        self.rule = rule
        self.ctx = None   # the host paths' staging, made on first use

    def __del__(self):
        destroy_handle(self, "ctx", "dpt_ctx_destroy")
        destroy_handle(self, "handle", "dpt_detok_destroy")

    def _ctx(self):
        if self.ctx is None:
            self.ctx = new_handle("dpt_ctx_create", self.device)
        return self.ctx

    @staticmethod
    def _csr(ids, id_off, status):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        id_off = np.ascontiguousarray(id_off, dtype=np.uint64)
        if len(id_off) < 1:
            raise ValueError("id_off needs n + 1 entries")
        n = len(id_off) - 1
        if status is not None:
            status = np.ascontiguousarray(status, dtype=np.int32)
            if len(status) < n:
                raise ValueError("status shorter than the batch")
        if len(ids) < int(id_off[-1]):
            raise ValueError("ids shorter than id_off[-1]")
        return ids[int(id_off[0]):], id_off, status, n

    # ---------------------------------------------------------------- host buffers
    def decode_csr(self, ids: np.ndarray, id_off: np.ndarray, status: Optional[np.ndarray] = None,
                   strip_space: bool = False):
        """CSR ids in -> (bytes u8[], out_off u64[n+1], dec_status int32[n]): string s decodes to
        bytes[out_off[s]:out_off[s+1]]; dec_status[s] is status[s], or 4 when an id of s has no token (its
        bytes are then unspecified)."""
        ids, id_off, status, n = self._csr(ids, id_off, status)
        flags = _decode_flags(strip_space)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        dec_status = np.zeros(max(n, 1), dtype=np.int32)
        cap = 4 * len(ids) + 64   # (most pieces are shorter; a longer decode answers DPT_E_CAP with its need)
        L = _lib.lib()
        while True:
            out = np.empty(max(cap, 1), dtype=np.uint8)
            rc = L.dpt_decode_host(self._ctx(), self.handle, _ptr(ids), _ptr(id_off), _ptr(status), n, flags, _ptr(out), cap,
                                   _ptr(out_off), _ptr(dec_status))
            if rc == _lib.DPT_E_CAP and int(out_off[-1]) > cap:
                cap = int(out_off[-1])
                continue
            check(rc, "dpt_decode_host")
            return out[: int(out_off[-1])], out_off, dec_status[:n]

    def roundtrip_csr(self, text: np.ndarray, offs: np.ndarray, ids: np.ndarray, id_off: np.ndarray,
                      status: Optional[np.ndarray] = None, strip_space: bool = False):
        """The decode of every string against text[offs[s]:offs[s+1]] without writing it -> (rt int32[n],
        first_diff int64[n]): rt[s] is status[s] when that is not 0, else RT_EQUAL, RT_DIFFERS or 4 (an id
        without a token); first_diff[s] the first differing byte offset (the shorter length when one side is
        a prefix of the other), -1 where rt[s] != RT_DIFFERS."""
        ids, id_off, status, n = self._csr(ids, id_off, status)
        if len(offs) != n + 1:
            raise ValueError("offs and id_off differ in length")
        b = _host_batch(text, offs)
        if len(b.text) < int(b.offs[-1]):
            raise ValueError("text shorter than offs[-1]")
        rt = np.zeros(max(n, 1), dtype=np.int32)
        fd = np.zeros(max(n, 1), dtype=np.uint32)
        check(_lib.lib().dpt_roundtrip_host(self._ctx(), self.handle, _ptr(ids), _ptr(id_off), _ptr(status), b.p_text,
                                            b.p_offs, n, _decode_flags(strip_space), _ptr(rt), _ptr(fd)),
              "dpt_roundtrip_host")
        rt = rt[:n]
        return rt, np.where(rt == _lib.RT_DIFFERS, fd[:n].astype(np.int64), -1)

    # ---------------------------------------------------------------- device buffers
    # (the argument types are void*: a plain int passes as that address, 0 as NULL)
    def sizes_device(self, ids_ptr: int, idoff_ptr: int, n_str: int, out_len_ptr: int, status_ptr: int = 0,
                     strip_space: bool = False, stream: int = 0) -> None:
        """dpt_decode_sizes: out_len (uint64 per string) = the decoded bytes of each string.  Device
        addresses, stream-ordered, no sync, no workspace."""
        check(_lib.lib().dpt_decode_sizes(self.handle, ids_ptr, idoff_ptr, status_ptr, n_str, _decode_flags(strip_space),
                                          out_len_ptr, stream), "dpt_decode_sizes")

    def decode_device(self, ids_ptr: int, idoff_ptr: int, n_str: int, out_ptr: int, out_off_ptr: int, dec_status_ptr: int,
                      status_ptr: int = 0, strip_space: bool = False, stream: int = 0) -> None:
        """dpt_decode: string s's bytes at out + out_off[s] - out_off[0] (out_off: uint64[n_str + 1], the
        prefix sum of ``sizes_device``'s lengths from any start), dec_status int32 per string."""
        check(_lib.lib().dpt_decode(self.handle, ids_ptr, idoff_ptr, status_ptr, n_str, _decode_flags(strip_space),
                                    out_ptr, out_off_ptr, dec_status_ptr, stream), "dpt_decode")

    def roundtrip_device(self, ids_ptr: int, idoff_ptr: int, text_ptr: int, off_ptr: int, n_str: int, rt_ptr: int,
                         first_diff_ptr: int = 0, status_ptr: int = 0, strip_space: bool = False, stream: int = 0) -> None:
        """dpt_roundtrip: rt (int32 per string) and first_diff (uint32 per string, 0: not wanted; written
        only where rt is RT_DIFFERS) of the decode against text / offsets (the encode's own)."""
        check(_lib.lib().dpt_roundtrip(self.handle, ids_ptr, idoff_ptr, status_ptr, text_ptr, off_ptr, n_str,
                                       _decode_flags(strip_space), rt_ptr, first_diff_ptr, stream), "dpt_roundtrip")
