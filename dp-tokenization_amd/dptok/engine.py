"""Host side of the engine: vocabulary upload, batch encode, status -> exception.

This mirrors the reference's L2 adapter (packages/tokenizer_utils.py:52-96) one
level down: a ``Vocab`` is the captured ``t2i``/``vocab`` of ``dp_tokenize_llama``
(:53-57), an ``Encoder`` runs the per-word DP loop of the ``dp_tokenize`` closure
(:66-80) for a whole batch on the GPU.  The numpy packers live in pack.py and ``Detok`` in detok.py;
their names stay importable from here.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, pack
from ._lib import (DPT_FLAG_LEN_ONLY, DPT_FLAG_UNCAPPED, DPT_MODE_ATOMS, DPT_MODE_PRESPLIT, DPT_MODE_RAW, DptError,
                   check, destroy_handle, new_handle)
from .detok import DETOK_RULES, Detok  # noqa: F401
from .pack import (HostBatch, PieceTable, TokenSpans, _host_batch, _ptr, _pylists, atoms_to_csr, csr_token_spans,  # noqa: F401
                   encode_utf8, pack_presplit_words, pack_strings, pack_vocab, pack_word_atoms, presplit_outcome)

MODES = {"raw": DPT_MODE_RAW, "presplit": DPT_MODE_PRESPLIT, "atoms": DPT_MODE_ATOMS, DPT_MODE_RAW: DPT_MODE_RAW,
         DPT_MODE_PRESPLIT: DPT_MODE_PRESPLIT, DPT_MODE_ATOMS: DPT_MODE_ATOMS}


def csr_lists(ids, id_off, status, none=None, keep_failed: bool = True) -> List[Tuple[List[int], int]]:
    """``pack.csr_lists`` through this module's ``_pylists`` (None: the plain-Python conversion)."""
    return pack.csr_lists(ids, id_off, status, none, keep_failed, _pylists)


def raise_for_status(status: int, text: str = "") -> None:
    """Re-raise the reference's exception for a per-string status."""
    if status == _lib.STATUS_OK:
        return
    if status == _lib.STATUS_NO_TOKENIZATION:
        # reference: ipdb.set_trace() then obtain_longest_token([]) -> max([]) (dp_tokenize.py:84)
        raise ValueError("max() arg is an empty sequence (no tokenization of a word of %r)" % text[:60])
    if status == _lib.STATUS_EMPTY_WORD:
        # reference: segment_index_dp[-1] on an empty word (dp_tokenize.py:49)
        raise IndexError("list index out of range (empty word)")
    if status == _lib.STATUS_TOO_LONG:
        raise DptError("input outside the engine's limits (status 3)")
    raise DptError("engine internal error (status %d)" % status)


def raise_and_collect(texts: Sequence[str], results) -> List[List[int]]:
    """Per string (ids, status) -> the ids of every string; the first failed one, in order, raises."""
    out = []
    for t, (ids, st) in zip(texts, results):
        if st != _lib.STATUS_OK:
            raise_for_status(st, t)
        out.append(ids)
    return out


class Vocab:
    """Device-resident vocabulary (double-array byte trie) built from ``t2i``."""

    def __init__(self, t2i: Dict[str, int], device: int = 0):
        blob, off, ids, n = pack_vocab(t2i)
        self.handle = new_handle("dpt_vocab_create", _ptr(blob), _ptr(off), _ptr(ids), n, device)
        self.device = device
        self.t2i = t2i
        st = _lib.VocabStats()
        check(_lib.lib().dpt_vocab_stats_get(self.handle, ctypes.byref(st)), "dpt_vocab_stats_get")
        self.stats = {f: getattr(st, f) for f, _ in st._fields_}

    def __del__(self):
        destroy_handle(self, "handle", "dpt_vocab_destroy")


class Encoder:
    """Batch shortest-tokenization on one GPU (one workspace; use from one stream at a time)."""

    def __init__(self, vocab: Vocab):
        self.vocab = vocab
        self.handle = new_handle("dpt_ctx_create", vocab.device)

    def __del__(self):
        destroy_handle(self, "handle", "dpt_ctx_destroy")

    # ---------------------------------------------------------------- host buffers
    def _encode_host(self, m: int, b: HostBatch):
        n, n_bytes = b.n, b.n_bytes
        if m != DPT_MODE_RAW and b.cut_mask is None:
            raise ValueError("presplit/atoms mode needs cut_mask")
        ids = np.empty(max(n_bytes, 1), dtype=np.int32)
        id_off = np.empty(n + 1, dtype=np.uint64)
        status = np.empty(max(n, 1), dtype=np.int32)
        capped = np.empty(max(n, 1), dtype=np.int32)
        check(_lib.lib().dpt_encode_host(self.handle, self.vocab.handle, m, b.p_text, n_bytes, b.p_offs, b.p_cut, n, _ptr(ids),
                                         max(n_bytes, 1), _ptr(id_off), _ptr(status), _ptr(capped)), "dpt_encode_host")
        return ids[: int(id_off[-1])], id_off, status[:n], capped[:n]

    def encode_csr(self, text: np.ndarray, offs: np.ndarray, mode="raw", cut_mask: Optional[np.ndarray] = None):
        """CSR host arrays in -> (ids int32[], id_off u64[n+1], status int32[n], capped int32[n])."""
        return self._encode_host(MODES[mode], _host_batch(text, offs, cut_mask))

    def encode_csr_spans(self, text: np.ndarray, offs: np.ndarray, mode="raw", cut_mask: Optional[np.ndarray] = None):
        """``encode_csr`` followed by dpt_token_spans_host on its outputs -> (ids, id_off, status, capped,
        tok_end u32[n_tok], tok_word u32[n_tok], span_status int32[n]): token k of string s (index
        id_off[s] + k) covers bytes [tok_end[k-1] or 0, tok_end[k]) of the string and lies in its word
        tok_word[k]; span_status[s] is status[s], or 4 if the ids did not tile the string (never expected)."""
        m = MODES[mode]
        b = _host_batch(text, offs, cut_mask)
        ids, id_off, status, capped = self._encode_host(m, b)
        n, n_tok = b.n, len(ids)
        ids_buf = ids if n_tok else np.zeros(1, dtype=np.int32)
        st_buf = status if n else np.zeros(1, dtype=np.int32)
        tok_end = np.zeros(max(n_tok, 1), dtype=np.uint32)
        tok_word = np.zeros(max(n_tok, 1), dtype=np.uint32)
        span_status = np.zeros(max(n, 1), dtype=np.int32)
        check(_lib.lib().dpt_token_spans_host(self.handle, self.vocab.handle, m, b.p_text, b.n_bytes, b.p_offs, b.p_cut,
                                              n, _ptr(ids_buf), _ptr(id_off), _ptr(st_buf), _ptr(tok_end), _ptr(tok_word),
                                              _ptr(span_status)), "dpt_token_spans_host")
        return ids, id_off, status, capped, tok_end[:n_tok], tok_word[:n_tok], span_status[:n]

    def encode_one(self, s: str) -> Tuple[List[int], int]:
        """One raw-mode string -> (ids, status): the drop-in's per-string call (reference main_analyze_s2orc.py:74-78)
        with as little host work as a ctypes call allows -- the UTF-8 bytes passed as they are, the offsets,
        outputs and their pointers kept from the previous call (dpt_encode_host runs it as one zero-copy launch)."""
        b = s.encode("utf-8", "surrogatepass")
        n = len(b)
        one = self.__dict__.get("_one")
        if one is None or one[0] < n + 1:
            cap = max(4096, 2 * n + 2)
            ids = np.empty(cap, dtype=np.int32)
            off = np.zeros(4, dtype=np.uint64)   # [0:2] the string's offsets (in), [2:4] id_off (out)
            st = np.empty(2, dtype=np.int32)
            L = _lib.lib()
            fn = ctypes.cast(L.dpt_encode_host, ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                                 ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p,
                                                                 ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                                 ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                                                 ctypes.c_void_p))
            one = self._one = (cap, ids, off, st, fn, off.ctypes.data, ids.ctypes.data, st.ctypes.data,
                               st.ctypes.data + 4, off.ctypes.data + 16)
        cap, ids, off, st, fn, p_off, p_ids, p_st, p_cap, p_idoff = one
        off[1] = n
        rc = fn(self.handle, self.vocab.handle, DPT_MODE_RAW, b, n, p_off, None, 1, p_ids, max(n, 1), p_idoff, p_st, p_cap)
        if rc != _lib.DPT_OK:
            check(rc, "dpt_encode_host")
        return ids[:int(off[3])].tolist(), int(st[0])

    def encode_strs(self, texts: Sequence[str]) -> List[Tuple[List[int], int]]:
        text, offs = pack_strings(texts)
        ids, id_off, st, _ = self.encode_csr(text, offs)
        return csr_lists(ids, id_off, st)

    def encode_presplit(self, strings: Sequence[Sequence[str]]) -> List[Tuple[List[int], int]]:
        """Many strings, each pre-split into words (llama mode, DPT_MODE_PRESPLIT), in ONE launch:
        per string (ids, status), ids only where the status is OK.  A string is cut at its first empty
        word and has no words at all when it is empty (``pack.presplit_outcome``)."""
        text, offs, cut, n_words, cut_at = pack_presplit_words(strings)
        ids, id_off, st, _ = self.encode_csr(text, offs, mode="presplit", cut_mask=cut)
        st, none = presplit_outcome(st, n_words, cut_at)
        return csr_lists(ids, id_off, st, none=none, keep_failed=False)

    def encode_packed_presplit(self, text: np.ndarray, offs: np.ndarray, cut: np.ndarray,
                               n_pieces: np.ndarray) -> List[Tuple[List[int], int]]:
        """``PieceTable.pack`` output in ONE launch: per string (ids, status); a string of no pieces
        has no words (the reference's loop emits nothing, status 0).  Pieces are never empty here,
        so no word is."""
        ids, id_off, st, _ = self.encode_csr(text, offs, mode="presplit", cut_mask=cut)
        return csr_lists(ids, id_off, st, none=(np.asarray(n_pieces) == 0), keep_failed=False)

    def encode_words(self, words: Sequence[str]) -> Tuple[List[int], int]:
        """One string pre-split into words (llama mode, DPT_MODE_PRESPLIT): ids and status."""
        return self.encode_presplit([words])[0]

    def encode_word_atoms(self, strings: Sequence[Sequence[Sequence[str]]]) -> List[Tuple[List[int], int]]:
        """Strings given as words of atoms (DPT_MODE_ATOMS), one launch for the batch: per string
        (ids, status).  A string with no words gives ([], ok) -- the BLOOM adapter's empty input
        (reference tokenizer_utils.py:166-178 loops over zero words)."""
        text, o, cut = pack_word_atoms(strings)
        ids, id_off, st, _ = self.encode_csr(text, o, mode="atoms", cut_mask=cut)
        return csr_lists(ids, id_off, st, none=np.fromiter((not words for words in strings), dtype=bool, count=len(strings)))

    def dp(self, text: np.ndarray, offs: np.ndarray, mode="atoms", cut_mask: Optional[np.ndarray] = None,
           uncapped: bool = False, edges: bool = False, far: bool = False):
        """DP by-products without ids (dpt_dp_host): (status, lengths, edges or None), and with ``far``
        (edges only) a 4th value: the (edges index, back distance) pairs of optimal predecessors more
        than 64 atoms back (dpt_dp_host_far), an int array of shape (k, 2).  lengths are the capped
        len_dp[-1] sums (reference dp_tokenize.py:70) or, with ``uncapped``, the minimum token counts
        (65535 per impossible word, inspect_tokenizer.py:77-86)."""
        b = _host_batch(text, offs, cut_mask)
        n, n_bytes = b.n, b.n_bytes
        if int(b.offs[0]) != 0:
            raise ValueError("dp(): offsets must start at 0")
        status = np.empty(max(n, 1), dtype=np.int32)
        lengths = np.empty(max(n, 1), dtype=np.int32)
        ed = np.zeros(max(n_bytes, 1), dtype=np.uint64) if (edges or far) else None
        m = MODES[mode] | (DPT_FLAG_UNCAPPED if uncapped else DPT_FLAG_LEN_ONLY)
        L = _lib.lib()
        if not far:
            check(L.dpt_dp_host(self.handle, self.vocab.handle, m, b.p_text, n_bytes, b.p_offs, b.p_cut,
                                n, _ptr(status), _ptr(lengths), _ptr(ed)), "dpt_dp_host")
            return status[:n], lengths[:n], ed
        cap = 1024
        while True:
            fp = np.zeros((cap, 2), dtype=np.uint64)
            nf = ctypes.c_uint64(0)
            rc = L.dpt_dp_host_far(self.handle, self.vocab.handle, m, b.p_text, n_bytes, b.p_offs, b.p_cut,
                                   n, _ptr(status), _ptr(lengths), _ptr(ed), _ptr(fp), cap, ctypes.byref(nf))
            if rc == _lib.DPT_E_CAP and nf.value > cap:
                cap = int(nf.value)   # the DP runs again with room for every pair
                continue
            check(rc, "dpt_dp_host_far")
            return status[:n], lengths[:n], ed, fp[: nf.value].astype(np.int64)

    # ---------------------------------------------------------------- device buffers
    # (the argument types are void*: a plain int passes as that address, 0 as NULL)
    def encode_device(self, text_ptr: int, n_bytes: int, off_ptr: int, n_str: int, ids_ptr: int, ids_cap: int,
                      idoff_ptr: int, status_ptr: int, capped_ptr: int = 0, cut_ptr: int = 0, stream: int = 0,
                      mode="raw") -> None:
        """All pointers are device addresses (e.g. ``torch.Tensor.data_ptr()``); stream-ordered, no sync."""
        check(_lib.lib().dpt_encode(self.handle, self.vocab.handle, MODES[mode], text_ptr, n_bytes, off_ptr, cut_ptr, n_str,
                                    ids_ptr, ids_cap, idoff_ptr, status_ptr, capped_ptr, stream), "dpt_encode")

    def encode_device_padded(self, text_ptr: int, n_bytes: int, off_ptr: int, n_str: int, ids_ptr: int, ids_cap: int,
                             counts_ptr: int, status_ptr: int, capped_ptr: int = 0, cut_ptr: int = 0, stream: int = 0,
                             mode="raw") -> None:
        """dpt_encode_padded: string s's ids stay at its byte offset, ids[str_off[s]-str_off[0] + k] for
        k < counts[s] (uint64); no CSR packing pass.  Device addresses, stream-ordered, no sync."""
        check(_lib.lib().dpt_encode_padded(self.handle, self.vocab.handle, MODES[mode], text_ptr, n_bytes, off_ptr, cut_ptr,
                                           n_str, ids_ptr, ids_cap, counts_ptr, status_ptr, capped_ptr, stream),
              "dpt_encode_padded")

    def spans_device(self, text_ptr: int, n_bytes: int, off_ptr: int, n_str: int, ids_ptr: int, idoff_ptr: int,
                     status_ptr: int, tok_end_ptr: int, span_status_ptr: int, tok_word_ptr: int = 0, cut_ptr: int = 0,
                     stream: int = 0, mode="raw") -> None:
        """dpt_token_spans on the outputs of an ``encode_device`` call with the same text / offsets / mode:
        tok_end (uint32 per id), tok_word (uint32 per id, 0: not wanted) and span_status (int32 per string).
        Device addresses, stream-ordered, no sync, no workspace (the engine's ctx is not used)."""
        check(_lib.lib().dpt_token_spans(self.vocab.handle, MODES[mode], text_ptr, n_bytes, off_ptr, cut_ptr, n_str, ids_ptr,
                                         idoff_ptr, status_ptr, tok_end_ptr, tok_word_ptr, span_status_ptr, stream),
              "dpt_token_spans")

    def reserve(self, n_bytes: int, n_str: int, long_bytes: int = 0) -> None:
        """Pre-size the workspace for this vocabulary's staging width (a later call of at most that size
        allocates nothing and does not synchronise); ``long_bytes``: input bytes the unbounded pass holds
        per call (0: default).  Not enough to record ``encode_device`` into a HIP graph
        (``torch.cuda.graph``): the engine keeps host state in step with every call, which a replay does
        not see -- capture is not supported."""
        check(_lib.lib().dpt_ctx_reserve_vocab(self.handle, self.vocab.handle, n_bytes, n_str, long_bytes),
              "dpt_ctx_reserve_vocab")

    def _two_u64(self, call: str) -> Tuple[int, int]:
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        check(getattr(_lib.lib(), call)(self.handle, ctypes.byref(a), ctypes.byref(b)), call)
        return a.value, b.value

    def workspace_bytes(self) -> Tuple[int, int]:
        """(device-path workspace, host-path staging) bytes held on the device."""
        return self._two_u64("dpt_ctx_workspace_bytes")

    def long_need(self) -> Tuple[int, int]:
        """(input bytes the last call's unbounded pass took, its arena capacity); call after the
        encode's stream has completed."""
        return self._two_u64("dpt_ctx_long_need")

    def set_histogram(self, hist_ptr: int, n_bins: int, overwrite: bool = False) -> None:
        """Fold the token-count histogram into the next encode on this engine (dpt_ctx_set_histogram_ex:
        its finish pass adds to hist, device int64[n_bins + 8], or with ``overwrite`` replaces it -- the
        device zeroes it first, in stream order); 0 cancels."""
        check(_lib.lib().dpt_ctx_set_histogram_ex(self.handle, hist_ptr, n_bins, 1 if overwrite else 0),
              "dpt_ctx_set_histogram_ex")

    def histogram_device(self, idoff_ptr: int, status_ptr: int, n_str: int, hist_ptr: int, n_bins: int,
                         stream: int = 0) -> None:
        check(_lib.lib().dpt_token_histogram(idoff_ptr, status_ptr, n_str, hist_ptr, n_bins, stream), "dpt_token_histogram")

    def debug_no_lean(self, on: bool) -> None:
        """TEST-ONLY (dpt_ctx_debug_no_lean): this engine's calls without the lean launch."""
        check(_lib.lib().dpt_ctx_debug_no_lean(self.handle, 1 if on else 0), "dpt_ctx_debug_no_lean")

    def debug_lean_words(self):
        """TEST-ONLY (dpt_ctx_debug_lean_words): (hint off, strings the last lean launch deferred, probes so far, calls without
        the lean launch since the hint went off)."""
        out = (ctypes.c_uint32 * 4)()
        check(_lib.lib().dpt_ctx_debug_lean_words(self.handle, out), "dpt_ctx_debug_lean_words")
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def debug_counter_bias(self, bias: int) -> None:
        """TEST-ONLY (dpt_ctx_debug_counter_bias): later calls start the unbounded pass's arena and far-pair
        counters at ``bias`` (results unchanged; its kernels' offsets become >= bias)."""
        check(_lib.lib().dpt_ctx_debug_counter_bias(self.handle, bias), "dpt_ctx_debug_counter_bias")

    def profile(self, on: bool = True) -> None:
        check(_lib.lib().dpt_ctx_profile(self.handle, 1 if on else 0), "dpt_ctx_profile")

    def profile_read(self) -> Tuple[List[float], int]:
        ms = (ctypes.c_double * 3)()
        n = ctypes.c_uint64()
        check(_lib.lib().dpt_ctx_profile_read(self.handle, ms, ctypes.byref(n)), "dpt_ctx_profile_read")
        return [ms[0], ms[1], ms[2]], n.value
