"""The tokenizer's own (greedy BPE) encoding on the device: DPT_MODE_ATOMS input in, ids in the padded layout out.

``Bpe`` holds the pair table (include/dpt.h dpt_bpe_create); ``pairs_from_merges`` and ``pairs_from_scores`` build
its four arrays from a tokenizer.json model or from a SentencePiece model's scores."""
from __future__ import annotations

import json
from typing import Dict, Iterable, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import DptError, check, destroy_handle, new_handle
from .pack import _ptr

NO_RANK = 0xFFFFFFFF


def _arrays(left, right, merged, rank):
    a = [np.ascontiguousarray(x, dtype=np.int64) for x in (left, right, merged, rank)]
    if len({len(x) for x in a}) != 1:
        raise ValueError("left, right, merged and rank differ in length")
    if len(a[0]) and (min(int(x.min()) for x in a) < 0 or max(int(x.max()) for x in a[:3]) > 0x7FFFFFFF or int(a[3].max()) > NO_RANK):
        raise DptError("pair table: an id outside int32 or a rank outside uint32")
    return a[0].astype(np.int32), a[1].astype(np.int32), a[2].astype(np.int32), a[3].astype(np.uint32)


def pairs_from_merges(vocab: Dict[str, int], merges: Iterable, model: dict = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(left, right, merged, rank) from a tokenizer.json BPE model's ``vocab`` and ``merges``: entry k of ``merges``,
    ``"a b"`` (the older form) or ``["a", "b"]``, merges the tokens a and b into a + b at rank k.  ``model`` (the
    tokenizer.json ``model`` object, optional) is refused with ValueError when it sets ``ignore_merges``,
    ``dropout``, a continuing-subword prefix or an end-of-word suffix: the rule here has none of them."""
    if model is not None:
        for key in ("ignore_merges", "dropout", "continuing_subword_prefix", "end_of_word_suffix"):
            if model.get(key):
                raise ValueError(f"pairs_from_merges: the model sets {key}")
    left, right, merged = [], [], []
    for m in merges:
        if isinstance(m, str):
            parts = m.split(" ")
            if len(parts) != 2:
                raise ValueError(f"pairs_from_merges: merge {m!r} is not two tokens")
            a, b = parts
        else:
            a, b = m
        try:
            left.append(vocab[a]), right.append(vocab[b]), merged.append(vocab[a + b])
        except KeyError as e:
            raise ValueError(f"pairs_from_merges: merge ({a!r}, {b!r}) names a token that is not in the vocabulary") from e
    return _arrays(left, right, merged, np.arange(len(left)))


def pairs_from_tokenizer_json(text: str):
    """``pairs_from_merges`` of a tokenizer.json document (what ``backend_tokenizer.to_str()`` returns)."""
    model = json.loads(text)["model"]
    if model.get("type", "BPE") != "BPE":
        raise ValueError("pairs_from_tokenizer_json: the model is not BPE")
    return pairs_from_merges(model["vocab"], model["merges"], model)


def pairs_from_scores(piece_to_id: Dict[str, int], scores: Dict[str, float], exclude_ids: Iterable[int] = ()):
    """(left, right, merged, rank) from a SentencePiece BPE model: every split of every piece that is not excluded
    into two pieces that are not excluded is a pair, merging into the piece at the rank of the piece's score -- the
    dense order of descending score (equal scores share a rank).  ``exclude_ids``: the control, unknown, unused and
    ``<0xNN>`` byte pieces, which never take part in merges."""
    out = set(int(i) for i in exclude_ids)
    pieces = {p: i for p, i in piece_to_id.items() if i not in out}
    order = {s: k for k, s in enumerate(sorted({float(scores[p]) for p in pieces}, reverse=True))}
    left, right, merged, rank = [], [], [], []
    for p, i in pieces.items():
        for cut in range(1, len(p)):
            a, b = pieces.get(p[:cut]), pieces.get(p[cut:])
            if a is not None and b is not None:
                left.append(a), right.append(b), merged.append(i), rank.append(order[float(scores[p])])
    return _arrays(left, right, merged, rank)


def debug_lookup(left, right, merged, rank, q_left, q_right):
    """dpt_debug_bpe_lookup (test-only, no device): the table's answers (merged int32[], rank uint32[]) to the
    queries, -1 and 0xFFFFFFFF for a miss."""
    l, r, m, k = _arrays(left, right, merged, rank)
    ql, qr = np.ascontiguousarray(q_left, dtype=np.int32), np.ascontiguousarray(q_right, dtype=np.int32)
    om, ok = np.empty(max(len(ql), 1), dtype=np.int32), np.empty(max(len(ql), 1), dtype=np.uint32)
    check(_lib.lib().dpt_debug_bpe_lookup(_ptr(l), _ptr(r), _ptr(m), _ptr(k), len(l), _ptr(ql), _ptr(qr), len(ql), _ptr(om), _ptr(ok)),
          "dpt_debug_bpe_lookup")
    return om[:len(ql)], ok[:len(ql)]


class Bpe:
    """Device-resident pair table of a greedy BPE merge (include/dpt.h dpt_bpe_create): entry k merges the adjacent
    symbols ``left[k], right[k]`` into ``merged[k]``, lowest ``rank`` first, leftmost on ties.  Immutable; may be
    shared by threads and streams."""

    def __init__(self, left: Sequence[int], right: Sequence[int], merged: Sequence[int], rank: Sequence[int], device: int = 0):
        if not _lib.has_bpe():   # (loads the library)
            raise DptError(f"{_lib.LIB_PATH} was built before the BPE calls (no dpt_bpe_create): rebuild it")
        l, r, m, k = _arrays(left, right, merged, rank)
        self.handle = new_handle("dpt_bpe_create", _ptr(l), _ptr(r), _ptr(m), _ptr(k), len(l), device)
        self.device = device
        self.n_pairs = len(l)

    def __del__(self):
        destroy_handle(self, "handle", "dpt_bpe_destroy")

    # (the argument types are void*: a plain int passes as that address, 0 as NULL)
    def encode_padded_device(self, vocab, text_ptr: int, n_bytes: int, off_ptr: int, cut_ptr: int, n_str: int, ids_ptr: int,
                             ids_cap: int, counts_ptr: int, status_ptr: int, tok_word_ptr: int = 0, stream: int = 0) -> None:
        """dpt_bpe_encode over ``vocab`` (a ``Vocab``): the ATOMS input's default encoding in ``encode_padded``'s
        layout -- ids (int32) and tok_word (uint32, nullable) at str_off[s] - str_off[0] + k for k < counts[s]
        (uint64 per string), status (int32 per string).  Device addresses, stream-ordered, no sync, no workspace."""
        check(_lib.lib().dpt_bpe_encode(self.handle, vocab.handle, text_ptr, n_bytes, off_ptr, cut_ptr, n_str, ids_ptr, ids_cap,
                                        counts_ptr, status_ptr, tok_word_ptr, stream), "dpt_bpe_encode")

    def encode_atoms(self, vocab, text_t, offs_t, cut_t, tok_word: bool = False):
        """torch device tensors in (ATOMS text uint8, offsets int64[n + 1], cut mask uint8) -> (ids int32[n_bytes],
        counts int64[n], status int32[n], tok_word int32[n_bytes] or None) on the same device; string s's ids are
        ``ids[offs[s] - offs[0]:][:counts[s]]``."""
        import torch
        n, nb, dev = offs_t.numel() - 1, int(text_t.numel()), text_t.device
        with torch.cuda.device(dev):
            ids = torch.empty(max(nb, 1), dtype=torch.int32, device=dev)
            words = torch.empty(max(nb, 1), dtype=torch.int32, device=dev) if tok_word else None
            counts = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
            status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
            if n > 0:
                anchor = ids.data_ptr()   # (an all-empty batch: the call still wants addresses)
                self.encode_padded_device(vocab, text_t.data_ptr() if nb else anchor, nb, offs_t.data_ptr(),
                                          cut_t.data_ptr() if nb else anchor, n, ids.data_ptr(), nb, counts.data_ptr(),
                                          status.data_ptr(), words.data_ptr() if tok_word else 0,
                                          torch.cuda.current_stream(dev).cuda_stream)
        return ids[:nb], counts[:n], status[:n], (words[:nb] if tok_word else None)
