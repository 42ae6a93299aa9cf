"""TEST INFRASTRUCTURE: a plain-Python model of the device-side default (greedy BPE) encoding (include/dpt.h
dpt_bpe_create / dpt_bpe_encode; csrc/dpt_bpe.cpp and csrc/dpt_bpe.hip) and of the llama ATOMS form
(dpt_pretok_write_atoms), built on tests/pretok_ref.py.  The rule: every atom becomes the id of the token with exactly
its bytes; within each word the symbols merge until no adjacent pair is in the table, each step merging the adjacent
pair of lowest (rank, position); nothing merges across a word start."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

import pretok_ref as pr

NO_TOKENIZATION = 1                 # DPT_STATUS_NO_TOKENIZATION
NO_RANK = 0xFFFFFFFF

Table = Dict[Tuple[int, int], Tuple[int, int]]   # (left, right) -> (rank, merged)


def table_of(left, right, merged, rank) -> Table:
    t: Table = {}
    for a, b, m, r in zip(left, right, merged, rank):
        assert (int(a), int(b)) not in t
        t[(int(a), int(b))] = (int(r), int(m))
    return t


def merge_word(sym: Sequence[int], table: Table) -> List[int]:
    """One word's symbols merged: a dict lookup per adjacent pair and a linear argmin per step."""
    sym = list(sym)
    while len(sym) > 1:
        best = None
        for i in range(len(sym) - 1):
            e = table.get((sym[i], sym[i + 1]))
            if e is not None and (best is None or e[0] < best[0]):
                best = (e[0], i, e[1])
        if best is None:
            break
        sym[best[1]:best[1] + 2] = [best[2]]
    return sym


def merge_word_fast(sym: Sequence[int], table: Table) -> List[int]:
    """``merge_word`` for long words: the same rule over linked slots with a heap of (rank, position) keys, stale
    entries skipped (positions never reorder, so the heap's order is the rule's)."""
    import heapq
    sym = list(sym)
    n = len(sym)
    nxt, prv, alive = list(range(1, n + 1)), list(range(-1, n - 1)), [True] * n
    heap = []

    def push(i):
        j = nxt[i]
        if j < n:
            e = table.get((sym[i], sym[j]))
            if e is not None:
                heapq.heappush(heap, (e[0], i, sym[i], sym[j], e[1]))

    for i in range(n - 1):
        push(i)
    while heap:
        _, i, a, b, m = heapq.heappop(heap)
        j = nxt[i] if alive[i] else n
        if not alive[i] or j >= n or sym[i] != a or sym[j] != b:
            continue
        sym[i], alive[j] = m, False
        nxt[i] = nxt[j]
        if nxt[j] < n:
            prv[nxt[j]] = i
        push(i)
        if prv[i] >= 0:
            push(prv[i])
    return [s for s, a in zip(sym, alive) if a]


def encode_one(piece_id: Dict[bytes, int], table: Table, text2: bytes, cut: bytes, fast: bool = False):
    """One ATOMS string -> (status, ids, tok_word)."""
    if not text2:
        return 0, [], []
    starts = [i for i in range(len(text2)) if i == 0 or cut[i] & 3] + [len(text2)]
    words: List[List[int]] = []
    for a, b in zip(starts, starts[1:]):
        tid = piece_id.get(text2[a:b])
        if tid is None:
            return NO_TOKENIZATION, [], []
        if a == 0 or cut[a] & 1:
            words.append([])
        words[-1].append(tid)
    ids, tok_word = [], []
    for k, w in enumerate(words):
        m = (merge_word_fast if fast or len(w) > 64 else merge_word)(w, table)
        ids += m
        tok_word += [k] * len(m)
    return 0, ids, tok_word


def encode(piece_id: Dict[bytes, int], table: Table, lens: Sequence[int], text2: bytes, cut: bytes):
    """A batch of ATOMS strings, back to back in text2 / cut -> per string (status, ids, tok_word)."""
    out, o = [], 0
    for n in lens:
        n = int(n)
        out.append(encode_one(piece_id, table, text2[o:o + n], cut[o:o + n]))
        o += n
    return out


def piece_ids(t2i: Dict[str, int]) -> Dict[bytes, int]:
    return {k.encode("utf-8", "surrogatepass"): v for k, v in t2i.items()}


# ------------------------------------------------------------------ the llama ATOMS form

def atoms_one(t: pr.Table, s: bytes) -> Tuple[int, bytes, bytes]:
    """``pretok_ref.presplit_one`` with an ATOMS mask: the same text; 3 at the output's first byte and at every
    word-opening U+2581, 2 at the first byte of every other atom -- the BOS piece is one atom, each known character
    one, each <0xNN> of byte fallback one (six bytes); a literal "<0x41>" typed in the text is six."""
    st, text2, cut1 = pr.presplit_one(t, s)
    if st != 0:
        return st, b"", b""
    cut = bytearray(len(text2))
    pos = len(t.bos)
    if text2:
        cut[0] = 3
    chars = s.decode("utf-8")

    def put(n: int, m: int):
        nonlocal pos
        cut[pos] = m
        pos += n

    if chars:
        put(3, 3)
    for ch in chars:
        if ch == " ":
            put(3, 3)
        elif ord(ch) in t.known:
            put(len(ch.encode("utf-8")), 2)
        else:
            for _ in ch.encode("utf-8"):
                put(6, 2)
    assert pos == len(text2) and all((c & 1) == d for c, d in zip(cut, cut1))
    return 0, text2, bytes(cut)


def atoms(t: pr.Table, strings: Sequence[bytes]):
    """A batch -> (pre_status int32[n], out_len uint64[n], text2 bytes, cut bytes), as ``pretok_ref.presplit``."""
    st, ln, txt, cut = [], [], [], []
    for s in strings:
        a, b, c = atoms_one(t, s)
        st.append(a), ln.append(len(b)), txt.append(b), cut.append(c)
    return np.array(st, dtype=np.int32), np.array(ln, dtype=np.uint64), b"".join(txt), b"".join(cut)
