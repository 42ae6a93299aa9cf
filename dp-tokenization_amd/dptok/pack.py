"""Host arrays in and out of the engine (the library is never loaded here): strings, vocabularies, words
and atoms -> the CSR buffers the C-ABI takes, and its CSR ids -> Python lists and ``TokenSpans``.  numpy
throughout; ctypes only to turn an array into the ``void *`` a call takes (``_ptr``, ``HostBatch``).
"""
from __future__ import annotations

import ctypes
import gc
import itertools
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from ._lib import STATUS_EMPTY_WORD, STATUS_OK, DptError

try:   # built with libdpt.so (csrc/Makefile); the pure-Python conversion below gives the same lists
    from . import _pylists
except ImportError:   # pragma: no cover
    _pylists = None


def encode_utf8(s: str) -> bytes:
    return s.encode("utf-8", "surrogatepass")


def _csr_bytes(pieces: Sequence[bytes], lens: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Byte pieces -> (blob u8: the pieces back to back and a NUL, off u64[n+1]); ``lens``: the bytes of
    each of the n strings where a string is several pieces (default: one piece each)."""
    if lens is None:
        lens = list(map(len, pieces))
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = lens
    off.cumsum(out=off)                              # (in place: no temporary, no list -> array pass of its own)
    return np.frombuffer(b"".join(pieces) + b"\0", dtype=np.uint8), off


def _flat_counts(lists: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """Lists of ints -> (their values back to back int64[], the length of each int64[n])."""
    cnt = np.fromiter((len(x) for x in lists), dtype=np.int64, count=len(lists))
    return np.fromiter(itertools.chain.from_iterable(lists), dtype=np.int64, count=int(cnt.sum())), cnt


def pack_strings(texts: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    return _csr_bytes([encode_utf8(t) for t in texts])


def pack_vocab(t2i: Dict[str, int]):
    """``t2i`` as dpt_vocab_create and dpt_detok_create take it -> (blob u8: the tokens' UTF-8 bytes back to
    back and a NUL, off u64[n+1], ids int32[n], n)."""
    blob, off = _csr_bytes([encode_utf8(t) for t in t2i])
    return blob, off, np.array(list(t2i.values()), dtype=np.int32), len(t2i)


def _pack_id_lists(id_lists):
    """List of id lists -> (ids int32[], id_off u64[n+1])."""
    ids, cnt = _flat_counts(id_lists)
    if len(ids) and (int(ids.min()) < -2**31 or int(ids.max()) >= 2**31):
        raise DptError("decode: an id outside int32")
    id_off = np.zeros(len(id_lists) + 1, dtype=np.uint64)
    if len(cnt):
        id_off[1:] = np.cumsum(cnt, dtype=np.uint64)
    return ids.astype(np.int32), id_off


def _pack_atoms(strings, empty_word_ok: bool):
    """Strings as words of atoms -> (text, offsets, cut mask: bit 1 at every atom's first byte, bit 0 at
    every word's)."""
    parts, cuts, lens = [], [], []
    for words in strings:
        n = 0
        for atoms in words:
            for k, a in enumerate(atoms):
                e = encode_utf8(a)
                if not e:
                    raise ValueError("empty atom")
                c = bytearray(len(e))
                c[0] = 3 if k == 0 else 2          # bit 1: atom start, bit 0: word start
                parts.append(e)
                cuts.append(bytes(c))
                n += len(e)
            if not atoms and not empty_word_ok:
                raise ValueError("empty word")
        lens.append(n)
    text, offs = _csr_bytes(parts, lens)
    return text, offs, np.frombuffer(b"".join(cuts) + b"\0", dtype=np.uint8)


def atoms_to_csr(atom_lists: Sequence[Sequence[str]]):
    """Lists of atom strings -> (text, offsets, cut mask) for DPT_MODE_ATOMS (one word per list:
    bit 1 marks every atom start, bit 0 the first).  Empty atoms are not representable; an empty list
    is a zero-length string."""
    return _pack_atoms([(atoms,) for atoms in atom_lists], True)


def pack_word_atoms(strings: Sequence[Sequence[Sequence[str]]]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Strings given as words of atoms -> DPT_MODE_ATOMS buffers (text u8, offsets u64[n+1], cut
    mask u8: bit 1 at every atom's first byte, bit 0 at every word's).  Raises ValueError for an
    empty atom or an empty word."""
    return _pack_atoms(strings, False)


def pack_presplit_words(strings: Sequence[Sequence[str]]):
    """Strings given as lists of words -> DPT_MODE_PRESPLIT buffers (text u8, offsets u64[n+1], cut
    mask u8 = 1 at every word's first byte) + per string its word count and the index of its first
    empty word (-1: none; the string is cut there, see ``presplit_outcome``)."""
    enc_words, n_words, cut_at = [], [], []
    for words in strings:
        k = next((i for i, w in enumerate(words) if not w), -1)
        ws = words if k < 0 else words[:k]
        enc_words.extend(encode_utf8(w) for w in ws)
        n_words.append(len(ws))
        cut_at.append(k)
    text, wend = _csr_bytes(enc_words)               # wend[k]: the bytes of the first k words
    offs = wend[np.concatenate([[0], np.cumsum(n_words, dtype=np.int64)])]
    cut = np.zeros(len(text), dtype=np.uint8)
    cut[wend[:-1].astype(np.int64)] = 1              # every word's first byte
    return text, offs, cut, n_words, cut_at


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class HostBatch(NamedTuple):
    """A host batch as the C-ABI takes it; it holds the arrays its pointers point into."""
    text: np.ndarray                    # contiguous u8
    offs: np.ndarray                    # contiguous u64[n + 1]
    cut_mask: Optional[np.ndarray]      # contiguous u8, or None
    n: int                              # strings
    n_bytes: int                        # offs[-1] - offs[0]
    p_text: ctypes.c_void_p             # text and cut_mask at offs[0]: a batch may start anywhere in its buffers
    p_cut: Optional[ctypes.c_void_p]
    p_offs: ctypes.c_void_p


def _host_batch(text, offs, cut_mask=None) -> HostBatch:
    """The argument prelude of every host-buffer call, done once."""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    if cut_mask is not None:
        cut_mask = np.ascontiguousarray(cut_mask, dtype=np.uint8)
    n = len(offs) - 1
    n_bytes = int(offs[-1] - offs[0]) if n >= 0 else 0
    base = int(offs[0])
    return HostBatch(text, offs, cut_mask, n, n_bytes, _ptr(text[base:] if base else text),
                     _ptr(cut_mask[base:] if cut_mask is not None else None), _ptr(offs))


def presplit_outcome(status, n_words, cut_at) -> Tuple[np.ndarray, np.ndarray]:
    """The empty-word rule for a ``pack_presplit_words`` batch -> (status int32[n], none bool[n]).  Words
    are processed in order like the reference's loop (tokenizer_utils.py:70-75): an empty word raises
    IndexError there (dp_tokenize.py:49) unless an earlier word already failed (no tokenization ->
    ValueError), so a string is cut at its first empty word and its status becomes EMPTY_WORD when the
    prefix before it tokenized (or was empty).  ``none``: no words at all, the loop emits nothing."""
    status = np.asarray(status, dtype=np.int32)
    cut_at = np.asarray(cut_at, dtype=np.int64)
    none = (cut_at < 0) & (np.asarray(n_words, dtype=np.int64) == 0)
    empty = (cut_at >= 0) & ((status == STATUS_OK) | (status == STATUS_EMPTY_WORD))
    return np.where(empty, np.int32(STATUS_EMPTY_WORD), status), none


_WS_BYTES = "▁".encode("utf-8")


class PieceTable:
    """Per vocabulary id: the piece's UTF-8 bytes and whether it starts with '▁' -- llama mode's
    host pre-tokenization (reference packages/tokenizer_utils.py:24-31: ids -> pieces through the
    inverted vocabulary, then ``merge_tokens(sep='▁')`` :7-22) as array gathers over a whole
    batch.  merge_tokens starts a word at the first piece and at every piece that starts with the
    separator and appends every other piece to the current word, so a string's pre-split text is
    the concatenation of its pieces' bytes, with a word start at the first piece and at each '▁'
    piece -- the bytes and cut mask ``pack_presplit_words`` builds from the merged words."""

    def __init__(self, t2i: Dict[str, int]):
        ids = np.fromiter(t2i.values(), dtype=np.int64, count=len(t2i))
        n = int(ids.max()) + 1 if len(ids) else 0
        # a dense table only (ids of get_vocab() are 0..|V|-1); negative or very sparse ids: unusable
        self.ok = len(ids) > 0 and int(ids.min()) >= 0 and n <= 4 * len(ids) + 1024
        if not self.ok:
            return
        inv = {}
        for tok, i in t2i.items():   # the last token of a duplicated id wins, like {v: k for k, v in items}
            inv[i] = tok
        enc = [encode_utf8(inv[i]) if i in inv else b"" for i in range(n)]
        self.present = np.zeros(n, dtype=bool)
        self.present[list(inv.keys())] = True
        self.blob, pend = _csr_bytes(enc)
        self.poff = pend[:-1].astype(np.int64)
        self.plen = pend[1:].astype(np.int64) - self.poff
        self.ws = np.fromiter((e.startswith(_WS_BYTES) for e in enc), dtype=bool, count=n)
        # merge_tokens of a list with an empty piece can yield an empty word (IndexError in the
        # reference's DP): such a vocabulary takes the word-list path
        self.empty_piece = bool((self.plen[self.present] == 0).any())

    def pack(self, id_lists: Sequence[Sequence[int]]):
        """Token ids per string -> (text u8, offsets u64[n+1], cut mask u8, pieces per string) for
        DPT_MODE_PRESPLIT.  KeyError for an id outside the vocabulary (the reference's
        ``vocab_bidict.inverse[token]``)."""
        n_str = len(id_lists)
        flat, cnt = _flat_counts(id_lists)
        total = len(flat)
        if total:
            bad = (flat < 0) | (flat >= len(self.present))
            bad[~bad] = ~self.present[flat[~bad]]
            if bad.any():
                raise KeyError(int(flat[np.argmax(bad)]))
        plen = self.plen[flat]
        pend = np.cumsum(plen)
        pstart = pend - plen
        nb = int(pend[-1]) if total else 0
        # byte k of the batch comes from blob[poff[id] + (k - pstart)]
        src = np.repeat(self.poff[flat] - pstart, plen) + np.arange(nb, dtype=np.int64)
        text = np.empty(nb + 1, dtype=np.uint8)
        text[:nb] = self.blob[src]
        text[nb] = 0
        first = np.zeros(total, dtype=bool)
        send = np.cumsum(cnt)
        first[(send - cnt)[cnt > 0]] = True   # every string's first piece opens its first word
        cut = np.zeros(nb + 1, dtype=np.uint8)
        cut[pstart[first | self.ws[flat]]] = 1
        offs = np.zeros(n_str + 1, dtype=np.uint64)
        if n_str:
            offs[1:] = np.concatenate([[0], pend])[send]
        return text, offs, cut, cnt


def csr_lists(ids: np.ndarray, id_off: np.ndarray, status: np.ndarray, none: Optional[np.ndarray] = None,
              keep_failed: bool = True, pylists=_pylists) -> List[Tuple[List[int], int]]:
    """CSR ids -> per string (List[int], status): ([], OK) where ``none``; the string's ids where its
    status is OK or ``keep_failed``; else ([], status).  One C pass (``pylists``, the _pylists extension:
    cached int objects, no intermediate flat list) -- the host path's conversion was ~20x its GPU call;
    ``pylists=None``: the same lists in plain Python."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    id_off = np.ascontiguousarray(id_off, dtype=np.uint64)
    status = np.ascontiguousarray(status, dtype=np.int32)
    if none is not None:
        none = np.ascontiguousarray(none, dtype=np.uint8)
    if pylists is not None:
        # (the cyclic GC off while thousands of new lists appear: each gen-0 pass would re-scan them;
        # lists of ints hold no cycles, and the next collection sees them once)
        was = gc.isenabled()
        gc.disable()
        try:
            return pylists.csr_lists(ids, id_off, status, none, STATUS_OK, 1 if keep_failed else 0)
        finally:
            if was:
                gc.enable()
    flat, o, sl = ids.tolist(), [int(x) - int(id_off[0]) for x in id_off.tolist()], status.tolist()
    nn = none.tolist() if none is not None else [0] * len(sl)
    return [([], STATUS_OK) if nn[i] else
            ((flat[o[i]:o[i + 1]] if (keep_failed or sl[i] == STATUS_OK) else []), sl[i])
            for i in range(len(sl))]


class TokenSpans(NamedTuple):
    """One string's tokenization aligned to its text: ``offsets[k]`` = (start, end) of token k in
    CHARACTERS of ``text`` (the string the engine tokenized), ``word_ids[k]`` the 0-based word it lies in."""
    ids: List[int]
    offsets: List[Tuple[int, int]]
    word_ids: List[int]
    text: str


def csr_token_spans(text: np.ndarray, offs: np.ndarray, ids: np.ndarray, id_off: np.ndarray, tok_end: np.ndarray,
                    tok_word: np.ndarray) -> List[TokenSpans]:
    """``Encoder.encode_csr_spans`` output -> one ``TokenSpans`` per string.  The byte ends become
    character offsets through one count of non-continuation bytes over the batch (a token ends on a
    code-point boundary, so the characters before its end are the non-continuation bytes before it)."""
    o = np.asarray(offs).astype(np.int64)
    raw = np.asarray(text, dtype=np.uint8)[int(o[0]):int(o[-1])]
    o = o - o[0]
    n = len(o) - 1
    cum = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum((raw & 0xC0) != 0x80, out=cum[1:])
    io = np.asarray(id_off).astype(np.int64)
    io = io - io[0]
    cnt = np.diff(io)
    sb = np.repeat(o[:-1], cnt)                     # each token's string start, bytes
    ce = cum[sb + np.asarray(tok_end).astype(np.int64)] - cum[sb]
    cs = np.empty_like(ce)
    cs[1:] = ce[:-1]                                # a token starts where the one before it ends ...
    cs[io[:-1][cnt > 0]] = 0                        # ... and a string's first token at 0
    pairs = list(zip(cs.tolist(), ce.tolist()))
    flat, words, blob = np.asarray(ids).tolist(), np.asarray(tok_word).tolist(), raw.tobytes()
    ol, il = o.tolist(), io.tolist()
    return [TokenSpans(flat[il[s]:il[s + 1]], pairs[il[s]:il[s + 1]], words[il[s]:il[s + 1]],
                       blob[ol[s]:ol[s + 1]].decode("utf-8", "surrogatepass")) for s in range(n)]
