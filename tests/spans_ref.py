"""TEST INFRASTRUCTURE: the expected output of dpt_token_spans by a pure-Python walk.

The engine finds a token's end from the byte lengths of the ids before it and a scan of the text.
The walk here does not: it inverts the vocabulary to strings and consumes each token's string
against the input.  RAW: atom by atom against ``packages.tokenizer_utils.pretokenize_raw`` (pinned to
the reference), one atom per input code point.  PRESPLIT / ATOMS: byte slices of the form's text,
each compared with the token's bytes; words from the cut mask.  It asserts on the way that every
token reproduces the text it covers.
"""
import numpy as np

from packages.tokenizer_utils import _InverseDict, pretokenize_raw

_PRETOK = pretokenize_raw(_InverseDict({"<0x0A>": "\n"}))


def invert(t2i):
    """id -> token string (the last token of a duplicated id wins, like a dict inversion)."""
    return {i: t for t, i in t2i.items()}


def walk_raw(s, toks):
    """One RAW string and its token strings -> (byte ends, word indices)."""
    words = _PRETOK(s) if s else []
    atoms = [(a, wi) for wi, w in enumerate(words) for a in w]
    assert len(atoms) == len(s)
    ends, wids = [], []
    ai = pos = 0
    for tok in toks:
        assert tok and ai < len(atoms), (s[:40], tok)
        wids.append(atoms[ai][1])
        got = ""
        while len(got) < len(tok):
            assert ai < len(atoms), (s[:40], tok)
            got += atoms[ai][0]
            pos += len(s[ai].encode("utf-8", "surrogatepass"))   # atom ai is input code point ai
            ai += 1
        assert got == tok, (s[:40], tok, got)   # text[start:end], atomised, is the token
        ends.append(pos)
    assert ai == len(atoms), (s[:40], ai, len(atoms))
    return ends, wids


def walk_bytes(text, wstart, toks):
    """One PRESPLIT / ATOMS string (bytes), its word-start flags per byte (bool array) and its token
    strings -> (byte ends, word indices)."""
    nw = np.cumsum(wstart[1:]) if len(text) > 1 else np.zeros(0, np.int64)   # word starts in [1, p], at p - 1
    ends, wids = [], []
    pos = 0
    for tok in toks:
        b = tok.encode("utf-8", "surrogatepass")
        assert b and text[pos:pos + len(b)] == b, (text[:40], tok)
        wids.append(int(nw[pos - 1]) if pos else 0)
        pos += len(b)
        ends.append(pos)
    assert pos == len(text), (text[:40], pos)
    return ends, wids


def expected(t2i, form, text, offs, cut, ids, id_off, status):
    """(tok_end u32[n_tok], tok_word u32[n_tok], span_status i32[n]) for a CSR batch in ``form`` ("raw",
    "presplit", "atoms") and the ids / id_off / status its encode returned.  Strings with a non-zero
    status keep it and have no entries."""
    inv = invert(t2i)
    o = np.asarray(offs).astype(np.int64)
    io = np.asarray(id_off).astype(np.int64) - int(id_off[0])
    raw = bytes(np.asarray(text, dtype=np.uint8)[int(o[0]):int(o[-1])])
    cutb = None if cut is None else np.asarray(cut, dtype=np.uint8)[int(o[0]):int(o[-1])]
    o = o - o[0]
    flat = np.asarray(ids).tolist()
    n = len(o) - 1
    tok_end = np.zeros(int(io[-1]), dtype=np.uint32)
    tok_word = np.zeros(int(io[-1]), dtype=np.uint32)
    span_status = np.asarray(status, dtype=np.int32).copy()
    for s in range(n):
        if status[s] != 0:
            assert io[s] == io[s + 1]
            continue
        toks = [inv[i] for i in flat[io[s]:io[s + 1]]]
        b = raw[o[s]:o[s + 1]]
        if form == "raw":
            ends, wids = walk_raw(b.decode("utf-8", "surrogatepass"), toks)
        else:
            c = cutb[o[s]:o[s + 1]]
            ends, wids = walk_bytes(b, (c != 0) if form == "presplit" else ((c & 1) != 0), toks)
        tok_end[io[s]:io[s + 1]] = ends
        tok_word[io[s]:io[s + 1]] = wids
    return tok_end, tok_word, span_status
