"""A plain numpy / Python model of dpt_word_compare_sizes and dpt_word_compare_write, written from the rule in
include/dpt.h: per string the validity of the two word-index streams, the status, the lengths, the per-word counts
and the selected words' records.

A side is a dict ``{"off": uint64[n + 1], "counts": None or int[n], "status": None or int32[n], "tok_word":
uint32[], "tok_end": None or uint32[]}``; string s's values are ``tok_word[off[s] - off[0]:][:n]`` with
``n = counts[s]`` when counts is given and ``off[s + 1] - off[s]`` otherwise."""
import numpy as np

LESS, GREATER = 1, 2
INTERNAL = 4
SEL_FIELDS = ("sel_str", "sel_word", "sel_begin", "sel_end", "sel_a_first", "sel_a_count", "sel_b_first", "sel_b_count")


def make_side(off, tok_word, counts=None, status=None, tok_end=None):
    return {"off": np.asarray(off, dtype=np.uint64), "counts": None if counts is None else np.asarray(counts, dtype=np.uint64),
            "status": None if status is None else np.asarray(status, dtype=np.int32),
            "tok_word": np.asarray(tok_word, dtype=np.uint32), "tok_end": None if tok_end is None else np.asarray(tok_end, dtype=np.uint32)}


def n_strings(side):
    return len(side["off"]) - 1


def stream(side, s, field="tok_word"):
    """The values of string s (int64), whatever its status."""
    at = int(side["off"][s]) - int(side["off"][0])
    n = int(side["counts"][s]) if side["counts"] is not None else int(side["off"][s + 1]) - int(side["off"][s])
    return side[field][at:at + n].astype(np.int64)


def runs(w):
    """A stream's (well-formed, word count, per-word counts, per-word first token index)."""
    w = np.asarray(w, dtype=np.int64)
    none = np.zeros(0, dtype=np.int64)
    if len(w) == 0:
        return True, 0, none, none
    steps = np.diff(w)
    if w[0] != 0 or ((steps != 0) & (steps != 1)).any():
        return False, 0, none, none
    first = np.flatnonzero(np.concatenate([[True], steps == 1]))
    return True, int(w[-1]) + 1, np.diff(np.concatenate([first, [len(w)]])), first


def selects(flags, ca, cb):
    out = np.zeros(len(ca), dtype=bool)
    if flags & LESS:
        out |= ca < cb
    if flags & GREATER:
        out |= ca > cb
    return out


def _status(a, b, s):
    sa = 0 if a["status"] is None else int(a["status"][s])
    sb = 0 if b["status"] is None else int(b["status"][s])
    return sa, sb


def string(a, b, s, flags):
    """One string: (wc_status, len_a, len_b, cnt_a, cnt_b, first_a, first_b, selected word indices)."""
    none = np.zeros(0, dtype=np.int64)
    sa, sb = _status(a, b, s)
    la = len(stream(a, s)) if sa == 0 else 0
    lb = len(stream(b, s)) if sb == 0 else 0
    if sa or sb:
        return (sa or sb), la, lb, none, none, none, none, none
    oka, wa, ca, fa = runs(stream(a, s))
    okb, wb, cb, fb = runs(stream(b, s))
    if not (oka and okb and wa == wb):
        return INTERNAL, la, lb, none, none, none, none, none
    return 0, la, lb, ca, cb, fa, fb, np.flatnonzero(selects(flags, ca, cb))


def sizes(a, b, flags):
    """-> {"n_words", "n_sel", "len_a", "len_b": uint32[n], "wc_status": int32[n]}"""
    assert flags in (1, 2, 3)
    n = n_strings(a)
    out = {k: np.zeros(n, dtype=np.uint32) for k in ("n_words", "n_sel", "len_a", "len_b")}
    out["wc_status"] = np.zeros(n, dtype=np.int32)
    for s in range(n):
        st, la, lb, ca, _, _, _, sel = string(a, b, s, flags)
        out["wc_status"][s], out["len_a"][s], out["len_b"][s] = st, la, lb
        out["n_words"][s], out["n_sel"][s] = len(ca), len(sel)
    return out


def offsets(counts, start=0):
    off = np.full(len(counts) + 1, start, dtype=np.uint64)
    off[1:] += np.cumsum(np.asarray(counts, dtype=np.uint64), dtype=np.uint64)
    return off


def write(a, b, flags, word_off=None, sel_off=None, fill=0xA5A5A5A5):
    """-> {"wc_status", "cnt_a", "cnt_b", the SEL_FIELDS, "word_keep", "sel_keep"}.  The per-word arrays have
    word_off[n] - word_off[0] entries and the per-selected-word arrays sel_off[n] - sel_off[0] (None without the
    offsets; sel_begin / sel_end None without a's tok_end).  Entries nothing is written to hold ``fill``: the ranges of
    the strings whose status is a side's.  ``word_keep`` / ``sel_keep`` are False on the ranges whose contents are
    unspecified: those of a string that has status 4."""
    assert flags in (1, 2, 3)
    n = n_strings(a)
    out = {"wc_status": np.zeros(n, dtype=np.int32)}
    for k in ("cnt_a", "cnt_b") + SEL_FIELDS:
        out[k] = None
    if word_off is not None:
        wo = np.asarray(word_off, dtype=np.uint64).astype(np.int64) - int(word_off[0])
        out["cnt_a"], out["cnt_b"] = (np.full(int(wo[-1]), fill, dtype=np.uint32) for _ in range(2))
        out["word_keep"] = np.ones(int(wo[-1]), dtype=bool)
    if sel_off is not None:
        so = np.asarray(sel_off, dtype=np.uint64).astype(np.int64) - int(sel_off[0])
        for k in SEL_FIELDS:
            if a["tok_end"] is not None or k not in ("sel_begin", "sel_end"):
                out[k] = np.full(int(so[-1]), fill, dtype=np.uint32)
        out["sel_keep"] = np.ones(int(so[-1]), dtype=bool)
    for s in range(n):
        st, _, _, ca, cb, fa, fb, sel = string(a, b, s, flags)
        if st == 0 and word_off is not None and wo[s + 1] - wo[s] != len(ca):
            st = INTERNAL
        if st == 0 and sel_off is not None and so[s + 1] - so[s] != len(sel):
            st = INTERNAL
        out["wc_status"][s] = st
        if st == INTERNAL and _status(a, b, s) == (0, 0):
            if word_off is not None:
                out["word_keep"][wo[s]:wo[s + 1]] = False
            if sel_off is not None:
                out["sel_keep"][so[s]:so[s + 1]] = False
        if st != 0:
            continue
        if word_off is not None:
            out["cnt_a"][wo[s]:wo[s + 1]], out["cnt_b"][wo[s]:wo[s + 1]] = ca, cb
        if sel_off is not None:
            r = slice(so[s], so[s + 1])
            out["sel_str"][r], out["sel_word"][r] = s, sel
            out["sel_a_first"][r], out["sel_a_count"][r] = fa[sel], ca[sel]
            out["sel_b_first"][r], out["sel_b_count"][r] = fb[sel], cb[sel]
            if a["tok_end"] is not None:
                ends = stream(a, s, "tok_end")
                out["sel_begin"][r] = [ends[fa[w] - 1] if w else 0 for w in sel]
                out["sel_end"][r] = [ends[fa[w] + ca[w] - 1] for w in sel]
    return out


def compare(a, b, flags):
    """sizes, the two prefix sums, write: what a caller gets who follows the two calls through."""
    sz = sizes(a, b, flags)
    out = write(a, b, flags, offsets(sz["n_words"]), offsets(sz["n_sel"]))
    out.update(sz, word_off=offsets(sz["n_words"]), sel_off=offsets(sz["n_sel"]))
    return out
