"""Word-index streams for the word-compare tests (test_words_ref.py, test_gpu_words.py): streams from per-word
counts, the malformed variants, and batches of string pairs packed into sides in either layout."""
import numpy as np

import words_ref as wr

MALFORMED = ("first_is_1", "step_of_2", "decrease", "words_differ")


def stream_of(counts):
    """Per-word token counts -> the stream 0 0 1 2 2 2 ..."""
    counts = np.asarray(counts, dtype=np.int64)
    return np.repeat(np.arange(len(counts), dtype=np.int64), counts)


def split_counts(rng, n, words):
    """``words`` positive counts that sum to n (n >= words; both 0 gives none)."""
    if words == 0:
        assert n == 0
        return np.zeros(0, dtype=np.int64)
    assert n >= words
    cuts = np.sort(rng.choice(np.arange(1, n), size=words - 1, replace=False)) if words > 1 else np.zeros(0, dtype=np.int64)
    return np.diff(np.concatenate([[0], cuts, [n]])).astype(np.int64)


def malformed(kind, wa, wb, at):
    """The pair with one defect, ``at`` in [0, 1) placing it in side b's stream (side a's for words_differ)."""
    wa, wb = wa.copy(), wb.copy()
    if kind == "first_is_1":
        wb += 1
    elif kind == "step_of_2":
        k = min(max(1, int(at * len(wb))), len(wb) - 1)
        wb[k:] += 2 - (wb[k] - wb[k - 1])
    elif kind == "decrease":
        cand = np.flatnonzero(wb[:-1] >= 1) + 1          # the k with a value above 0 before them
        if len(cand) == 0:                               # (a one-word stream cannot go down: a step of 2 instead)
            wb[1:] += 2
        else:
            k = int(cand[min(int(at * len(cand)), len(cand) - 1)])
            wb[k:] -= wb[k] - wb[k - 1] + 1
    elif kind == "words_differ":
        wa = np.concatenate([wa, [wa[-1] + 1]])
    else:
        raise ValueError(kind)
    return wa, wb


def pack_side(streams, padded, status=None, off0=0, slack=None, ends=None, junk=0xDEAD):
    """Strings' streams -> a side (words_ref.make_side).  ``padded``: the layout of dpt_bpe_encode, string s's values in a
    slot of len + slack[s] entries with ``counts``; else CSR.  ``ends``: per string the tok_end values."""
    n = len(streams)
    lens = np.array([len(w) for w in streams], dtype=np.int64)
    room = lens + (np.asarray(slack, dtype=np.int64) if padded and slack is not None else 0)
    off = wr.offsets(room, off0)
    tok_word = np.full(int(room.sum()), junk, dtype=np.uint32)
    tok_end = np.full(int(room.sum()), junk, dtype=np.uint32) if ends is not None else None
    at = (off - off[0]).astype(np.int64)
    for s in range(n):
        tok_word[at[s]:at[s] + lens[s]] = np.asarray(streams[s], dtype=np.int64).astype(np.uint32)
        if ends is not None:
            tok_end[at[s]:at[s] + lens[s]] = ends[s]
    return wr.make_side(off, tok_word, counts=lens if padded else None, status=status, tok_end=tok_end)


def fake_ends(rng, w):
    """Strictly increasing byte ends for a stream's tokens."""
    return np.cumsum(rng.integers(1, 5, size=len(w))).astype(np.uint32)


def random_pairs(rng, n_pairs, max_tokens=40, p_bad=0.15):
    """-> (list of stream a, list of stream b, list of defect or None): pairs that share a word count, some with one
    defect, some empty."""
    sa, sb, kinds = [], [], []
    for _ in range(n_pairs):
        words = int(rng.integers(0, max_tokens // 2))
        na, nb = (int(rng.integers(words, max_tokens + 1)) if words else 0 for _ in range(2))
        wa, wb = stream_of(split_counts(rng, na, words)), stream_of(split_counts(rng, nb, words))
        kind = None
        if words and len(wb) >= 2 and rng.random() < p_bad:
            kind = MALFORMED[int(rng.integers(0, len(MALFORMED)))]
            wa, wb = malformed(kind, wa, wb, float(rng.random()))
            if rng.random() < 0.5 and kind != "words_differ":
                wa, wb = wb, wa
        sa.append(wa), sb.append(wb), kinds.append(kind)
    return sa, sb, kinds
