"""TEST INFRASTRUCTURE: the packing rule (include/dpt.h dpt_pack_sizes / dpt_pack_plan / dpt_pack_write) as plain
Python -- the model the tests compare the kernels with.  Written from the rule's text, not from the kernels:
``plan_loop`` is the header's loop, literally; ``rows_ref`` builds the rows from lists; ``plan_chain`` is the same
placement as a numpy ``searchsorted`` chain over the prefix sums, for sizes the loop is too slow at."""
import numpy as np

from collate_ref import BOS, EOS, TRUNC_LEFT, wrap

MASK_FIRST = 256
NONE = 0xFFFFFFFF


def random_lengths(rng, n, L):
    """lengths in [0, L] with zero runs and exact fills"""
    ln = rng.integers(0, L + 1, size=n)
    for _ in range(int(rng.integers(0, 4))):
        if n:
            a = int(rng.integers(0, n))
            ln[a:a + int(rng.integers(1, 8))] = 0
    if n >= 2 and rng.random() < 0.5:   # an exact fill: two neighbours that sum to L
        a = int(rng.integers(0, n - 1))
        ln[a] = int(rng.integers(0, L + 1))
        ln[a + 1] = L - ln[a]
    return ln


def lengths_ref(off, counts=None, status=None, *, row_len, flags=0):
    """len[s]: 0 for a failed string, else min(n, L - n_special) + n_special"""
    n_special = (1 if flags & BOS else 0) + (1 if flags & EOS else 0)
    out = []
    for s in range(len(off) - 1):
        n = int(off[s + 1] - off[s]) if counts is None else int(counts[s])
        out.append(0 if status is not None and status[s] != 0 else min(n, row_len - n_special) + n_special)
    return out


def plan_loop(lengths, L, row_cap=None):
    """-> (str_row, str_col, row_first, row_fill, n_rows); row_first of row_cap + 1 and row_fill of row_cap entries
    (row_cap None: n_rows), holding the rows below row_cap and the empty values from n_rows on."""
    n_str = len(lengths)
    str_row, str_col = [NONE] * n_str, [0] * n_str
    firsts, fills = [], []
    r, fill = -1, L + 1
    for s in range(n_str):
        if lengths[s] <= 0:
            continue
        if fill + lengths[s] > L:
            r += 1
            fill = 0
            firsts.append(s)
            fills.append(0)
        str_row[s], str_col[s] = r, fill
        fill += lengths[s]
        fills[r] = fill
    n_rows = r + 1
    cap = n_rows if row_cap is None else row_cap
    row_first = (firsts + [n_str] * (cap + 1))[:cap + 1]
    row_fill = (fills + [0] * cap)[:cap]
    return str_row, str_col, row_first, row_fill, n_rows


def plan_chain(lengths, L):
    """The same placement from the prefix sums P alone: the next row start after start s is the smallest t > s with
    P[t+1] - P[s] > L, i.e. searchsorted(P, P[s] + L, 'right') - 1; the first start is searchsorted(P, P[0], 'right')
    - 1.  -> (str_row, str_col, row_first [n_rows], row_fill [n_rows], n_rows) as numpy arrays."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n_str = len(lengths)
    P = np.concatenate([[0], np.cumsum(lengths)])
    starts = []
    s = int(np.searchsorted(P, P[0], "right")) - 1
    while s < n_str:
        starts.append(s)
        s = int(np.searchsorted(P, P[s] + L, "right")) - 1
    starts = np.asarray(starts, dtype=np.int64)
    n_rows = len(starts)
    str_row = np.full(n_str, NONE, dtype=np.int64)
    str_col = np.zeros(n_str, dtype=np.int64)
    if n_rows:
        row_of = np.searchsorted(starts, np.arange(n_str), "right") - 1
        placed = (lengths > 0) & (row_of >= 0)
        str_row[placed] = row_of[placed]
        str_col[placed] = (P[:-1] - P[starts[np.maximum(row_of, 0)]])[placed]
        ends = np.concatenate([starts[1:], [n_str]])
        row_fill = P[ends] - P[starts]
    else:
        row_fill = np.zeros(0, dtype=np.int64)
    return str_row, str_col, starts, row_fill, n_rows


def rows_ref(ids, off, counts=None, status=None, *, row_len, row_cap=None, pad_id=0, bos_id=0, eos_id=0, ignore_id=-100, flags=0):
    """-> (input_ids, position_ids, segment_ids, labels): four lists of row_cap rows (None: n_rows) of ``row_len`` ints.
    ``ids`` is the flat id list that ``off[0]`` corresponds to."""
    L = row_len
    lengths = lengths_ref(off, counts, status, row_len=L, flags=flags)
    str_row, _, row_first, _, n_rows = plan_loop(lengths, L)
    cap = n_rows if row_cap is None else row_cap
    n_special = (1 if flags & BOS else 0) + (1 if flags & EOS else 0)
    pad, ign = wrap(pad_id), wrap(ignore_id)
    out = [[], [], [], []]
    for r in range(cap):
        row = [[], [], [], []]
        for s in range(row_first[r], row_first[r + 1]) if r < n_rows else ():   # (row_first[n_rows] = n_str)
            if str_row[s] != r:
                continue
            n = int(off[s + 1] - off[s]) if counts is None else int(counts[s])
            keep = lengths[s] - n_special
            first = int(off[s] - off[0]) + (n - keep if flags & TRUNC_LEFT else 0)
            seq = ([wrap(bos_id)] if flags & BOS else []) + [wrap(ids[first + k]) for k in range(keep)] + ([wrap(eos_id)] if flags & EOS else [])
            assert len(seq) == lengths[s]
            row[0] += seq
            row[1] += list(range(len(seq)))
            row[2] += [s - row_first[r] + 1] * len(seq)
            row[3] += [ign if (flags & MASK_FIRST) and k == 0 else v for k, v in enumerate(seq)]
        fill = L - len(row[0])
        assert fill >= 0
        for k, v in enumerate((pad, 0, 0, ign)):
            out[k].append(row[k] + [v] * fill)
    return tuple(out)
