"""words_ref (the numpy model of dpt_word_compare_sizes / dpt_word_compare_write) against a brute-force count: per
string a dictionary word -> tokens, filled token by token.  Hand-written cases and 2,000 seeded random pairs, the
malformed streams among them (no GPU needed)."""
import numpy as np
import pytest

import words_cases as wc
import words_ref as wr


def brute(wa, wb, sa, sb, flags, ends_a=None):
    """One string, token by token -> (status, n_words, selected records as tuples (word, begin, end, a_first, a_count,
    b_first, b_count), cnt_a, cnt_b)."""
    if sa or sb:
        return (sa or sb), 0, [], [], []
    sides = []
    for w in (wa, wb):
        count, first, ok = {}, {}, True
        for k, v in enumerate(int(x) for x in w):
            if k == 0 and v != 0:
                ok = False
            if k and v - int(w[k - 1]) not in (0, 1):
                ok = False
            count[v] = count.get(v, 0) + 1
            first.setdefault(v, k)
        sides.append((ok, count, first))
    (oka, ca, fa), (okb, cb, fb) = sides
    if not (oka and okb) or len(ca) != len(cb):
        return wr.INTERNAL, 0, [], [], []
    recs = []
    for w in range(len(ca)):
        if (flags & wr.LESS and ca[w] < cb[w]) or (flags & wr.GREATER and ca[w] > cb[w]):
            begin = end = None
            if ends_a is not None:
                begin, end = (int(ends_a[fa[w] - 1]) if w else 0), int(ends_a[fa[w] + ca[w] - 1])
            recs.append((w, begin, end, fa[w], ca[w], fb[w], cb[w]))
    return 0, len(ca), recs, [ca[w] for w in range(len(ca))], [cb[w] for w in range(len(cb))]


def check_batch(sa_streams, sb_streams, st_a, st_b, flags, pad_a, pad_b, rng, off0=0):
    n = len(sa_streams)
    ends = [wc.fake_ends(rng, w) for w in sa_streams]
    a = wc.pack_side(sa_streams, pad_a, status=st_a, off0=off0, slack=rng.integers(0, 4, size=n), ends=ends)
    b = wc.pack_side(sb_streams, pad_b, status=st_b, off0=3 * off0, slack=rng.integers(0, 4, size=n))
    got = wr.compare(a, b, flags)
    assert got["word_off"][-1] == got["n_words"].sum() and got["sel_off"][-1] == got["n_sel"].sum()
    assert got["word_keep"].all() and got["sel_keep"].all()                 # exact ranges: everything is specified
    wo, so = got["word_off"].astype(np.int64), got["sel_off"].astype(np.int64)
    for s in range(n):
        qa = 0 if st_a is None else int(st_a[s])
        qb = 0 if st_b is None else int(st_b[s])
        st, nw, recs, ca, cb = brute(sa_streams[s], sb_streams[s], qa, qb, flags, ends[s])
        assert got["wc_status"][s] == st, s
        assert got["len_a"][s] == (len(sa_streams[s]) if qa == 0 else 0) and got["len_b"][s] == (len(sb_streams[s]) if qb == 0 else 0)
        assert got["n_words"][s] == nw and got["n_sel"][s] == len(recs), s
        assert got["cnt_a"][wo[s]:wo[s + 1]].tolist() == ca and got["cnt_b"][wo[s]:wo[s + 1]].tolist() == cb, s
        r = slice(so[s], so[s + 1])
        assert (got["sel_str"][r] == s).all()
        fields = ("sel_word", "sel_begin", "sel_end", "sel_a_first", "sel_a_count", "sel_b_first", "sel_b_count")
        assert list(zip(*(got[f][r].tolist() for f in fields))) == recs, s
    return got


def test_hand_written_pair():
    rng = np.random.default_rng(0)
    wa, wb = [0, 0, 1, 2, 2, 2], [0, 1, 1, 1, 2]
    for flags, words in ((wr.LESS, [1]), (wr.GREATER, [0, 2]), (wr.LESS | wr.GREATER, [0, 1, 2])):
        got = check_batch([np.array(wa)], [np.array(wb)], None, None, flags, False, True, rng)
        assert got["sel_word"].tolist() == words and got["cnt_a"].tolist() == [2, 1, 3] and got["cnt_b"].tolist() == [1, 3, 1]
    got = check_batch([np.array(wa)], [np.array(wb)], None, None, wr.LESS, True, False, rng, off0=7)
    assert (got["sel_a_first"][0], got["sel_a_count"][0], got["sel_b_first"][0], got["sel_b_count"][0]) == (2, 1, 1, 3)


def test_hand_written_statuses_and_empties():
    rng = np.random.default_rng(1)
    e, one, two = np.zeros(0, np.int64), np.array([0]), np.array([0, 0])
    a = [e, e, one, two, two, two, one]
    b = [e, one, e, one, one, one, np.array([1])]
    st_a = np.array([0, 0, 0, 0, 6, 3, 0], dtype=np.int32)
    st_b = np.array([0, 0, 0, 0, 1, 0, 0], dtype=np.int32)
    got = check_batch(a, b, st_a, st_b, wr.GREATER, False, True, rng)
    assert got["wc_status"].tolist() == [0, 4, 4, 0, 6, 3, 4]
    assert got["n_words"].tolist() == [0, 0, 0, 1, 0, 0, 0] and got["n_sel"].tolist() == [0, 0, 0, 1, 0, 0, 0]
    assert got["len_a"].tolist() == [0, 0, 1, 2, 0, 0, 1] and got["len_b"].tolist() == [0, 1, 0, 1, 0, 1, 1]


@pytest.mark.parametrize("kind", wc.MALFORMED)
def test_each_defect_is_malformed(kind):
    wa, wb = wc.stream_of([2, 1, 3, 1]), wc.stream_of([1, 1, 1, 4])
    assert wr.runs(wa)[0] and wr.runs(wb)[0]
    for at in (0.0, 0.5, 0.99):
        xa, xb = wc.malformed(kind, wa, wb, at)
        oka, na = wr.runs(xa)[:2]
        okb, nb = wr.runs(xb)[:2]
        assert not (oka and okb and na == nb), (kind, at)
        if kind != "words_differ":
            assert not okb
    if kind == "decrease":
        assert (np.diff(wc.malformed(kind, wa, wb, 0.5)[1]) < 0).any()
    assert wr.runs(wc.malformed("decrease", wa, np.zeros(5, np.int64), 0.5)[1])[0] is False


def test_write_with_short_ranges():
    """A range one too short: status 4 for that string alone, its range unspecified, the others' exact."""
    wa, wb = wc.stream_of([2, 1, 3]), wc.stream_of([1, 3, 1])
    a, b = wc.pack_side([wa] * 3, False), wc.pack_side([wb] * 3, True)
    sz = wr.sizes(a, b, 3)
    assert sz["n_words"].tolist() == [3, 3, 3] and sz["n_sel"].tolist() == [3, 3, 3]
    for which in ("word", "sel"):
        counts = {"word": [3, 3, 3], "sel": [3, 3, 3]}
        counts[which][1] = 2
        got = wr.write(a, b, 3, wr.offsets(counts["word"], 5), wr.offsets(counts["sel"], 9))
        assert got["wc_status"].tolist() == [0, 4, 0]
        assert got["word_keep"].tolist() == [True] * 3 + [False] * counts["word"][1] + [True] * 3
        assert got["sel_keep"].tolist() == [True] * 3 + [False] * counts["sel"][1] + [True] * 3
        assert got["cnt_a"][got["word_keep"]].tolist() == [2, 1, 3] * 2 and got["sel_word"][got["sel_keep"]].tolist() == [0, 1, 2] * 2
        assert got["sel_str"][got["sel_keep"]].tolist() == [0, 0, 0, 2, 2, 2]


def test_random_pairs():
    rng = np.random.default_rng(20240521)
    n_pairs = n_bad = 0
    for round_ in range(100):
        sa, sb, kinds = wc.random_pairs(rng, 20)
        st_a = rng.choice(np.array([0, 0, 0, 0, 0, 0, 1, 6], dtype=np.int32), size=20) if round_ % 3 == 0 else None
        st_b = rng.choice(np.array([0, 0, 0, 0, 0, 0, 2, 4], dtype=np.int32), size=20) if round_ % 4 == 0 else None
        flags = (1, 2, 3)[round_ % 3]
        got = check_batch(sa, sb, st_a, st_b, flags, round_ % 2 == 0, round_ % 4 < 2, rng, off0=round_ % 5)
        n_pairs += len(sa)
        n_bad += int((got["wc_status"] == wr.INTERNAL).sum())
    assert n_pairs == 2000 and 150 < n_bad < 600
