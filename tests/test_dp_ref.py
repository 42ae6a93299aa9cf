"""tests/dp_ref.py, the reference tests/test_gpu_dp_edges.py compares the kernels with, pinned without a
GPU: its atomisation and capped DP against the C oracle, its masks and uncapped costs against
oracle/ref_port.py, and -- from the reference alone -- the conditions the GPU tests' inputs must meet, so
that none of them passes on an input that exercises nothing."""
import random

import numpy as np
import pytest

import dp_ref
import matrix_corpus as mc

BASE_VOCABS = ("base", "long")


def _popcount(a):
    a = a.copy()
    n = np.zeros(len(a), np.int64)
    while a.any():
        n += (a & np.uint64(1)).astype(np.int64)
        a >>= np.uint64(1)
    return n


@pytest.fixture(scope="module")
def oracles():
    from oracle import oracle
    return {k: oracle.OracleVocab(mc.vocabularies()[k]) for k in BASE_VOCABS}


@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("vocab", BASE_VOCABS)
def test_status_and_capped_lengths_equal_the_c_oracle(vocab, form, oracles):
    text, offs, cut = mc.form(form)
    _, _, st, capped = oracles[vocab].encode_csr(text, offs, mode=mc.oracle_mode(form), cut_mask=cut)
    r = dp_ref.corpus_ref(vocab, form)
    assert np.array_equal(r.status[0], st), np.flatnonzero(r.status[0] != st)[:10]
    assert np.array_equal(r.lengths[0], capped), np.flatnonzero(r.lengths[0] != capped)[:10]
    assert not r.far[0] and not r.far[1]


def test_raw_atomisation_is_ref_ports():
    from oracle import ref_port
    strings = mc.corpus()
    text, offs, _ = mc.form("raw")
    got = dp_ref.atomise(text, offs, None, dp_ref.RAW)
    for s, ws in zip(strings, got):
        assert [w for w, _ in ws] == ref_port.raw_words(s), s[:40]
        assert sum(nb for _, nb in ws) == len(s.encode("utf-8"))


def _sample_words():
    """(atoms, vocabulary) of 320 corpus words of at most 40 atoms, from every form and both base
    vocabularies, and the heads of 80 words of the cap-trap batch (unreachable ends, a binding cap)."""
    rnd = random.Random(3)
    out = []
    for vocab in BASE_VOCABS:
        toks = dp_ref.Voc(mc.vocabularies()[vocab])
        for form in mc.FORMS:
            ws = [w for s in dp_ref.corpus_ref(vocab, form).words for w, _ in s if 0 < len(w) <= 40]
            out += [(w, toks) for w in rnd.sample(ws, 54 if form != "atoms" else 52)]
    n_corpus = len(out)
    for form in ("raw", "atoms"):
        r = dp_ref.trap_ref(form, False)
        toks = dp_ref.Voc(dp_ref.trap_vocab(False))
        ws = [w[:40] for s in r.words for w, _ in s if w]     # any atom list is a word: the first 40 atoms
        out += [(w, toks) for w in rnd.sample(ws, 40)]
    return out, n_corpus


def _walk(atoms, w):
    """Every tokenization the masks of one word encode, the largest predecessor popped first
    (packages/dp_tokenize.py compute_shortest_tokenizations' walk)."""
    far = {}
    for i, d in w.far:
        far.setdefault(i - 1, []).append(d)
    masks = np.array(w.mask[1:], dtype=np.uint64)
    n = w.n
    stack = [(j, n, []) for j in dp_ref.preds_from_masks(masks, far, 0, n)]
    done = []
    while stack:
        j, i, partial = stack.pop()
        toks = ["".join(atoms[j:i])] + partial
        if j == 0:
            done.append(toks)
        else:
            for jj in dp_ref.preds_from_masks(masks, far, 0, j):
                stack.append((jj, j, list(toks)))
    return done


def test_masks_and_uncapped_costs_equal_ref_port():
    from oracle import ref_port
    words, n_corpus = _sample_words()
    assert n_corpus >= 300
    n_enum = n_multi = n_unreach = 0
    for atoms, voc in words:
        c, u = dp_ref.word_dp(atoms, voc)
        n = len(atoms)
        cost, preds = ref_port.forward_dp(atoms, voc.tokens)
        reach = [ref_port.min_tokens_for_string(atoms[:j], voc.tokens) != dp_ref.INF for j in range(n + 1)]
        assert cost == c.cost and reach == c.reach
        n_unreach += reach.count(False)
        for i in range(1, n + 1):
            want = sum(1 << (i - 1 - j) for j in preds[i] if reach[j])
            assert c.mask[i] == want, (atoms, i, hex(c.mask[i]), hex(want))
        assert ref_port.min_tokens_for_string(atoms, voc.tokens) == u.cost[n]
        lists, length = ref_port.enumerate_shortest(atoms, voc.tokens, limit=201)
        if len(lists) <= 200:
            assert _walk(atoms, c) == lists and length == c.cost[n], atoms
            assert bool(lists) == c.valid[n]
            n_enum += 1
            n_multi += len(lists) > 1
    print("words", len(words), "enumerated", n_enum, "with several tokenizations", n_multi, "unreachable ends", n_unreach)
    assert n_enum >= 300 and n_multi >= 50 and n_unreach >= 30


@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("vocab", BASE_VOCABS)
def test_corpus_exercises_the_edge_stores(vocab, form):
    """Per pass class (matrix_corpus.pass_of of the word's bytes) at least 1000 atom ends whose capped mask
    has two or more bits.  The reference counts, for `base` (None / mid / big / long): raw 16837 / 3348 /
    13311 / 15870, presplit 16058 / 2699 / 8634 / 22066, atoms 15920 / 2674 / 8622 / 22018; `long` has a
    few hundred fewer in the first class.  Strings whose first mask index is no multiple of 4: 306..333;
    words that start in a later 256-byte window of a string of several words: 122..161 strings; strings
    with an atom end whose index is not its byte end: 79 (raw), 428 (presplit), 426 (atoms)."""
    r = dp_ref.corpus_ref(vocab, form)
    text, offs, cut = mc.form(form)
    multi = r.is_end & (_popcount(r.edges[0]) >= 2)
    per = {c: int((multi & (r.end_pass == k)).sum()) for k, c in enumerate(dp_ref.PASS_CLASSES)}
    # the pass classes are matrix_corpus.pass_of's: per string, the longest word of both agree
    longest = mc.longest_words(form, text, offs, cut)
    mine = [max([nb for _, nb in ws] or [0]) for ws in r.words]
    assert [mc.pass_of(int(x)) for x in longest] == [dp_ref.pass_of(x) for x in mine]
    unaligned = int(((r.first_index % 4 != 0) & (r.n_atoms > 0)).sum())
    later = int(((r.later_window_atoms > 0) & (r.n_words > 1)).sum())
    print(vocab, form, "ends with >= 2 bits per pass", per, "unaligned first index", unaligned,
          "second-window words", later, "index != byte end", int(r.index_differs.sum()),
          "unreachable ends", int(r.end_unreach.sum()))
    for c, n in per.items():
        assert n >= 1000, (c, n)
    assert unaligned >= 50 and later >= 50 and r.index_differs.sum() >= 50


@pytest.mark.parametrize("lanes64", (False, True))
@pytest.mark.parametrize("form", ("raw", "atoms"))
def test_cap_trap_batch_conditions(form, lanes64):
    """Per pass class at least 20 ends whose capped and uncapped masks differ (the reference counts 58..64,
    of them 24..48 in strings of capped status 0), at least 20 unreachable ends (170..1671, of them 63..761
    in strings of capped status 0), and strings of status 1 capped and 0 uncapped (20 or 21 of 48)."""
    from oracle import oracle
    tokens, text, offs, cut = dp_ref.trap_batch(form, lanes64)
    r = dp_ref.trap_ref(form, lanes64)
    assert (max(len(t) for t in tokens) > 16) == lanes64 and max(len(t) for t in tokens) <= 64
    _, _, st, capped = oracle.OracleVocab({t: i for i, t in enumerate(tokens)}).encode_csr(
        text, offs, mode=dp_ref.MODE_OF[form], cut_mask=cut)
    assert np.array_equal(st, r.status[0]) and np.array_equal(capped, r.lengths[0])
    ok0 = r.is_end & (r.status[0][np.maximum(r.end_str, 0)] == 0)
    differ = r.is_end & (r.edges[0] != r.edges[1])
    rows = {}
    for k, c in enumerate(dp_ref.PASS_CLASSES):
        cls = r.end_pass == k
        rows[c] = (int((differ & cls).sum()), int((differ & cls & ok0).sum()), int((r.end_unreach & cls).sum()),
                   int((r.end_unreach & cls & ok0).sum()))
    flips = int(((r.status[0] == 1) & (r.status[1] == 0)).sum())
    print(form, lanes64, "per pass (masks differ, of them in status-0 strings, unreachable ends, of them in "
          "status-0 strings)", rows, "status 1 capped and 0 uncapped:", flips)
    for c, (d, d0, u, u0) in rows.items():
        assert d >= 20 and d0 >= 20 and u >= 20 and u0 >= 20, (c, d, d0, u, u0)
    assert flips >= 5
    assert ((r.status[0] == 1) & (r.status[1] == 1)).sum() >= 3 and (r.status[0] == 2).sum() == 1
    assert ((r.later_window_atoms > 0) & (r.n_words > 1)).sum() >= 20 and r.index_differs.sum() >= 20
    assert not r.far[0] and not r.far[1]


@pytest.mark.parametrize("form", ("raw", "atoms"))
def test_far_batch_conditions(form):
    r = dp_ref.far_ref(form)
    assert r.n_str >= 8 and (r.n_words >= 3).all() and (r.status[1] == 0).all()
    at_end = np.bincount([e for e, _ in r.far[0]])
    only_capped = sorted(set(r.far[0]) - set(r.far[1]))
    in_ok = [p for p in only_capped if r.status[0][r.end_str[p[0]]] == 0]
    print(form, "far pairs", len(r.far[0]), "uncapped", len(r.far[1]), "most at one end", int(at_end.max()),
          "capped only", len(only_capped), "of them in status-0 strings", len(in_ok),
          "strings of capped status 1:", int((r.status[0] == 1).sum()))
    assert len(r.far[0]) > 1024 and len(r.far[1]) > 1024     # Encoder.dp starts with room for 1024
    # where the cap binds, the far pairs of the two DPs differ too; some strings fail under the cap alone
    assert set(r.far[1]) <= set(r.far[0]) and len(in_ok) >= 10 and (r.status[0] == 1).sum() >= 3
    assert set(np.unique(r.status[0])) == {0, 1}
    assert at_end.max() >= 3 and min(d for _, d in r.far[0]) >= 64
    far_strings = {int(r.end_str[e]) for e, _ in r.far[0]}
    assert len(far_strings) >= 8 and r.n_str - len(far_strings) >= 5      # and strings without any
    assert far_strings == {int(r.end_str[e]) for e, _ in r.far[1]}
    # the far words sit behind other words: no far end in the first word of its string
    first_word = {s: len(r.words[s][0][0]) for s in far_strings}
    assert all(int(r.end_atom[e]) > first_word[int(r.end_str[e])] for e, _ in r.far[0])
