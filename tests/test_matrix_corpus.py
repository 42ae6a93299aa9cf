"""The dispatch-matrix corpus (tests/matrix_corpus.py) deserves its name: with the C oracle alone, for
each of the four vocabularies and the three forms, it has enough strings that tokenize, enough that do
not, long-token ids, multi-byte-token ids, and words for each of the passes after the first."""
import numpy as np
import pytest

import matrix_corpus as mc


@pytest.fixture(scope="module")
def oracles():
    from oracle import oracle
    return {k: oracle.OracleVocab(v) for k, v in mc.vocabularies().items()}


def test_vocabularies_have_the_shapes_the_dispatch_needs():
    v = mc.vocabularies()
    assert tuple(v) == mc.VOCAB_NAMES
    for name, t2i in v.items():
        max_cp = max(len(t) for t in t2i)
        assert (17 <= max_cp <= 64) if name.startswith("long") else max_cp <= 16, (name, max_cp)
        assert (min(t2i.values()) >= mc.ID_SHIFT) if name.endswith("+40000") else max(t2i.values()) <= 32767
        assert all(t in t2i for t in mc.MULTIBYTE)
    assert len(mc.long_token_list()) == 120


def test_corpus_size_and_forms_agree():
    strings = mc.corpus()
    assert 400 <= len(strings) <= 500
    n_bytes = {f: int(mc.form(f)[1][-1]) for f in mc.FORMS}
    assert 100_000 <= n_bytes["raw"] <= 400_000, n_bytes
    for f in mc.FORMS:
        text, offs, cut = mc.form(f)
        assert len(offs) == len(strings) + 1 and len(text) == int(offs[-1])
        assert (cut is None) == (f == "raw") and (cut is None or len(cut) == len(text))
    # the ATOMS form: merged atoms of 2..12 bytes on both sides of the windowed kernels' 8-byte limit
    text, offs, cut = mc.form("atoms")
    starts = np.flatnonzero(cut & 2)
    alen = np.diff(np.append(starts, len(text)))
    sid = np.searchsorted(offs.astype(np.int64), starts, side="right") - 1
    multi_cp = np.array([len(text[a:a + n].tobytes().decode("utf-8")) > 1 and text[a] != ord("<")
                         for a, n in zip(starts, alen)])
    assert set(sid[multi_cp] % 10) == {0}
    assert alen[multi_cp].min() >= 2 and alen[multi_cp].max() <= 12
    assert (alen[multi_cp] <= 8).sum() >= 20 and (alen[multi_cp] > 8).sum() >= 3


@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("vocab", mc.VOCAB_NAMES)
def test_corpus_conditions(vocab, form, oracles):
    t2i = mc.vocabularies()[vocab]
    text, offs, cut = mc.form(form)
    ids, id_off, st, capped = oracles[vocab].encode_csr(text, offs, mode=mc.oracle_mode(form), cut_mask=cut)
    n = len(st)
    n_long = int(np.isin(ids, list(mc.long_ids(t2i))).sum())
    n_multi = int(np.isin(ids, list(mc.multibyte_ids(t2i))).sum())
    longest = mc.longest_words(form, text, offs, cut)
    per_pass = {k: int(((st == 0) & (longest > a) & (longest <= b)).sum()) for k, (a, b) in mc.PASSES.items()}
    print(vocab, form, "status 0/1/2:", [int((st == k).sum()) for k in range(3)], "long-token ids:", n_long,
          "multi-byte-token ids:", n_multi, "words per pass:", per_pass)
    assert set(np.unique(st)) <= {0, 1, 2}
    assert (st == 0).sum() >= 0.8 * n
    assert (st == 1).sum() >= 5
    if form == "raw":
        assert (st == 2).sum() >= 2
    if vocab.startswith("long") and form != "raw":
        assert n_long >= 200
    assert n_multi >= 20
    for k, c in per_pass.items():
        assert c >= 4, (k, c)
    # an atom over 8 bytes that is a token: the unbounded pass emits an id for it
    if form == "atoms":
        i9 = t2i["文😀é"]
        assert (ids == i9).sum() >= 1


@pytest.mark.parametrize("form", mc.FORMS)
def test_shards_cover_the_corpus_unaligned_with_words_for_every_pass(form):
    text, offs, cut = mc.upload(form)
    ftext, foffs, fcut = mc.form(form)
    sh = mc.shards(form)
    n = len(offs) - 1
    assert len(sh) >= 3 and sh[0][0] == 0 and sh[-1][1] == n
    assert all(sh[k][1] == sh[k + 1][0] for k in range(len(sh) - 1))
    assert {int(offs[lo]) % 4 for lo, _ in sh} >= {1, 2, 3}
    assert int(offs[0]) != 0 and int(offs[-1]) < len(text)
    assert np.array_equal(text[int(offs[0]):int(offs[-1])], ftext)
    longest = mc.longest_words(form, ftext, foffs, fcut)
    for lo, hi in sh:
        assert {mc.pass_of(int(x)) for x in longest[lo:hi]} >= {None, "mid", "big", "long"}, (lo, hi)
