"""``dp_tokenize.batch_compare(texts, words=True)`` of both adapters (packages/tokenizer_utils.py with
``device_pretokenize=True``): the improved words found on the device against the per-word counts of the plain call,
and their token strings against the ones sliced from ``dp_tokenize.batch_spans`` and from ``tokenizer.encode``."""
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OLD_KEYS = ("dp_lengths", "default_lengths", "improved", "dp_word_counts", "default_word_counts")


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(a, b)


def _check_words(dp, tok, texts, dp_piece, default_piece):
    """-> (device-taken strings, improved words in all)"""
    plain = dp.batch_compare(texts)
    c = dp.batch_compare(texts, words=True)
    assert set(plain) == set(OLD_KEYS) and set(c) == set(OLD_KEYS) | {"improved_word_ids", "improved_tokens", "worse_tokens"}
    for key in OLD_KEYS:                                                     # every old key as without the keyword
        if key.endswith("word_counts"):
            assert len(c[key]) == len(plain[key]) and all(_same(x, y) for x, y in zip(c[key], plain[key])), key
        else:
            assert c[key].dtype == plain[key].dtype and np.array_equal(c[key], plain[key]), key
    spans = dp.batch_spans(texts)
    taken = n_words = 0
    for k, t in enumerate(texts):
        w = c["default_word_counts"][k]
        got = [c[key][k] for key in ("improved_word_ids", "improved_tokens", "worse_tokens")]
        if w is None:                                                        # the host tokenizer took it
            assert got == [None, None, None], t
            continue
        taken += 1
        want = np.flatnonzero(c["dp_word_counts"][k] < w).tolist()
        assert got[0] == want, (t, got[0], want)
        a_ids, a_words = np.asarray(spans[k].ids, dtype=np.int64), np.asarray(spans[k].word_ids, dtype=np.int64)
        b_ids = [int(i) for i in tok.encode(t)]
        b_end = np.cumsum(w).tolist()
        assert (b_end[-1] if b_end else 0) == len(b_ids)
        assert got[1] == [[dp_piece(int(i)) for i in a_ids[a_words == x]] for x in want], t
        assert got[2] == [[default_piece(i) for i in b_ids[b_end[x] - int(w[x]):b_end[x]]] for x in want], t
        assert all(isinstance(s, str) for word in got[1] + got[2] for s in word)
        assert all(len(a) < len(b) for a, b in zip(got[1], got[2]))
        if c["improved"][k]:                                                 # shorter in all: shorter in some word
            assert got[0], t
        n_words += len(want)
    assert c["improved"].any()
    return taken, n_words


@pytest.mark.parametrize("kind", ["sp", "hf"])
def test_llama_improved_words(kind):
    pytest.importorskip("sentencepiece")
    from packages.tokenizer_utils import dp_tokenize_llama
    from sp_llama import SPLlama, hf_llama, llama_texts
    tok = SPLlama() if kind == "sp" else hf_llama()
    dp, _ = dp_tokenize_llama(tok, "llama", device_pretokenize=True)
    assert dp.pretok_stats.default_off is None, dp.pretok_stats.default_off
    inverse = {i: t for t, i in tok.get_vocab().items()}
    texts = [t for t in llama_texts() if "\udc80" not in t][:200]
    taken, n_words = _check_words(dp, tok, texts, inverse.__getitem__, inverse.__getitem__)
    assert taken > 80 and n_words > 20
    empty = dp.batch_compare([], words=True)
    assert empty["improved_word_ids"] == [] and empty["improved_tokens"] == [] and empty["worse_tokens"] == []


@pytest.mark.parametrize("big", [False, True])
def test_bloom_improved_words(big):
    from bloom_fixture import big_vocab, bloom_big_texts, bloom_texts, bloom_tokenizer, make_hf_cache
    from packages.tokenizer_utils import dp_tokenize_bloom
    with tempfile.TemporaryDirectory() as d:
        hf = make_hf_cache(d, big=big)
        tok = bloom_tokenizer(hf)
        dp, _ = dp_tokenize_bloom(tok, hf, device_pretokenize=True)
    assert dp.pretok_stats.default_off is None, dp.pretok_stats.default_off
    texts = bloom_big_texts(big_vocab()) if big else bloom_texts()
    literal = next(iter(list(tok.get_added_vocab()) + list(tok.all_special_tokens)), None)
    if literal:
        texts = texts + ["a text with %s inside it" % literal, literal]     # an added-token literal: the host takes it
    texts = texts[:150]
    dp_inverse = {i: t for t, i in dp.vocab_to_index.items()}
    taken, n_words = _check_words(dp, tok, texts, dp_inverse.__getitem__, lambda i: tok.convert_ids_to_tokens([i])[0])
    assert taken >= 149 and n_words > 20
