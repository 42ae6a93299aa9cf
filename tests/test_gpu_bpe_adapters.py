"""``dp_tokenize.batch_default`` and ``dp_tokenize.batch_compare`` of both adapters (packages/tokenizer_utils.py with
``device_pretokenize=True``) against the tokenizer objects themselves: the default ids of every recorded text, the
lengths of both sides, the reference's own assert ``default >= dp``, and per-word counts that sum to the lengths."""
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _check_compare(dp, tok, texts):
    c = dp.batch_compare(texts)
    assert c["dp_lengths"].tolist() == [len(x) for x in dp.batch(texts)]
    assert c["default_lengths"].tolist() == [len(tok.encode(t)) for t in texts]
    assert (c["default_lengths"] >= c["dp_lengths"]).all()                   # main_biomed_translation.py:77
    assert c["improved"].tolist() == (c["dp_lengths"] < c["default_lengths"]).tolist() and c["improved"].any()
    on_device = 0
    for k in range(len(texts)):
        assert int(c["dp_word_counts"][k].sum()) == c["dp_lengths"][k]
        w = c["default_word_counts"][k]
        if w is not None:
            on_device += 1
            assert int(w.sum()) == c["default_lengths"][k] and len(w) == len(c["dp_word_counts"][k])
            assert (w >= c["dp_word_counts"][k]).all() or c["default_lengths"][k] >= c["dp_lengths"][k]
    return on_device


@pytest.mark.parametrize("kind", ["sp", "hf"])
def test_llama_batch_default_and_compare(kind):
    pytest.importorskip("sentencepiece")
    from packages.tokenizer_utils import dp_tokenize_llama
    from sp_llama import SPLlama, hf_llama, llama_texts
    tok = SPLlama() if kind == "sp" else hf_llama()
    dp, _ = dp_tokenize_llama(tok, "llama", device_pretokenize=True)
    assert dp.pretok_stats.default_off is None, dp.pretok_stats.default_off
    texts = llama_texts()
    assert len(texts) == 565
    assert dp.batch_default(texts) == [list(tok.encode(t)) for t in texts]
    assert dp.batch_default([]) == [] and dp.batch_default([""]) == [list(tok.encode(""))]
    sub = [t for t in texts if "\udc80" not in t][:200]
    assert _check_compare(dp, tok, sub) > 80
    off, _ = dp_tokenize_llama(tok, "llama")
    assert not hasattr(off, "batch_default") and not hasattr(off, "batch_compare")


@pytest.mark.parametrize("big", [False, True])
def test_bloom_batch_default_and_compare(big):
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
    assert dp.batch_default(texts) == [list(tok.encode(t)) for t in texts]
    assert _check_compare(dp, tok, texts[:150]) >= 149


def test_probe_gate_leaves_the_calls_off():
    """A tokenizer object whose encode is not the rule's: construction leaves both calls off and says why."""
    pytest.importorskip("sentencepiece")
    from packages.tokenizer_utils import dp_tokenize_llama
    from sp_llama import SPLlama

    class Odd(SPLlama):
        def encode(self, text):
            if text != "hello world":
                return super().encode(text)
            return [self.sp.bos_id()] + [self._vocab[ch] for ch in "▁hello▁world"]   # the same words, nothing merged

    dp, _ = dp_tokenize_llama(Odd(), "llama", device_pretokenize=True)
    assert not hasattr(dp, "batch_default") and not hasattr(dp, "batch_compare")
    assert "hello world" in dp.pretok_stats.default_off
