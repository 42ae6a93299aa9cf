"""The default-encoding rule's Python model (tests/bpe_ref.py) against the real tokenizers: ``sentencepiece`` and both
tokenizer objects on the certified llama texts, ``tokenizers`` on both BLOOM text sets; and the two routes to the llama
pair table.  No GPU: the model is what the kernel is compared with."""
import json
import tempfile

import pytest

import bpe_ref
import bytelevel_ref as br
import pretok_ref as pr

LITERALS = [b"<unk>", b"<s>", b"</s>"]


@pytest.fixture(scope="module")
def llama():
    pytest.importorskip("sentencepiece")
    from dptok.bpe import pairs_from_scores
    from sp_llama import SPLlama
    tok = SPLlama()
    sp, t2i = tok.sp, tok.get_vocab()
    n = sp.get_piece_size()
    exclude = [i for i in range(n) if sp.is_control(i) or sp.is_unknown(i) or sp.is_unused(i) or sp.is_byte(i)]
    pairs = pairs_from_scores(t2i, {sp.id_to_piece(i): sp.get_score(i) for i in range(n)}, exclude)
    table = pr.build_table(pr.vocab_pieces(t2i), b"<s>", LITERALS)
    return tok, t2i, pairs, table


def llama_certified(table):
    from sp_llama import llama_texts
    out = []
    for t in llama_texts():
        st, text2, cut = bpe_ref.atoms_one(table, t.encode("utf-8", "surrogatepass"))
        if st == 0:
            out.append((t, text2, cut))
    return out


def test_llama_model_equals_sentencepiece_and_hf(llama):
    from sp_llama import hf_llama
    tok, t2i, pairs, table = llama
    hf = hf_llama()
    merges, pid = bpe_ref.table_of(*pairs), bpe_ref.piece_ids(t2i)
    texts = llama_certified(table)
    assert len(texts) == 292
    for t, text2, cut in texts:
        st, ids, words = bpe_ref.encode_one(pid, merges, text2, cut)
        assert st == 0 and ids == tok.encode(t) == list(hf.encode(t)), t
        assert words == sorted(words) and len(words) == len(ids) and (not words or words[0] == 0)
    # a literal "<0x41>" is six atoms, the byte-fallback piece one
    ascii_table = pr.table_from(set(range(0x20, 0x7F)), True, b"<s>", LITERALS)
    st, text2, cut = bpe_ref.atoms_one(ascii_table, "<0x41>\n".encode())
    assert text2 == "<s>▁<0x41><0x0A>".encode() and list(cut) == [3, 0, 0, 3, 0, 0] + [2] * 6 + [2, 0, 0, 0, 0, 0]
    # and both slow and fast merges agree
    for t, text2, cut in texts[:80]:
        assert bpe_ref.encode_one(pid, merges, text2, cut, fast=True) == bpe_ref.encode_one(pid, merges, text2, cut)


def test_llama_table_routes_agree(llama):
    from dptok.bpe import pairs_from_tokenizer_json
    from sp_llama import hf_llama
    _, _, pairs, _ = llama
    a = bpe_ref.table_of(*pairs)
    b = bpe_ref.table_of(*pairs_from_tokenizer_json(hf_llama().backend_tokenizer.to_str()))
    assert len(a) == len(b) == 68229 and set(a) == set(b)
    assert {k: v[1] for k, v in a.items()} == {k: v[1] for k, v in b.items()}
    # the ranks differ as numbers (piece order against merge order) but order the pairs of any word alike: the same
    # merged piece at the same dense position
    ra, rb = sorted(set(v[0] for v in a.values())), sorted(set(v[0] for v in b.values()))
    da, db = {r: k for k, r in enumerate(ra)}, {r: k for k, r in enumerate(rb)}
    by_piece_a, by_piece_b = {}, {}
    for k, v in a.items():
        by_piece_a.setdefault(v[1], set()).add(da[v[0]])
    for k, v in b.items():
        by_piece_b.setdefault(v[1], set()).add(db[v[0]])
    assert all(len(s) == 1 for s in by_piece_a.values())                     # one rank per merged piece (route a)
    order_a = sorted(by_piece_a, key=lambda p: min(by_piece_a[p]))
    order_b = sorted(by_piece_b, key=lambda p: min(by_piece_b[p]))
    assert order_a == order_b


@pytest.mark.parametrize("big", [False, True])
def test_bloom_model_equals_tokenizers(big):
    from bloom_fixture import SNAPSHOT, big_vocab, bloom_big_texts, bloom_texts, bloom_tokenizer, make_hf_cache
    from dptok.bpe import pairs_from_tokenizer_json
    import os
    with tempfile.TemporaryDirectory() as d:
        hf = make_hf_cache(d, big=big)
        tok = bloom_tokenizer(hf)
        with open(os.path.join(hf, SNAPSHOT, "tokenizer.json"), encoding="utf-8") as fh:
            doc = fh.read()
    pairs = pairs_from_tokenizer_json(doc)
    vocab = json.loads(doc)["model"]["vocab"]
    assert len(pairs[0]) == (250420 if big else len(json.loads(doc)["model"]["merges"]))
    merges, pid = bpe_ref.table_of(*pairs), bpe_ref.piece_ids(vocab)
    texts = bloom_big_texts(big_vocab()) if big else bloom_texts()
    assert len(texts) == (400 if big else 300)
    table = br.build_table(br.BLOOM_SEPARATORS)
    longest = 0
    for t in texts:
        st, text2, cut = br.split_one(table, t.encode("utf-8"))
        got = bpe_ref.encode_one(pid, merges, text2, cut)
        assert st == 0 and got[0] == 0 and got[1] == list(tok.encode(t)), t
        longest = max([longest] + [len(w) for w in br.words_of(text2, cut)])
    assert longest == 102 if big else longest > 10


def test_pairs_from_merges_forms_and_refusals():
    from dptok.bpe import pairs_from_merges
    vocab = {"a": 0, "b": 1, "ab": 2, "abb": 3}
    one = pairs_from_merges(vocab, ["a b", "ab b"])
    two = pairs_from_merges(vocab, [["a", "b"], ["ab", "b"]])
    assert [x.tolist() for x in one] == [x.tolist() for x in two] == [[0, 2], [1, 1], [2, 3], [0, 1]]
    for key, val in (("ignore_merges", True), ("dropout", 0.1), ("continuing_subword_prefix", "##"), ("end_of_word_suffix", "</w>")):
        with pytest.raises(ValueError, match=key):
            pairs_from_merges(vocab, ["a b"], {key: val})
    pairs_from_merges(vocab, ["a b"], {"ignore_merges": False, "dropout": None, "continuing_subword_prefix": "", "end_of_word_suffix": None})
    with pytest.raises(ValueError):
        pairs_from_merges(vocab, ["a c"])


def test_rule_is_one_merge_at_a_time():
    p, q, r, s, P, Q, R = range(7)
    t = bpe_ref.table_of([p, P, r], [q, r, s], [P, Q, R], [0, 1, 2])
    assert bpe_ref.merge_word([p, q, r, s], t) == bpe_ref.merge_word_fast([p, q, r, s], t) == [Q, s]
    a, aa = 0, 1
    t = bpe_ref.table_of([a, aa], [a, aa], [aa, 2], [0, 1])
    assert [bpe_ref.merge_word([a] * n, t) for n in range(1, 6)] == [[0], [1], [1, 0], [2], [2, 0]]
