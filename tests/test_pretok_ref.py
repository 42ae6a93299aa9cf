"""The pre-tokenization rule's Python model (tests/pretok_ref.py) against the reference's own words over real
SentencePiece (tests/golden/sp_llama_cases.json.gz: two tokenizer objects, 565 texts each), and against
``synth.llama_words`` on ASCII corpora.  No GPU, no library: the model is what the kernels are compared with."""
import numpy as np
import pytest

from conftest import load_golden

import pretok_ref as pr

LITERALS = [b"<unk>", b"<s>", b"</s>"]   # the model's control pieces: what both tokenizer objects treat specially


@pytest.fixture(scope="module")
def sp_table():
    pytest.importorskip("sentencepiece")
    from sp_llama import SPLlama
    t = pr.build_table(pr.vocab_pieces(SPLlama().get_vocab()), b"<s>", LITERALS)
    assert isinstance(t, pr.Table)
    return t


@pytest.fixture(scope="module")
def cases():
    by = {}
    for c in load_golden("sp_llama_cases.json.gz")["cases"]:
        by.setdefault(c["tokenizer"], []).append(c)
    assert sorted(by) == ["hf", "sp"] and all(len(v) == 565 for v in by.values())
    assert [c["text"] for c in by["hf"]] == [c["text"] for c in by["sp"]]
    return by


def _bytes(text):
    return text.encode("utf-8", "surrogatepass")


@pytest.mark.parametrize("kind", ["hf", "sp"])
def test_certified_words_are_the_recorded_words(kind, cases, sp_table):
    certified = 0
    for c in cases[kind]:
        st, text2, cut = pr.presplit_one(sp_table, _bytes(c["text"]))
        if st != 0:
            assert (st, text2, cut) == (pr.NEEDS_HOST, b"", b"")
            continue
        certified += 1
        assert len(text2) == len(cut) and set(cut) <= {0, 1}
        assert pr.words_of(text2, cut) == c["words"], c["text"]
    print("certified %d of %d (%s)" % (certified, len(cases[kind]), kind))
    assert certified >= 290


def test_every_text_the_tokenizers_disagree_on_is_refused(cases, sp_table):
    differ = [a["text"] for a, b in zip(cases["hf"], cases["sp"]) if a["words"] != b["words"]]
    assert len(differ) > 200
    for t in differ:
        assert pr.presplit_one(sp_table, _bytes(t))[0] == pr.NEEDS_HOST, t


def test_certified_cover_the_rule_edge_classes(cases, sp_table):
    ok = [c["text"] for c in cases["sp"] if pr.presplit_one(sp_table, _bytes(c["text"]))[0] == 0]
    assert sum(any(ord(ch) > 127 for ch in t) for t in ok) > 100            # non-ASCII
    assert sum("  " in t for t in ok) > 50                                   # runs of spaces (runs_ok)
    assert sum(b"<0x" in pr.presplit_one(sp_table, _bytes(t))[1] for t in ok) > 100   # byte fallback
    assert sp_table.runs_ok and "" in ok


@pytest.mark.parametrize("n,length,seed", [(64, 256, 1), (200, 37, 9), (16, 1, 3)])
def test_ascii_corpora_equal_llama_words(n, length, seed):
    from dptok import synth
    text, offs = synth.random_ascii_corpus(n, length, seed=seed)
    assert (text[offs[:-1].astype(np.int64)] != 0x20).all()                  # no string starts with a space
    t = pr.table_from(set(range(0x20, 0x7F)), True, b"<s>", LITERALS)
    raw = text.tobytes()
    strings = [raw[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]
    strings = [s for s in strings if b"<s>" not in s and b"</s>" not in s and b"<unk>" not in s]
    assert len(strings) >= n - 2
    st, ln, text2, cut = pr.presplit(t, strings + [b"ab\ncd e", b"x"])
    want = synth.llama_words(*synth._pack(strings + [b"ab\ncd e", b"x"]))
    assert not st.any()
    assert text2 == want[0].tobytes() and cut == want[2].tobytes()
    assert np.concatenate([[0], np.cumsum(ln)]).tolist() == want[1].tolist()


def test_refusals_and_empty_outputs():
    t = pr.table_from({ord("a"), ord("b"), 0xE9}, False, b"<s>", [b"<s>"])
    R = (pr.NEEDS_HOST, b"", b"")
    assert pr.presplit_one(t, b"") == (0, b"<s>", b"\x01\0\0")
    assert pr.presplit_one(t._replace(bos=b""), b"") == (0, b"", b"")
    assert pr.presplit_one(t._replace(bos=b""), b"a") == (0, pr.WS + b"a", b"\x01\0\0\0")
    assert pr.words_of("<s>▁a▁é".encode(), bytes([1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0])) == ["<s>", "▁a", "▁é"]
    assert pr.presplit_one(t, "a é\n".encode()) == (0, "<s>▁a▁é<0x0A>".encode(), bytes([1, 0, 0, 1, 0, 0, 0, 1, 0, 0] + [0] * 8))
    assert pr.presplit_one(t, "ü".encode())[1] == "<s>▁<0xC3><0xBC>".encode()
    for s in (b" a", "a▁".encode(), b"a<s>", b"a  b", b"a\xc3", b"\xc0\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\x80a",
              b"\xe2\x82", b"\xf0\x9f\x98"):
        assert pr.presplit_one(t, s) == R, s
    assert pr.presplit_one(t._replace(runs_ok=True), b"a  b")[0] == 0
    assert pr.presplit_one(t, b"a<s")[0] == 0                                # a literal's proper prefix
