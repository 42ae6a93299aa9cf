"""tests/decode_ref.py against recorded results (no GPU, no library): its SentencePiece rule reproduces
the SentencePiece tokenizer's own decode of every recorded llama-mode case, and decoding the recorded ids
of the corpus and BLOOM fixtures gives back the text -- with the one exception the round trip exists to
find.  These pin the rules the decode tables and kernels are tested against."""
import gzip
import json
import os

import pytest

import decode_ref
from conftest import GOLDEN, load_golden

RAW_FIXTURES = {"cfg1_toy1k.json.gz": 1000, "cfg2_llama32k.json.gz": 400, "cfg4_s2orc.json.gz": 40,
                "cfg5_arabic.json.gz": 300, "oov_llama32k.json.gz": 237, "edge_toy1k.json.gz": 18,
                "edge_llama32k.json.gz": 20}


def test_alphabet():
    a = decode_ref.bytelevel_alphabet()
    assert sorted(a.values()) == list(range(256))
    assert a[ord("A")] == ord("A") and a[0x120] == 0x20 and a[0x10A] == 0x0A and a[0x100] == 0 and a[0x143] == 0xAD
    assert decode_ref.piece("Ġhello".encode(), "bytelevel") == b" hello"
    assert decode_ref.piece("Ã©".encode(), "bytelevel") == "é".encode()
    assert decode_ref.piece("中".encode(), "bytelevel") == "中".encode()       # outside the alphabet: verbatim
    assert decode_ref.piece("▁a▁".encode(), "sp") == b" a " and decode_ref.piece(b"<0x0A>", "sp") == b"\n"
    assert decode_ref.piece(b"<0x0a>", "sp") == b"<0x0a>" and decode_ref.piece(b"x<0x0A>", "sp") == b"x<0x0A>"
    assert decode_ref.piece("▁a".encode(), "pieces") == "▁a".encode()


def test_sp_rule_is_sentencepiece_decode():
    from sp_llama import SPLlama
    tok = SPLlama()
    by_id = decode_ref.pieces_by_id(decode_ref.pairs_of(tok.get_vocab()), "sp", skip_ids=[tok.sp.bos_id()])
    cases = [c for c in load_golden("sp_llama_cases.json.gz")["cases"] if c["tokenizer"] == "sp"]
    assert len(cases) == 565
    n_ok = 0
    for c in cases:
        assert c["status"] == 0
        b, ok = decode_ref.decode_ids(by_id, c["ids"], strip=True)
        assert ok
        n_ok += b.decode("utf-8", "replace") == c["decoded"]
    assert n_ok == 565


def test_raw_fixtures_round_trip(vocabs):
    differing = []
    for name, want in RAW_FIXTURES.items():
        g = load_golden(name)
        by_id = decode_ref.pieces_by_id(decode_ref.pairs_of(vocabs[g["vocab"]]), "sp")
        cases = [c for c in g["cases"] if c.get("status") == 0]
        assert len(cases) == want, name
        for c in cases:
            v, d = decode_ref.roundtrip_one(by_id, c["ids"], c["text"].encode("utf-8", "surrogatepass"), strip=True)
            assert v in (decode_ref.RT_EQUAL, decode_ref.RT_DIFFERS)
            if v != decode_ref.RT_EQUAL:
                differing.append((name, c["text"], d))
    # the DP picks the byte-fallback piece <0x41>, which decodes to "A"
    assert differing == [("edge_llama32k.json.gz", "a<0x41>b", 1)]


@pytest.mark.parametrize("name,n", [("bloom_cases.json.gz", 300), ("bloom_big_cases.json.gz", 400)])
def test_bloom_fixtures_round_trip(name, n):
    import bloom_fixture
    if "big" in name:
        t2i = bloom_fixture.big_vocab()
    else:
        with gzip.open(os.path.join(GOLDEN, "bloom_synth_tokenizer.json.gz"), "rt", encoding="utf-8") as fh:
            t2i = {t: i for i, t in enumerate(json.load(fh)["model"]["vocab"])}
    by_id = decode_ref.pieces_by_id(decode_ref.pairs_of(t2i), "bytelevel")
    cases = [c for c in load_golden(name)["cases"] if c["error"] is None]
    assert len(cases) == n
    for c in cases:
        assert decode_ref.roundtrip_one(by_id, c["ids"], c["text"].encode("utf-8")) == (decode_ref.RT_EQUAL, None), c["text"]


def test_roundtrip_verdicts():
    by_id = {1: b"", 2: b" ab", 3: b"c", 4: b" "}
    rt = decode_ref.roundtrip_one
    assert rt(by_id, [1, 2, 3], b"abc", strip=True) == (0, None)
    assert rt(by_id, [1, 2, 3], b"abc") == (5, 0)
    assert rt(by_id, [2, 3], b"ab", strip=True) == (5, 2)        # the text is a prefix
    assert rt(by_id, [2], b"abc", strip=True) == (5, 2)          # the decode is a prefix
    assert rt(by_id, [2, 9, 3], b"abc", strip=True) == (4, None)
    assert rt(by_id, [2, 9, 3], b"xbc", strip=True) == (5, 0)    # found before the id without a piece
    assert rt(by_id, [2, 9], b"a", strip=True) == (5, 1)
    assert rt(by_id, [4, 4], b" ", strip=True) == (0, None) and rt(by_id, [], b"") == (0, None)
