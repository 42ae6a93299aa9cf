"""The byte-level (BLOOM) pre-tokenization rule of tests/bytelevel_ref.py against what the `tokenizers` library
recorded (tests/golden/bloom_pretok_cases.json.gz, made by tests/golden/make_bloom_pretok.py): the separator set, the
words of every recorded text, and the ATOMS buffers ``pack_word_atoms`` builds from those words on the host path.
No GPU."""
import pytest

from conftest import load_golden

import bytelevel_ref as br


@pytest.fixture(scope="module")
def golden():
    return load_golden("bloom_pretok_cases.json.gz")


def test_separator_set(golden):
    from dptok.bytelevel import BLOOM_SEPARATORS, bytes_to_unicode
    assert len(golden["separators"]) == 39 and golden["separators"] == sorted(golden["separators"])
    assert list(BLOOM_SEPARATORS) == golden["separators"] == sorted(br.BLOOM_SEPARATORS)
    assert ord("[") not in BLOOM_SEPARATORS and ord("]") not in BLOOM_SEPARATORS and ord("|") in BLOOM_SEPARATORS
    assert [bytes_to_unicode()[b] for b in range(256)] == br.ALPHABET
    assert br.ALPHABET[0x20] == "Ġ" and br.ALPHABET[0x0A] == "Ċ" and br.ALPHABET[0xAD] == "Ń" and br.ALPHABET[0x41] == "A"
    assert len(set(br.ALPHABET)) == 256 and all(len(a) == (1 if 0x21 <= b <= 0x7E else 2) for b, a in enumerate(br.ATOM))


def test_model_gives_the_recorded_words(golden):
    table = br.build_table(golden["separators"])
    cases = golden["cases"]
    assert len(cases) == golden["n_fixture"] + golden["n_big"] + golden["n_random"] >= 1000
    for c in cases:
        assert br.words_of_text(table, c["text"]) == c["words"], c["text"]
    from bloom_fixture import bloom_texts
    assert [c["text"] for c in cases[:300]] == bloom_texts()
    assert sum(1 for c in cases if "  " in c["text"]) > 50 and sum(1 for c in cases if "。" in c["text"]) > 20


def test_model_equals_pack_word_atoms(golden):
    """Byte for byte what today's host path hands the engine: pack_word_atoms of the recorded words' characters."""
    import numpy as np
    from dptok.pack import pack_word_atoms
    table = br.build_table(golden["separators"])
    cases = golden["cases"]
    text, offs, cut = pack_word_atoms([[list(w) for w in c["words"]] for c in cases])
    st, ln, text2, cut2 = br.split(table, [c["text"].encode("utf-8") for c in cases])
    assert not st.any()
    assert np.array_equal(np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64), offs)
    assert text2 == text.tobytes()[:-1] and cut2 == cut.tobytes()[:-1]
    assert set(cut2) == {0, 2, 3}
    words = br.words_of(*br.split_one(table, "a  b。c".encode())[1:])
    assert words == [["a"], ["Ġ"], ["Ġ", "b"], list("ãĢĤ"), ["c"]]


def test_small_examples():
    table = br.build_table(br.BLOOM_SEPARATORS)
    w = lambda t: br.words_of_text(table, t)   # noqa: E731
    assert w("") == [] and w(" ") == ["Ġ"] and w("a  b") == ["a", "Ġ", "Ġb"] and w("hi...") == ["hi", "..."]
    assert w(" a") == ["Ġa"] and w("a ") == ["a", "Ġ"] and w("a, b") == ["a", ",", "Ġb"] and w("[a]") == ["[a]"]
    assert w("a \n b") == ["a", "ĠĊ", "Ġb"] and w("x(y)") == ["x", "(", "y", ")"]
    for bad in (b"\xc3", b"a\xe2\x82", b"\xc0\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\x80", b"\xe0\x80\xaf"):
        assert br.split_one(table, bad) == (br.NEEDS_HOST, b"", b"")
    assert br.split_one(table, b"") == (0, b"", b"")


def test_live_sweep_agrees(golden):
    """The installed `tokenizers` still answers as recorded on the blocks that hold every separator."""
    tokenizers = pytest.importorskip("tokenizers")
    import gzip
    import os
    from conftest import GOLDEN
    with gzip.open(os.path.join(GOLDEN, "bloom_synth_tokenizer.json.gz"), "rb") as fh:
        pre = tokenizers.Tokenizer.from_str(fh.read().decode("utf-8")).pre_tokenizer
    swept = list(range(0x0000, 0x3100)) + list(range(0xFF00, 0xFFF0))
    live = [cp for cp in swept if len(pre.pre_tokenize_str("a" + chr(cp) + "a")) != 1]
    assert live == golden["separators"]
    table = br.build_table(golden["separators"])
    for c in golden["cases"][::7]:
        assert [x for x, _ in pre.pre_tokenize_str(c["text"])] == br.words_of_text(table, c["text"])
