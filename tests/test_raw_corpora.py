"""tests/raw_corpora.py builds what tests/test_gpu_parity.py built inline before the builders moved there.  The digests
below were recorded from the commit before the move by calling its test functions themselves -- with stand-ins for
dptok.Encoder / dptok.Vocab / oracle.OracleVocab that hash every (text, offsets[, mask]) handed to encode_csr and
every vocabulary uploaded (``raw_corpora.corpus_digest`` / ``vocab_digest``) -- so the move changed no input.  No GPU."""
import hashlib

import pytest

import raw_corpora as rc

A0 = "5604722ecfc9544df1e2fd7fa2b50f1d0d6e32222ffae076357fcd6f63ab8b6d"
WALKER = {31: ("54f088f8002d3085ee1d5f8fd31d05c0e9227ecfdd17430ea3d2f965a0e65325",
               "01db974284bd88aa5b72a84b3f98a6eb54aecf6ab59d884e5d366851357ecc5a"),
          32: ("1995bdc6c6a82924a281bf7bb4f6f68e7f03f2ef8ee84271841691784b221031",
               "5393571e9aba7d32c2102535f7bb55f8cb9989fdd3f26b034b1a6fbfb3df5f8d")}
# tie-heavy: the first and the last case, and the SHA-256 over all the (vocabulary, corpus) hex digests in order
TIE_FIRST = ("822c0050401299fa282d7887fd85f3529126f27142a0a3cbb9cb7c59aba7401f",
             "daea96ca64888fe262e87b85bd0af7c5c002b2bd9a3928338b50d2a62785660b")
TIE_LAST = ("8fda8e06bc4c20ae53bf3b11b3dcae86baed52a2455d5488d1eaf1219357be48",
            "09ecce0f8f19e81d35f0933872ab6509f7f905b8c5ae3e99b32ab24e8c9e3255")
TIE_ALL_30 = "4e599193f85ae68aea3e5cadf2b7285eac0ad1f57d68ddb57129a09001aa9d39"
TIE_FIRST_5 = "53d5b3f5600108fe146ad7a1764b6db5b53a6676d47fd2879b27a581a0b1acc9"
LONG_WORDS = "d250bf8bd570b5a7dff2aaaca49d7b74408ffa820bf738b88ebafc165a9d1956"
MID_PRESPLIT = "7d043af730dd40b76c25c68dfad525f2cf21d8fda6691fa844f666d9f4eb20fd"
MID_ATOMS = "188d3ac09886943341375faee3dc4ae085601e7a4d6746e4e1a2c9f862338c65"
WORK_PARTITIONS = {4095: "ac4efcadf2f475fbfddf702c3291eb35adaa0c9572b573e6694dfd100c42192d",
                   8192: "a37aed7a8cb6b44b1615a527f0eb576592ca3efc127b6cfbbef9bd66ecec8867",
                   65535: "60a1253c5d15154d9d5c98e8dc6caec6894751902d12f045db41879deeeff135",
                   65536: "e082f6326a01f7f796df1db6cdeb8b4b8c2ac6c02ea20ab9b1fe22841d11cd06",
                   100003: "235ccf6d474f0723a83b0c9ce0b334764c4f4b674c7d1984ae30aa456ec322d9"}


def test_a0_corpus():
    assert rc.corpus_digest(*rc.a0_corpus()) == A0


@pytest.mark.parametrize("seed", [31, 32])
def test_walker_case(seed):
    t2i, text, offs = rc.walker_case(seed)
    assert (rc.vocab_digest(t2i), rc.corpus_digest(text, offs)) == WALKER[seed]
    assert ("▁" in t2i) == (seed == 31)


def test_tie_heavy_cases():
    recs = [(rc.vocab_digest(t2i), rc.corpus_digest(text, offs)) for t2i, text, offs in rc.tie_heavy_cases(30, 400)]
    assert len(recs) == 30 and recs[0] == TIE_FIRST and recs[-1] == TIE_LAST

    def combined(r):
        return hashlib.sha256("".join(v + c for v, c in r).encode()).hexdigest()
    assert combined(recs) == TIE_ALL_30 and combined(recs[:5]) == TIE_FIRST_5
    # the lean-route test takes the first five: one generator, so they are the same five
    five = [(rc.vocab_digest(t2i), rc.corpus_digest(text, offs)) for t2i, text, offs in rc.tie_heavy_cases(5, 400)]
    assert five == recs[:5]


def test_long_words_corpus():
    assert rc.corpus_digest(*rc.long_words_corpus()) == LONG_WORDS


def test_mid_pass_forms():
    strings = rc.mid_pass_strings()
    assert rc.corpus_digest(*rc.mid_pass_presplit(strings)) == MID_PRESPLIT
    assert rc.corpus_digest(*rc.mid_pass_atoms(strings)) == MID_ATOMS
    # the raw form is new with the lean-route tests: the same words, one space between them
    text, offs = rc.mid_pass_raw(strings)
    raw = bytes(text)
    for i in (0, 1, 301, 599):
        assert raw[int(offs[i]):int(offs[i + 1])].decode() == " ".join(strings[i])


@pytest.mark.parametrize("n", sorted(WORK_PARTITIONS))
def test_work_partition_corpus(n):
    assert rc.corpus_digest(*rc.work_partition_corpus(n)) == WORK_PARTITIONS[n]
