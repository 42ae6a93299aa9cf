"""The loops of lane-mode B and C1 (forward_lanes of tokenize_kernel: the cut-point pass, the recurrence step, the C1
walk step and the de-mode re-walk) on what their shape can break and the older tests do not name: the census corpus
(tests/lane_walk_cases.py -- every situation the steps decide on, asserted reached by tests/test_lane_walk_census.py)
on both first-pass routes; waves whose rows have very different trip counts, one of them not walking at all; and the
other instantiations of the shared code (the one-string kernel's 64-lane rows, the 512-byte pass's chunks of up to 33
boundaries).  Every comparison is ids, offsets, status and capped lengths against the C oracle; every status is 0
apart from the empty string placed on purpose, so no string goes uncompared."""
import numpy as np
import pytest

from lane_walk_cases import census_corpus
from lean_routes import both_routes

pytestmark = pytest.mark.gpu

BOS = ["<s>", "<", "s", ">"]   # llama mode's first word and its atoms: with them the windows stay capless


@pytest.fixture(scope="module")
def ctx():
    from dptok import Encoder, Vocab
    from oracle import oracle
    t2i, texts = census_corpus()
    return Encoder(Vocab(t2i, 0)), oracle.OracleVocab(t2i), texts


def test_census_corpus_on_both_routes(ctx):
    from dptok import pack_strings
    enc, orc, texts = ctx
    assert enc.debug_lean_words() == (0, 0, 0, 0)
    text, offs = pack_strings(texts)
    ref = both_routes(enc, orc, text, offs)
    assert np.all(ref[2] == 0), np.nonzero(ref[2])[0][:10]
    words = enc.debug_lean_words()
    assert words[2] == 0 and words[3] == 0, ("the lean pair was not launched", words)


def _uneven(texts, rng):
    """a 1-byte string, a 256-byte single word, an empty string and a 300-byte string with spaces (two windows)"""
    letters = "".join(t.replace(" ", "a").replace("\n", "b") for t in texts)
    long2 = "".join(texts).replace("\n", "c")[:300]
    assert " " in long2[:256] and " " in long2[256:] and len(long2) == 300
    four = ["b", letters[:256], "", long2]
    return [four[int(k)] for k in rng.permutation(4)]


@pytest.mark.parametrize("n", [4, 8])
def test_uneven_rows_in_one_wave(ctx, n):
    """The wave steps as long as its longest lane; the empty string's row (status 2) does not walk at all."""
    from dptok import pack_strings
    enc, orc, texts = ctx
    rng = np.random.default_rng(n)
    batch = _uneven(texts, rng)
    if n == 8:   # the second wave's rows: the same four in another order next to census strings
        batch = batch[:2] + [texts[3], texts[-1]] + batch[2:] + [texts[-2], texts[7]]
    text, offs = pack_strings(batch)
    ref = both_routes(enc, orc, text, offs)
    want = np.array([2 if s == "" else 0 for s in batch], dtype=ref[2].dtype)
    assert np.array_equal(ref[2], want), ref[2]
    assert np.all(np.diff(ref[1].astype(np.int64))[want == 0] > 0)   # the other rows were tokenized


def test_one_string_kernel(ctx):
    """Encoder.encode_one: the whole wave on one window, chunks of at most 5 boundaries."""
    from dptok import pack_strings
    enc, orc, texts = ctx
    picks = texts[:8] + texts[-4:]   # a dozen, the rows built for T == 0 beside T >= 15 among them
    ids, off, st, _ = orc.encode_csr(*pack_strings(picks))
    assert np.all(st == 0)
    for k, s in enumerate(picks):
        got, status = enc.encode_one(s)
        assert status == 0
        assert list(got) == ids[int(off[k]): int(off[k + 1])].tolist(), (k, s)


def test_512_byte_pass():
    """Pre-split words of 300..509 letters: mid_kernel, chunks of up to 33 boundaries and the 64-bit cut mask."""
    from dptok import Encoder, Vocab, pack_strings, synth
    from oracle import oracle
    t2i, texts = census_corpus()
    t2i = {t: i for i, t in enumerate(sorted(set(t2i) | set(BOS)))}
    letters = "".join(t.replace(" ", "a").replace("\n", "b") for t in texts)
    lens = [300, 301, 333, 383, 384, 385, 417, 450, 480, 507, 508, 509]
    words, at = [], 0
    for n in lens:
        words.append(letters[at: at + n])
        at += n
    assert all(len(w) == n for w, n in zip(words, lens))
    text, offs, cut = synth.llama_words(*pack_strings(words))
    got = Encoder(Vocab(t2i, 0)).encode_csr(text, offs, mode="presplit", cut_mask=cut)
    ref = oracle.OracleVocab(t2i).encode_csr(text, offs, mode=oracle.PRESPLIT, cut_mask=cut)
    assert np.all(ref[2] == 0), ref[2]
    for k in (2, 1, 0, 3):   # status, offsets, ids, capped lengths
        assert np.array_equal(got[k], ref[k]), (k, np.nonzero(np.asarray(got[k][:len(ref[k])]) != ref[k][:len(got[k])])[0][:10])
