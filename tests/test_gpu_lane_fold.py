"""Lane-mode B with the dg fix-up folded into the C1 walk (tokenize_kernel's forward_lanes: the 256-byte
first pass, the one-string kernel, the 512-byte pass), against the C oracle on tie-heavy capless
vocabularies: space-free words (every chunk but the first has an incoming G, so the folded rule decides
over whole chunks), texts with spaces (the rule stops at the chunk's first word end, whose L* the
incoming G may raise), the same in llama mode, and the length-only calls.  Every status is 0, so every
string is compared.  tests/test_lane_fold_model.py pins the rule itself on the CPU."""
import numpy as np
import pytest

from test_lane_model import tie_heavy_case

pytestmark = pytest.mark.gpu

# chunk lengths C = ((na + LW - 1) / LW) | 1 of 1, 3, 5 and 17 boundaries and their edges (LW = 16 lanes
# per window; 64 in the one-string kernel, where C <= 5)
WORD_LENS = [17, 18, 19, 33, 34, 35, 36, 50, 51, 52, 254, 255, 256]
BATCHES = [1, 4, 5, 400]
# the BOS word of llama mode ("<s>", dptok.synth.llama_words) and its atoms: with them the windows stay
# capless (every atom a token by itself), which is what sends a wave to lane mode
BOS = ["<s>", "<", "s", ">"]


def _word(rng, n):
    """n letters of tie_heavy_case texts, their spaces replaced by a letter"""
    s = ""
    while len(s) < n:
        s += tie_heavy_case(rng, max_len=256)[1].replace(" ", "b")
    return s[:n]


def _vocab(rng, extra=()):
    vocab = sorted(set(tie_heavy_case(rng)[0]) | set(extra))
    return {t: i for i, t in enumerate(vocab)}


def _cmp(got, ref):
    assert np.all(ref[2] == 0), np.nonzero(ref[2])[0][:10]   # no case is skipped
    assert np.array_equal(got[2], ref[2]), np.nonzero(got[2] != ref[2])[0][:10]
    assert np.array_equal(got[1], ref[1]), np.nonzero(got[1] != ref[1])[0][:10]
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(got[3], ref[3])


def _single_word_batches(rng):
    for nb in BATCHES:
        if nb == 1:
            for n in WORD_LENS:
                yield [_word(rng, n)]
        else:
            yield [_word(rng, WORD_LENS[(k + nb) % len(WORD_LENS)]) for k in range(nb)]


@pytest.mark.parametrize("seed", [41, 42, 43])
def test_space_free_single_words(seed):
    """Case 1, and case 4 on the same strings: the DP-length call ran the removed loop too."""
    from dptok import Encoder, Vocab, pack_strings
    from oracle import oracle
    rng = np.random.default_rng(seed)
    for _ in range(2):
        t2i = _vocab(rng)
        enc, ov = Encoder(Vocab(t2i, 0)), oracle.OracleVocab(t2i)
        for texts in _single_word_batches(rng):
            text, offs = pack_strings(texts)
            ref = ov.encode_csr(text, offs)
            _cmp(enc.encode_csr(text, offs), ref)
            st, lens, _ = enc.dp(text, offs, mode="raw")
            assert np.array_equal(st, ref[2])
            assert np.array_equal(lens, ref[3])


@pytest.mark.parametrize("seed", [51, 52, 53])
def test_texts_with_spaces(seed):
    """Case 2: a word end inside a chunk."""
    from dptok import Encoder, Vocab, pack_strings
    from oracle import oracle
    rng = np.random.default_rng(seed)
    for _ in range(3):
        t2i = _vocab(rng)
        texts = [tie_heavy_case(rng, max_len=256)[1] for _ in range(400)]
        text, offs = pack_strings(texts)
        _cmp(Encoder(Vocab(t2i, 0)).encode_csr(text, offs), oracle.OracleVocab(t2i).encode_csr(text, offs))


@pytest.mark.parametrize("seed", [61, 62, 63])
def test_llama_mode_and_the_512_byte_pass(seed):
    """Case 3: the pre-split words of llama mode ('▁'-compressed windows), and space-free words of
    257..512 bytes ('▁' + 254..509 letters), which go to the 512-byte pass: chunks of up to 33
    boundaries, the 64-bit cut mask."""
    from dptok import Encoder, Vocab, pack_strings, synth
    from oracle import oracle
    rng = np.random.default_rng(seed)
    for _ in range(2):
        t2i = _vocab(rng, BOS)
        enc, ov = Encoder(Vocab(t2i, 0)), oracle.OracleVocab(t2i)
        texts = [tie_heavy_case(rng, max_len=256)[1] for _ in range(400)]
        longw = [_word(rng, n) for n in (254, 255, 256, 300, 383, 384, 385, 450, 508, 509) for _ in range(12)]
        for batch in (texts, longw, texts[:150] + longw[::2]):
            text, offs, cut = synth.llama_words(*pack_strings(batch))
            _cmp(enc.encode_csr(text, offs, mode="presplit", cut_mask=cut),
                 ov.encode_csr(text, offs, mode=oracle.PRESPLIT, cut_mask=cut))
