"""The lean first pass of plain raw calls (16-lane vocabularies; DESIGN.md 4, "the lean pass"): a kernel that takes
only pure-ASCII capless windows and defers every other string to a list, then the general kernel over what is left
of the partitions and over that list.  Every case runs the route twice on one context -- with the lean launch and,
through the context's test switch (dpt_ctx_debug_no_lean), without it -- through the device entry with a
DPT_HIST_OVERWRITE histogram: ids, offsets, status and histogram must be identical, and equal to the C oracle's."""
import numpy as np
import pytest

from lean_routes import both_routes as _both_routes, device_call as _device_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines(vocabs):
    from dptok import Encoder, Vocab
    return {k: Encoder(Vocab(v, 0)) for k, v in vocabs.items()}


@pytest.fixture(scope="module")
def oracles(vocabs):
    from oracle import oracle
    return {k: oracle.OracleVocab(v) for k, v in vocabs.items()}


def _pack(texts):
    from dptok import pack_strings
    return pack_strings(texts)


MIXED = ["plain ascii words here", "café au lait", "line one\nline two\n", "", "x", "tail with \n newline",
         "zq~|^ `{}", "another plain one, with punctuation!", "عربي text"]


@pytest.mark.parametrize("vocab", ["llama32k", "toy1k"])
@pytest.mark.parametrize("n", [4, 9])
def test_one_wave_mixed_slots(vocab, n, vocabs, engines, oracles):
    """pure ASCII, a 2-byte code point, '\\n', an empty string and (toy1k: most bytes are no token by themselves) windows
    that are not capless, side by side in the slots of one wave"""
    texts = MIXED[:n]
    # a byte that is no token by itself, where the vocabulary has one: its window is not capless
    lone = [chr(c) for c in range(1, 128) if chr(c) not in vocabs[vocab] and chr(c) not in " \n"]
    if lone:
        texts[1] = "ab" + lone[0] + "cd ef"
        texts[0] = "café au lait"
    assert all(len(t.encode()) <= 64 for t in texts)
    text, offs = _pack(texts)
    ref = _both_routes(engines[vocab], oracles[vocab], text, offs)
    assert ref[2][3] == 2   # the empty string


def test_deferred_after_staging_and_long_word(vocabs, engines, oracles):
    """a non-ASCII character in the second / the third window of a 600..700-byte ASCII string: the string is deferred
    after its first windows staged ids; and a single word of more than 256 bytes (the 2048-byte pass's)"""
    rng = np.random.default_rng(21)

    def ascii_text(nbytes):
        words = []
        while sum(len(w) + 1 for w in words) < nbytes:
            words.append("".join(chr(c) for c in rng.integers(0x61, 0x7B, size=int(rng.integers(2, 9)))))
        return " ".join(words)[:nbytes]
    a, b, c = ascii_text(650), ascii_text(690), ascii_text(620)
    hi = [k for k in vocabs["llama32k"] if len(k) == 1 and ord(k) > 0x7F][1:3]   # non-ASCII code points that are tokens
    assert len(hi) == 2
    texts = [a[:300] + hi[0] + a[300:],        # in the second window
             b[:560] + hi[1] + b[560:],        # in the third
             c,                                      # all lean, three windows
             "".join(chr(x) for x in rng.integers(0x21, 0x7F, size=300)),   # one 300-byte word
             "ab " + "".join(chr(x) for x in rng.integers(0x21, 0x7F, size=257)) + " cd",
             a[:200] + "\nmid\n" + a[200:600]]
    text, offs = _pack(texts)
    ref = _both_routes(engines["llama32k"], oracles["llama32k"], text, offs)
    assert (ref[2] == 0).all()


def test_two_partitions_one_percent_non_ascii(engines, oracles):
    """9,000 short strings (two partitions: min(16, n / 4096)), 1 % of them with a non-ASCII character at seeded
    positions: every deferred string comes back exactly once"""
    from dptok import synth
    n = 9000
    text, offs = synth.random_ascii_corpus(n, 24, seed=13)
    texts = synth.unpack(text, offs)
    rng = np.random.default_rng(14)
    for s in rng.choice(n, size=n // 100, replace=False):
        t = texts[int(s)]
        k = int(rng.integers(0, len(t) + 1))
        texts[int(s)] = t[:k] + "é" + t[k:]
    text, offs = _pack(texts)
    _both_routes(engines["llama32k"], oracles["llama32k"], text, offs)


def test_all_deferred_calls_between_lean_calls(engines, oracles):
    """2,000 Arabic-shaped strings (every string deferred: about four per wave, too few for the hint to go off --
    test_hint_observed has the size for that), an ASCII call and the Arabic call again on the same context, each with
    and without the lean launch: exact outputs whatever the calls before left behind"""
    from dptok import synth
    enc, orc = engines["llama32k"], oracles["llama32k"]
    arabic = synth.arabic_corpus(2000, length=64, seed=56)
    ascii_ = synth.random_ascii_corpus(2000, 64, seed=57)
    for text, offs in (arabic, ascii_, arabic, ascii_, ascii_):
        _both_routes(enc, orc, text, offs)


def test_workspace_bytes_with_and_without_lean(vocabs):
    """the lean route allocates nothing: its list is the third retry list, its hint a spare line of the counter block"""
    from dptok import Encoder, Vocab, synth
    text, offs = synth.random_ascii_corpus(5000, 64, seed=60)
    sizes = []
    for off in (False, True):
        enc = Encoder(Vocab(vocabs["llama32k"], 0))
        enc.debug_no_lean(off)
        _device_call(enc, text, offs)
        sizes.append(enc.workspace_bytes())
    assert sizes[0] == sizes[1], sizes


def test_hint_observed(vocabs, oracles):
    """The hint itself, read through dpt_ctx_debug_lean_words on a fresh context whose every call may take the lean route.
    100,000 strings: every wave of the grid holds more than two refills, so on Arabic text each lean wave defers its
    first eight strings (two refills of four), turns the hint off and claims nothing more -- the general launch finishes
    the partly consumed partitions, then the list.  While the hint is off the host plans seven calls of eight without
    the lean launch; the eighth launches it, the lean waves claim nothing and the first one probes: on Arabic text the
    hint stays off and nothing is deferred, on ASCII text it goes on, and the call after that is lean again.  Every call
    exact."""
    import torch
    from dptok import Encoder, Vocab, synth
    RETRY = 8   # dpt_internal.h LEAN_RETRY
    enc, orc = Encoder(Vocab(vocabs["llama32k"], 0)), oracles["llama32k"]
    n = 100_000
    arabic = synth.arabic_corpus(n, length=64, seed=58)
    ascii_ = synth.random_ascii_corpus(n, 64, seed=59)
    refs = {id(c): orc.encode_csr(*c) for c in (arabic, ascii_)}
    waves = 22 * torch.cuda.get_device_properties(0).multi_processor_count   # the grid, at most
    assert 12 * waves < n   # (else no wave reaches its third refill and the hint never goes off)
    assert enc.debug_lean_words() == (0, 0, 0, 0)

    def call(corpus):
        got = _device_call(enc, *corpus)
        for k in range(4):
            assert np.array_equal(got[k], refs[id(corpus)][k]), k
        return enc.debug_lean_words()
    assert call(ascii_) == (0, 0, 0, 0)                      # ASCII: all lean, nothing deferred
    off, deferred, probes, skipped = call(arabic)            # Arabic: the hint goes off; eight strings per wave at most
    assert off == 1 and 0 < deferred <= 8 * waves and (probes, skipped) == (0, 0)
    for k in range(1, RETRY):                                # no lean launch: the words stay, the host counts
        assert call(arabic) == (1, deferred, 0, k)
    assert call(arabic) == (1, 0, 1, RETRY)                  # the retry: nothing deferred, one probe, still off
    for k in range(RETRY + 1, 2 * RETRY):
        assert call(ascii_) == (1, 0, 1, k)
    assert call(ascii_) == (0, 0, 2, 2 * RETRY)              # the retry on ASCII text: its probe turns the hint on
    assert call(ascii_) == (0, 0, 2, 0)                      # lean again, no probe
