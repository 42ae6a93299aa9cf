"""dpt_bpe_encode (csrc/dpt_bpe.hip) against the plain-Python rule of tests/bpe_ref.py on the tables and strings of
tests/bpe_fuzz.py: random pair tables with many equal ranks, the doubling and the absorbing tables, words on every
edge of the LDS window, the carried open word, the hand-over to the in-place merge and that merge itself.  That the
corpus reaches each of these paths, and tells the rule from its look-alikes, is checked on the CPU
(tests/test_bpe_fuzz_ref.py); here every call goes through ``bpe_harness.check``: ids, counts, status and tok_word,
every output between canaries."""
import numpy as np
import pytest

import bpe_fuzz as bf
import bpe_harness
import bpe_ref

pytestmark = pytest.mark.gpu


def check(batch, **kw):
    """One call over a batch's strings -> the model's answer."""
    from dptok import Bpe, Vocab
    from dptok.pack import pack_word_atoms
    t = batch.table
    vocab, bpe = Vocab(t.t2i, 0), Bpe(*t.pairs, device=0)
    text, offs, cut = pack_word_atoms(batch.strings)
    nb = int(offs[-1])
    args = (bpe, vocab, bpe_ref.piece_ids(t.t2i), t.table, np.diff(offs.astype(np.int64)), text.tobytes()[:nb], cut.tobytes()[:nb])
    want = bpe_harness.check(*args, **kw)
    if not kw:      # the same answer at the other alignment, without tok_word
        bpe_harness.check(*args, want=want, pad=1, off0=0, tok_word=False)
    return want


def test_random_tables():
    batches = bf.batches("random")
    assert len(batches) == bf.N_RANDOM_TABLES
    for b in batches:
        want = check(b)
        assert len(want) == 25 and sorted(w[0] for w in want)[-3:] == [0, 1, 1]
        assert max(len(w[1]) for w in want) > 20


def test_adversarial_tables():
    batches = bf.batches("adversarial")
    assert [b.table.name for b in batches] == ["doubling-ascending", "doubling-descending", "absorb-right", "absorb-left"]
    for b in batches:
        want = check(b)
        assert all(w[0] == 0 for w in want)
        if b.table.name.startswith("absorb"):
            # the words alone, then each between short words: all of a word ends in its x or y
            n = len(bf.LENGTHS)
            assert all(len(w[1]) == 1 for w in want[:n]) and all(len(w[1]) == 22 for w in want[n:])
        else:
            a = b.table.symbols[0]
            assert want[bf.LENGTHS.index(450)][1] == [b.table.t2i[a * 64]] * 7 + [b.table.t2i[a * 2]]


def test_directed_window_events():
    batches = bf.batches("directed")
    assert [b.table.name.rsplit("-", 1)[1] for b in batches] == ["s1", "s1000000"]
    for b in batches:
        want = check(b)
        assert all(w[0] == 0 for w in want)


def test_fuzz_strings_share_a_wave(monkeypatch):
    from dptok import _lib
    (b,) = bf.batches("wave")
    monkeypatch.setenv("DPT_WAVE_GRID_BLOCKS", "1")
    assert _lib.wave_grid(len(b.strings), 4) == 1 and len(b.strings) >= 8 * 4
    want = check(b)
    assert sum(w[0] for w in want) >= 6 and sum(w == (0, [], []) for w in want) >= 5
