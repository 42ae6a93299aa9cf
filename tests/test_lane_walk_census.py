"""The census corpus (tests/lane_walk_cases.py) reaches every situation the loops of lane-mode B and C1 decide on
(forward_lanes of tokenize_kernel: the recurrence step, the C1 walk step and the de-mode re-walk), counted by the CPU
model of the algorithm (tools/lane_model.py, the ``stats`` dict).  A condition on the corpus, not a measurement: the
GPU test of the same strings (tests/test_gpu_lane_walk.py) then exercises each of them.  The model's tokens are
compared with the C oracle's on the way, so the counters are read off a correct run."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lane_walk_cases import census_corpus  # noqa: E402


@pytest.fixture(scope="module")
def census():
    import lane_model
    from oracle import oracle
    from dptok import pack_strings
    t2i, texts = census_corpus()
    inv = {i: t for t, i in t2i.items()}
    vocab = set(t2i)
    ids, off, st, _ = oracle.OracleVocab(t2i).encode_csr(*pack_strings(texts))
    assert np.all(st == 0), np.nonzero(st)[0][:10]
    stats = {}
    for n, text in enumerate(texts):
        want = [inv[i] for i in ids[int(off[n]): int(off[n + 1])].tolist()]
        assert lane_model.model(text, vocab, stats=stats) == want, (n, text)
    return stats


def test_corpus_bounds():
    t2i, texts = census_corpus()
    assert len(texts) <= 400 and max(len(t.encode()) for t in texts) <= 256
    assert any("\n" in t for t in texts)


@pytest.mark.parametrize("key", [
    "fold_changed",    # the chunk-start rule picks de over a different dg
    "wend_mid_walk",   # a word end is entered in the middle of a walk
    "re_ws",           # a chunk ends on a word start
    "not_p1in",        # a chunk's first piece is not P1
    "rewalk",          # the de-mode re-walk is taken ...
    "rewalk_steps",    # ... over at least one token
    "t0_t15_rows",     # a row holds a chunk with T == 0 beside a chunk with T >= 15
    "nl_span",         # a token span crosses a '\n' atom (the code-point prefix jumps by 6)
])
def test_corpus_reaches(census, key):
    assert census.get(key, 0) >= 1, (key, {k: v for k, v in census.items() if k != "g1"})
