"""TEST INFRASTRUCTURE: the census corpus of the lane-mode B / C1 loops (forward_lanes of tokenize_kernel): one
tie-heavy capless vocabulary (tests/test_lane_model.py::tie_heavy_case) with the '\\n' atom and a few tokens across
it, and at most 400 seeded strings of at most 256 bytes, some of them with '\\n'.  tests/test_lane_walk_census.py
asserts on the CPU model (tools/lane_model.py) that the corpus reaches every situation the walk and recurrence loops
branch on; tests/test_gpu_lane_walk.py runs the same strings through the kernels."""
import functools

import numpy as np

from test_lane_model import tie_heavy_case

NL = "<0x0A>"   # the atom a '\n' byte becomes: six code points over one byte
SEED = 7
N_RANDOM = 380
MAX_BYTES = 256


def _letters(rng, n):
    s = ""
    while len(s) < n:
        s += tie_heavy_case(rng, max_len=256)[1].replace(" ", "c")
    return s[:n]


@functools.lru_cache(maxsize=None)
def census_corpus(seed=SEED):
    """-> (token -> id, the strings)"""
    rng = np.random.default_rng(seed)
    vocab = set(tie_heavy_case(rng)[0])
    # the '\n' atom (so that windows with it stay capless) and tokens whose span crosses it
    vocab |= {NL, "a" + NL, NL + "b", "b" + NL + "a", "c" + NL + NL, "ab" + NL + "c", "▁" + NL}
    texts = []
    for n in range(N_RANDOM):
        t = tie_heavy_case(rng, max_len=MAX_BYTES)[1]
        if n % 3 == 0 and len(t) > 1:   # a few '\n' (never the first byte: it carries the word mark)
            c = list(t)
            for p in rng.integers(1, len(t), size=int(rng.integers(1, 6))):
                c[int(p)] = "\n"
            t = "".join(c)
        texts.append(t)
    # rows with an empty chunk beside a chunk of single-atom words: 209..224 atoms make chunks of 15 boundaries
    # that leave the last lanes nothing, and every space of a run is a one-atom word (a token each)
    for na, run in ((209, 40), (212, 64), (224, 48), (210, 33)):
        head = int(rng.integers(20, 90))
        texts.append(_letters(rng, head) + " " * run + _letters(rng, na - head - run))
    assert len(texts) <= 400 and all(len(t.encode()) <= MAX_BYTES and t.isascii() for t in texts)
    return {t: i for i, t in enumerate(sorted(vocab))}, texts
