"""The fold of lane-mode B's dg fix-up pass into the C1 walk (tokenize_kernel's forward_lanes,
restated by tools/lane_model.py): the folded form -- G(i) - 1 recorded at every end by the
recurrence, the chunk-start rule applied at the ends the walk visits -- selects what the two-pass
form (a fix-up loop over every end of (rs, lim], then the plain walk) selects.  CPU only;
tests/test_gpu_lane_fold.py checks the kernel."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from test_lane_model import tie_heavy_case  # noqa: E402

SEEDS = range(1000, 1016)
WINDOWS = 250


def test_folded_walk_equals_fixup_pass():
    """16 seeds x 250 windows; every fourth text has its spaces replaced by a letter, so every
    chunk but the first has an incoming G and the rule is live over whole chunks."""
    import lane_model
    stats = {}
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        for n in range(WINDOWS):
            vocab, text = tie_heavy_case(rng, max_len=256)
            if n % 4 == 0:
                text = text.replace(" ", "a")
            vs = set(vocab)
            folded = lane_model.model(text, vs, stats=stats)
            assert folded == lane_model.model(text, vs, fold=False), (seed, n, text, vocab)
    # not vacuous: the folded rule picked de where the plain rule picks a different dg
    assert stats["fold_changed"] > 0, stats["walk_steps"]
    assert stats["walk_steps"] > stats["fold_changed"]
    # what the recurrence (and the word-end update) wrote fits bits 11..14 of rec[i].cpos
    assert len(stats["g1"]) > 0
    assert all(0 <= g <= 15 for g in stats["g1"])
