"""tests/collate_pair_ref.py (the dpt_collate_pair rule as Python) against a model of the reference's collator,
against collate_ref on one-sided rows, and its truncation arithmetic exhaustively (no GPU needed)."""
import itertools
import random

from collate_pair_ref import (BOS, EOS, I64, MASK_A, PAD_LEFT, SEP, TRIM_A_FIRST, TRUNC_LEFT, collate_pair_ref, kept)
from collate_ref import collate_ref


def reference_collator(sources, targets, pad_id):
    """What ShortcutDataCollatorForSeq2Seq returns for features of (source ids, target ids): each row the
    concatenation, right-padded with the pad id to the longest; the labels are that same tensor."""
    rows = [s + t for s, t in zip(sources, targets)]
    longest = max(len(r) for r in rows)
    padded = [r + [pad_id] * (longest - len(r)) for r in rows]
    return padded, padded


def csr(lists, first=0):
    off = [first]
    for x in lists:
        off.append(off[-1] + len(x))
    return [i for x in lists for i in x], off, None, None


def test_default_case_is_the_reference_collator():
    rng = random.Random(1)
    for trial in range(20):
        n = rng.randint(1, 12)
        src = [[rng.randrange(250000) for _ in range(rng.choice([0, 0, 1, 3, 9]))] for _ in range(n)]
        tgt = [[rng.randrange(250000) for _ in range(rng.choice([0, 1, 2, 7]))] for _ in range(n)]
        src[rng.randrange(n)] += [7, 8]   # (some row is not empty)
        want_ids, want_labels = reference_collator(src, tgt, 3)
        L = len(want_ids[0])
        rows, masks, labs, types, lengths, b_start = collate_pair_ref(csr(src, first=trial), csr(tgt), row_len=L, pad_id=3,
                                                                      ignore_id=3, flags=I64)
        assert rows == want_ids and labs == want_labels
        assert lengths == [len(s) + len(t) for s, t in zip(src, tgt)] and b_start == [len(s) for s in src]
        assert masks == [[1] * n_ + [0] * (L - n_) for n_ in lengths]
        assert types == [[0] * len(s) + [1] * len(t) + [0] * (L - len(s) - len(t)) for s, t in zip(src, tgt)]


def test_empty_b_is_collate_ref():
    rng = random.Random(2)
    counts = [0, 1, 2, 3, 4, 5, 6, 9]
    a = csr([[rng.randrange(-5, 50000) for _ in range(n)] for n in counts], first=11)
    status = [0, 0, 1, 0, 0, 0, 2, 0]
    a = (a[0], a[1], None, status)
    b = ([], [5] * (len(counts) + 1), None, None)
    combos = [x | e | p | t for x in (0, BOS) for e in (0, EOS) for p in (0, PAD_LEFT) for t in (0, TRUNC_LEFT)]
    assert len(combos) == 16
    for flags in combos:
        for L in (2, 4, 5):
            kw = dict(row_len=L, pad_id=-7, bos_id=101, eos_id=102, ignore_id=-100, flags=flags)
            assert collate_pair_ref(a, b, sep_id=9, **kw)[:3] == collate_ref(a[0], a[1], None, status, **kw)[:3]
            assert collate_pair_ref(a, b, sep_id=9, **kw)[4] == collate_ref(a[0], a[1], None, status, **kw)[3]


def test_truncation_arithmetic_exhaustively():
    r = range(7)
    for nA, nB, max_a, max_b, room in itertools.product(r, r, r, r, r):
        cA = min(nA, max_a) if max_a else nA
        cB = min(nB, max_b) if max_b else nB
        for a_first in (False, True):
            kA, kB = kept(nA, nB, max_a, max_b, room, a_first)
            assert 0 <= kA <= cA and 0 <= kB <= cB
            assert kA + kB == min(cA + cB, room)
            # the side that gives first reaches 0 before the other loses any
            first, other, c_other = (kA, kB, cB) if a_first else (kB, kA, cA)
            assert other == c_other or first == 0


def test_hand_written_rows():
    a = ([10, 11, 12, 13], [0, 4], None, None)
    b = ([20, 21, 22], [0, 3], None, None)
    P, G = 0, -100

    def one(L, flags, **kw):
        out = collate_pair_ref(a, b, row_len=L, pad_id=P, bos_id=1, sep_id=5, eos_id=2, ignore_id=G, flags=flags, **kw)
        return tuple(x[0] for x in out)

    assert one(9, 0) == ([10, 11, 12, 13, 20, 21, 22, P, P], [1] * 7 + [0] * 2, [10, 11, 12, 13, 20, 21, 22, G, G],
                         [0, 0, 0, 0, 1, 1, 1, 0, 0], 7, 4)
    assert one(10, BOS | SEP | EOS | MASK_A) == ([1, 10, 11, 12, 13, 5, 20, 21, 22, 2], [1] * 10,
                                                 [G] * 6 + [20, 21, 22, 2], [0] * 6 + [1] * 4, 10, 6)
    # B gives first; the specials survive
    assert one(7, BOS | SEP | EOS)[0] == [1, 10, 11, 12, 13, 5, 2] and one(7, BOS | SEP | EOS)[5] == 6
    assert one(6, BOS | SEP | EOS)[0] == [1, 10, 11, 12, 5, 2]
    assert one(6, BOS | SEP | EOS | TRIM_A_FIRST)[0] == [1, 5, 20, 21, 22, 2]
    assert one(5, TRIM_A_FIRST | TRUNC_LEFT)[0] == [12, 13, 20, 21, 22]
    assert one(5, TRUNC_LEFT)[0] == [10, 11, 12, 13, 22]
    assert one(5, TRUNC_LEFT, max_a=2)[0] == [12, 13, 20, 21, 22]
    assert one(9, PAD_LEFT | SEP, max_b=1) == ([P, P, P, 10, 11, 12, 13, 5, 20], [0] * 3 + [1] * 6,
                                               [G, G, G, 10, 11, 12, 13, 5, 20], [0] * 8 + [1], 6, 8)
    # b_start is written when B keeps nothing, and a failed side gives the failed row
    assert one(4, 0)[4:] == (4, 4) and one(9, PAD_LEFT)[5] == 6
    failed = collate_pair_ref(a, (b[0], b[1], None, [3]), row_len=4, pad_id=9, ignore_id=G, flags=BOS)
    assert failed == ([[9] * 4], [[0] * 4], [[G] * 4], [[0] * 4], [0], [0])
    # the counts layout per side: ids at str_off, counts beside them
    mixed = collate_pair_ref(([10, 11, 12, 13], [100, 104], [2], None), b, row_len=6, flags=0)
    assert mixed[0] == [[10, 11, 20, 21, 22, 0]] and mixed[5] == [2]
