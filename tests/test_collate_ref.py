"""tests/collate_ref.py (the dpt_collate rule as Python) against hand-written answers (no GPU needed)."""
import pytest

from collate_ref import BOS, EOS, I64, PAD_LEFT, TRUNC_LEFT, collate_ref

IDS = [10, 11, 12, 13, 14, 15, 16]
P, G, B, E = 0, -100, 1, 2   # pad, ignore, bos, eos


def one(n, flags, L=4, ids=IDS, **kw):
    """string of the first n ids -> its (row, mask, labels, length)"""
    r, m, lab, ln = collate_ref(ids, [0, n], row_len=L, pad_id=P, bos_id=B, eos_id=E, ignore_id=G, flags=flags, **kw)
    return r[0], m[0], lab[0], ln[0]


def test_no_flags():
    assert one(2, 0) == ([10, 11, P, P], [1, 1, 0, 0], [10, 11, G, G], 2)
    assert one(4, 0) == ([10, 11, 12, 13], [1, 1, 1, 1], [10, 11, 12, 13], 4)
    assert one(6, 0) == ([10, 11, 12, 13], [1, 1, 1, 1], [10, 11, 12, 13], 4)


def test_each_flag_alone():
    assert one(2, BOS) == ([B, 10, 11, P], [1, 1, 1, 0], [B, 10, 11, G], 3)
    assert one(2, EOS) == ([10, 11, E, P], [1, 1, 1, 0], [10, 11, E, G], 3)
    assert one(2, PAD_LEFT) == ([P, P, 10, 11], [0, 0, 1, 1], [G, G, 10, 11], 2)
    assert one(6, TRUNC_LEFT) == ([12, 13, 14, 15], [1, 1, 1, 1], [12, 13, 14, 15], 4)
    assert one(2, TRUNC_LEFT) == ([10, 11, P, P], [1, 1, 0, 0], [10, 11, G, G], 2)
    assert one(2, I64) == one(2, 0)


def test_all_flags_together():
    f = BOS | EOS | PAD_LEFT | TRUNC_LEFT | I64
    assert one(1, f) == ([P, B, 10, E], [0, 1, 1, 1], [G, B, 10, E], 3)
    assert one(6, f) == ([B, 14, 15, E], [1, 1, 1, 1], [B, 14, 15, E], 4)   # the specials survive truncation
    assert one(6, BOS | EOS) == ([B, 10, 11, E], [1, 1, 1, 1], [B, 10, 11, E], 4)


@pytest.mark.parametrize("flags,nsp", [(0, 0), (BOS, 1), (EOS, 1), (BOS | EOS, 2)])
def test_lengths_around_the_row(flags, nsp):
    L = 5
    room = L - nsp
    head, tail = ([B] if flags & BOS else []), ([E] if flags & EOS else [])
    for n in (0, 1, room - 1, room, room + 1):
        keep = min(n, room)
        seq = head + IDS[:keep] + tail
        fill = L - len(seq)
        assert one(n, flags, L=L) == (seq + [P] * fill, [1] * len(seq) + [0] * fill, seq + [G] * fill, keep + nsp)
        seq_l = head + IDS[n - keep:n] + tail
        assert one(n, flags | PAD_LEFT | TRUNC_LEFT, L=L) == ([P] * fill + seq_l, [0] * fill + [1] * len(seq_l),
                                                              [G] * fill + seq_l, keep + nsp)


def test_empty_string_yields_its_specials():
    assert one(0, 0) == ([P] * 4, [0] * 4, [G] * 4, 0)
    assert one(0, BOS | EOS) == ([B, E, P, P], [1, 1, 0, 0], [B, E, G, G], 2)


def test_row_of_specials_only():
    assert one(3, BOS | EOS, L=2) == ([B, E], [1, 1], [B, E], 2)
    assert one(3, EOS | TRUNC_LEFT, L=1) == ([E], [1], [E], 1)
    with pytest.raises(ValueError):
        one(3, BOS | EOS, L=1)
    with pytest.raises(ValueError):
        one(3, 0, L=0)


def test_failed_string_and_layouts():
    ids = [10, 11, 12, 13, 14, 15]
    # CSR layout, a shard: off[0] = 100 corresponds to ids[0]
    r, m, lab, ln = collate_ref(ids, [100, 102, 102, 106], status=[0, 3, 0], row_len=3, pad_id=9, ignore_id=G,
                                bos_id=B, flags=BOS)
    assert r == [[B, 10, 11], [9, 9, 9], [B, 12, 13]]
    assert m == [[1, 1, 1], [0, 0, 0], [1, 1, 1]]
    assert lab == [[B, 10, 11], [G, G, G], [B, 12, 13]]
    assert ln == [3, 0, 3]
    # counts layout: the ids sit at the strings' byte offsets; a failed string's range and count are not read
    r, m, lab, ln = collate_ref(ids, [0, 3, 5, 6], counts=[2, 2, 0], status=[0, 1, 0], row_len=3, pad_id=9, ignore_id=G)
    assert r == [[10, 11, 9], [9, 9, 9], [9, 9, 9]] and m == [[1, 1, 0], [0, 0, 0], [0, 0, 0]] and ln == [2, 0, 0]
    assert lab == [[10, 11, G], [G, G, G], [G, G, G]]


def test_negative_ids_sign_extend():
    ids = [-1, -2 ** 31, 2 ** 31 - 1]
    r, m, lab, ln = collate_ref(ids, [0, 3], row_len=5, pad_id=-7, bos_id=-3, ignore_id=-100, flags=BOS | I64)
    assert r == [[-3, -1, -2 ** 31, 2 ** 31 - 1, -7]] and lab == [[-3, -1, -2 ** 31, 2 ** 31 - 1, -100]]
    assert m == [[1, 1, 1, 1, 0]] and ln == [4]
