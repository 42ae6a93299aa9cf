"""The CPU model of the raw window tiling and the lean classifier (tests/lean_ref.py): properties over seeded strings
and hand-worked cases for every branch of the window rule.  No GPU."""
import numpy as np
import pytest

import lean_ref
from lean_ref import raw_windows


def _seeded_strings(n, seed):
    """letters with spaces at a seeded density (0: none, so long words occur), lengths 0..1200"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        L = int(rng.integers(0, 1200)) if k % 5 else int(rng.integers(250, 265))
        p = (0.0, 0.003, 0.01, 0.05, 0.3)[k % 5 if k % 7 else 0]
        b = rng.integers(0x61, 0x7B, size=L).astype(np.uint8)
        b[rng.random(L) < p] = 0x20
        out.append(b.tobytes())
    return out


def test_window_properties():
    n_long = n_multi = 0
    for b in _seeded_strings(4000, 7):
        wins, long_word = raw_windows(b)
        pos = 0
        for k, (p, wlen) in enumerate(wins):
            assert p == pos and 1 <= wlen <= 256          # they tile from 0, none empty, none over 256 bytes
            assert k == 0 or b[p] == 0x20                 # every window but the first starts with a space
            pos += wlen
        if long_word:   # the walk stopped at a word that fits no window: more than 256 bytes left, none a usable space
            assert len(b) - pos > 256 and 0x20 not in b[pos + 1:pos + 257]
            n_long += 1
        else:
            assert pos == len(b)                          # ... and reach the end
            # each window but the last is as long as it can be: no later space would have fitted
            for p, wlen in wins[:-1]:
                assert 0x20 not in b[p + wlen + 1:p + 257]
        n_multi += len(wins) > 2
    assert n_long > 100 and n_multi > 500


def _s(n, spaces=()):
    b = bytearray(b"x" * n)
    for k in spaces:
        b[k] = 0x20
    return bytes(b)


@pytest.mark.parametrize("b,wins,long_word", [
    (b"", [], False),
    (_s(1), [(0, 1)], False),
    (_s(256), [(0, 256)], False),                          # exactly 256 bytes: the whole rest, space or none
    (_s(256, [0]), [(0, 256)], False),
    (_s(257, [1]), [(0, 1), (1, 256)], False),             # the only space at index 1
    (_s(257, [255]), [(0, 255), (255, 2)], False),         # ... at 255: the last of bytes 1..255
    (_s(257, [256]), [(0, 256), (256, 1)], False),         # ... at 256: the byte past a full window
    (_s(257), [], True),                                   # no space at all
    (_s(257, [0]), [], True),                              # byte 0 the only space: it starts the window anyway
    (_s(300, [100, 256]), [(0, 256), (256, 44)], False),   # byte 256 lies later than the space at 100
    (_s(300, [100, 255]), [(0, 255), (255, 45)], False),
    (_s(300, [100, 257]), [(0, 100), (100, 200)], False),  # a space at 257 is out of reach
    (_s(600, [10]), [(0, 10)], True),                      # a long word after a first window
    (_s(769, [1, 257, 513]), [(0, 1), (1, 256), (257, 256), (513, 256)], False),
])
def test_window_branches(b, wins, long_word):
    assert raw_windows(b) == (wins, long_word)


def test_no_token_sets_and_lean_window():
    t2i = {t: i for i, t in enumerate(["a", "b", "▁", "▁a", "<0x0A>", "\t", "▁ ", "ab"])}
    nt, fnt = lean_ref.no_token_bytes(t2i), lean_ref.first_no_token_bytes(t2i)
    # a space is '▁', '\n' is "<0x0A>", the rest themselves; the first byte carries the mark, unrespelled
    assert {0x20, 0x0A, 0x61, 0x62, 0x09}.isdisjoint(nt) and len(nt) == 128 - 5
    assert sorted(set(range(128)) - fnt) == [0x20, 0x61]
    assert lean_ref.lean_window(b"ab a\nb\t", nt)
    assert not lean_ref.lean_window(b"abc", nt)
    assert not lean_ref.lean_window("aé".encode(), nt)
    assert not lean_ref.lean_window(b"a\x7f", nt)
    assert lean_ref.lean_window(b"ab", nt, fnt) and lean_ref.lean_window(b" b", nt, fnt)
    assert not lean_ref.lean_window(b"ba", nt, fnt)       # 'b' is a token, '▁b' is not
    assert lean_ref.lean_window(b"", nt, fnt)
    no_mark = {"a": 0}                                     # '▁' no token: a space makes a window not capless
    assert 0x20 in lean_ref.no_token_bytes(no_mark) and not lean_ref.lean_window(b"a a", lean_ref.no_token_bytes(no_mark))


def test_predicted_deferred():
    nt = frozenset({0x7F})
    e = "é".encode()
    strings = [b"", b"abc", b"ab" + e, b"a\x7fb",
               _s(300, [100]) + e,                         # poison in the second window
               _s(10, [5]) + b" " + _s(300) + b" " + e,    # lean window, long word, then poison: the retry list
               e + _s(10) + b" " + _s(300),                # a poisoned window first, then the long word: deferred
               e + _s(300),                                # the long word holds the poison: no window, not deferred
               _s(257, [256])[:256] + b" " + e]            # a clean 256-byte window, poison after it
    assert lean_ref.predicted_deferred(strings, nt) == {2, 3, 4, 6, 8}
    # the first byte is judged by its own set
    assert lean_ref.predicted_deferred([b"\x7fab", b"a\x7f"], frozenset(), frozenset({0x7F})) == {0}
    text = np.frombuffer(b"".join(strings) + b"\0", np.uint8)
    offs = np.cumsum([0] + [len(s) for s in strings]).astype(np.uint64)
    assert lean_ref.split_blob(text, offs) == strings


def test_edge_matrix_is_what_it_says():
    """tests/lean_edge_matrix.py (run on the GPU by tests/test_gpu_lean_edges.py): the bases' windows, one poison per
    variant with the base's length and windows kept, calls of whole waves with at most five deferred strings and
    every count of 1..5, every base directly in front of each kind of neighbour, last in a blob, at every alignment"""
    import collections
    import lean_edge_matrix as mx
    bs = mx.bases()
    mx.check_bases(bs)
    tok2 = "ب".encode()
    by_name = {name: b for name, b, _, _ in bs}
    vs = mx.variants(bs, tok2)
    for v, (name, poison, place) in vs.items():
        b = by_name[name]
        assert len(v) == len(b) and raw_windows(v) == raw_windows(b)
        diff = [k for k in range(len(b)) if v[k] != b[k]]
        assert 1 <= len(diff) <= 2 and diff[-1] - diff[0] == len(diff) - 1 and (poison != "d" or diff[0] > 0)
    places = collections.Counter((p, pl) for _, p, pl in vs.values())
    for poison in "ed":
        for place in ("w1+1", "w1+2", "w1+3", "w1end", "w2+1", "w3+1", "w3end", "end"):
            assert places[(poison, place)] >= 10, (poison, place)
    assert places[("e", "w1+0")] >= 10 and places[("t", "w3end")] >= 10
    assert [name for name, b, _, _ in bs if mx.is_deferred(b)] == ["sp0", "sp0len256"]   # they start with a space

    def counts(calls):
        for name, strings in calls:
            assert len(strings) % mx.SLOTS == 0, name
        return collections.Counter(mx.n_deferred(s) for _, s in calls)
    c = counts(mx.variant_calls(bs, tok2))
    assert set(c) == {0, 1, 2, 3, 4, 5} and c[0] == 1 and min(c[k] for k in range(1, 6)) >= 40
    assert set(counts(mx.variant_calls(bs, tok2, mx.subset_select))) == {1, 2, 3, 4, 5}
    nb = mx.neighbour_calls(bs, tok2)
    assert {0, 5} <= set(counts(nb)) <= set(range(6)) and set(counts(mx.alignment_calls(bs))) == {2}
    follows = collections.defaultdict(set)
    last = set()
    for _, strings in nb + mx.alignment_calls(bs):
        for x, y in zip(strings, strings[1:]):
            follows[x].add(y[:1] if y[:1] in (b"\x7f", b"") else y[:2] if y[0] >= 0x80 else b"a")
        last.add(strings[-1])
    starts = collections.defaultdict(set)
    for _, strings in mx.alignment_calls(bs):
        pos = 0
        for s in strings:
            starts[s].add(pos % 4)
            pos += len(s)
    for name, b, _, _ in bs:
        assert {b"\x7f", b"", mx.E, tok2} <= follows[b], name
        assert b in last and starts[b] == {0, 1, 2, 3}, name
