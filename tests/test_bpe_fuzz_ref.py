"""What the device fuzz of dpt_bpe_encode (tests/test_gpu_bpe_fuzz.py) rests on, checked without a GPU: the reference
rule of tests/bpe_ref.py agrees with itself and with ``tokenizers`` on the fuzz tables, the corpus of tests/bpe_fuzz.py
tells the rule from two look-alikes and reaches every path of the kernel's schedule often enough, the pair tables
answer every lookup, and the schedule model's constants are the kernel's."""
import collections
import itertools
import os
import random
import re

import numpy as np
import pytest

import bpe_fuzz as bf
import bpe_ref


def all_tables():
    seen = {}
    for b in bf.corpus():
        seen.setdefault(b.table.name, b.table)
    for t in bf.small_tables():
        seen[t.name] = t
    return list(seen.values())


@pytest.fixture(scope="module")
def corpus_words():
    """Every distinct word of the corpus, as ids, of the strings that are all tokens: [(table name, Table, ids)]."""
    out, seen = [], set()
    for b in bf.corpus():
        table = b.table.table
        for s in b.strings:
            if any(a not in b.table.t2i for w in s for a in w):
                continue
            for w in s:
                ids = tuple(b.table.t2i[a] for a in w)
                if (b.table.name, ids) not in seen:
                    seen.add((b.table.name, ids))
                    out.append((b.table.name, table, ids))
    return out


def test_constants_in_sync():
    """W_LDS, WIN, FLUSH of tests/bpe_fuzz.py are those of csrc/dpt_bpe.hip, and a round is a wave of 64 lanes."""
    import dptok
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(dptok.__file__))), "csrc", "dpt_bpe.hip")
    with open(path, encoding="utf-8") as fh:
        text = fh.read()
    env = {}
    for name in ("W_LDS", "WIN", "FLUSH"):
        m = re.search(r"constexpr\s+unsigned\s+%s\s*=\s*([A-Z_0-9+\-* ]+);" % name, text)
        assert m, name
        env[name] = eval(m.group(1), {"__builtins__": {}}, dict(env))   # (integers, + - * and the names before it)
    assert env == {"W_LDS": bf.W_LDS, "WIN": bf.WIN, "FLUSH": bf.FLUSH}
    assert bf.ROUND == 64 and "k0 += 64" in text and "c * 64u + lane" in text


def test_model_equals_reference():
    """The schedule model -- windows, flushes, the carried word, the long word -- gives what the plain rule gives on
    every string of the corpus: ids, word indices and status."""
    from dptok.pack import pack_word_atoms
    n = 0
    for b in bf.corpus():
        text, offs, cut = pack_word_atoms(b.strings)
        nb = int(offs[-1])
        table = b.table.table
        want = bpe_ref.encode(bpe_ref.piece_ids(b.table.t2i), table, np.diff(offs.astype(np.int64)), text.tobytes()[:nb], cut.tobytes()[:nb])
        for s, w in zip(b.strings, want):
            nbytes, atoms = bf.atoms_of(b.table, s)
            _, status, ids, words = bf.model(nbytes, atoms, table)
            assert (status, ids, words) == w, (b.table.name, s)
            n += 1
    assert n > 400


def test_reference_is_self_consistent(corpus_words):
    """The literal rule equals the heap version the long words are checked with, on every word of up to 400 atoms."""
    n = 0
    for name, table, ids in corpus_words:
        if len(ids) <= 400:
            assert bpe_ref.merge_word(ids, table) == bpe_ref.merge_word_fast(ids, table) == bf.merge_slots(ids, 0, table)[0], (name, ids)
            n += 1
    assert n > 1000


def test_reference_equals_tokenizers(corpus_words):
    """An implementation that shares no code with the reference: ``tokenizers``' BPE model over the same vocabulary and
    merges, on the random tables whose ranks are all distinct (its merges are a list, so it has no equal ranks)."""
    models = pytest.importorskip("tokenizers.models")
    tables = [t for t in all_tables() if t.text_pairs and t.name.startswith("random") and len(set(t.pairs[3])) == len(t.pairs[3])]
    assert len(tables) >= 4 and any(len(t.pairs[0]) == 60 for t in tables)
    n = 0
    for t in tables:
        bpe = models.BPE(vocab=dict(t.t2i), merges=[(a, b) for a, b, _ in sorted(t.text_pairs, key=lambda p: p[2])])
        table, rnd = t.table, random.Random("anchor-" + t.name)
        back = {v: k for k, v in t.t2i.items()}
        words = [[back[i] for i in ids] for name, _, ids in corpus_words if name == t.name and len(ids) <= 400]
        words += [bf.make_word(t, rnd, rnd.choice(bf.LENGTHS[:14])) for _ in range(150)]
        for w in words:
            if bf.BIG in w:         # (not one character: tokenizers would split it)
                continue
            assert [tok.id for tok in bpe.tokenize("".join(w))] == bpe_ref.merge_word_fast([t.t2i[a] for a in w], table), (t.name, w)
            n += 1
    assert n >= 1200


def merge_local_minima(sym, table):
    """A look-alike: every sweep merges every pair whose (rank, position) is below both its neighbours'."""
    sym = list(sym)
    while True:
        keys = [(table[p][0], i) if p in table else None for i, p in enumerate(zip(sym, sym[1:]))]
        k = [x or (bpe_ref.NO_RANK + 1, 0) for x in keys]
        take = {i for i in range(len(k)) if keys[i] and (i == 0 or k[i] < k[i - 1]) and (i + 1 == len(k) or k[i] < k[i + 1])}
        if not take:
            return sym
        out, i = [], 0
        while i < len(sym):
            out.append(table[(sym[i], sym[i + 1])][1] if i in take else sym[i])
            i += 2 if i in take else 1
        sym = out


def test_corpus_discriminates(corpus_words):
    """A kernel that merged every local minimum at once, or took the rightmost pair on equal rank, would give other ids
    on at least 5 % of the corpus's words."""
    ws = [w for w in corpus_words if len(w[2]) > 1]
    ref = [bpe_ref.merge_word_fast(ids, table) for _, table, ids in ws]
    local = sum(merge_local_minima(ids, table) != r for (_, table, ids), r in zip(ws, ref)) / len(ws)
    right = sum(bf.merge_slots(ids, 0, table, rightmost=True)[0] != r for (_, table, ids), r in zip(ws, ref)) / len(ws)
    print(f"words {len(ws)}; differ: local minima {local:.3f}, rightmost on equal rank {right:.3f}")
    assert local >= 0.05 and right >= 0.05
    # and the two are what they say: on the toy cases of tests/test_gpu_bpe.py
    p, q, r, s, P, Q, R = range(7)
    t = bpe_ref.table_of([p, P, r], [q, r, s], [P, Q, R], [0, 1, 2])
    assert merge_local_minima([p, q, r, s], t) == [P, R] and bpe_ref.merge_word([p, q, r, s], t) == [Q, s]
    t = bpe_ref.table_of([0], [0], [1], [0])
    assert bf.merge_slots([0, 0, 0], 0, t, rightmost=True)[0] == [0, 1] and bpe_ref.merge_word([0, 0, 0], t) == [1, 0]


def test_corpus_reaches_every_path():
    """Summed over the corpus, every counter of the schedule's census is at least 5 and the three that random inputs
    were meant for at least 50; every listed word length occurs; every directed string takes its path."""
    total = collections.Counter()
    lengths = collections.Counter()
    for b in bf.corpus():
        table = b.table.table
        for s in b.strings:
            total.update(bf.census(b.table, s, table))
            lengths.update(len(w) for w in s)
    print("census:", dict(total))
    assert set(total) == set(bf.CENSUS)
    assert all(total[k] >= 5 for k in bf.CENSUS), dict(total)
    assert all(total[k] >= 50 for k in ("cross_chunk_merges", "carried_flushes", "window_to_long")), dict(total)
    assert all(lengths[n] >= 5 for n in bf.LENGTHS) and max(lengths) == bf.MAX_WORD
    directed = bf.batches("directed")
    assert len(directed) == 2
    for b in directed:
        named = bf.directed_strings(b.table)
        assert [s for _, s in named] == b.strings
        per_event = collections.Counter(key for key, _ in named)
        assert set(per_event.values()) == {bf.DIRECTED_PER_EVENT}
        assert set(per_event) == {"fill_eq_flush", "fill_eq_flush_plus_1", "carry_then_long", "long_close_skip0", "long_close_mid",
                                  "long_close_end", "zero_atom_rounds", "zero_atom_rounds_long"}
        for key, s in named:
            assert bf.census(b.table, s)[key] >= 1, (b.table.name, key)
    # every absorbing word takes one merge per iteration: n - 1 iterations where the window holds it whole
    for b in bf.batches("adversarial"):
        if b.table.name.startswith("absorb"):
            c = bf.census(b.table, [bf.absorb_word(b.table, bf.W_LDS)])
            # (x stays in slot 0 and eats into the later chunks; y's product moves down one slot per merge)
            cross = bf.W_LDS - bf.ROUND if b.table.name == "absorb-right" else bf.W_LDS // bf.ROUND - 1
            assert c["window_iterations"] == bf.W_LDS - 1 and c["cross_chunk_merges"] == cross
    # the strings that share a wave: at least 8 to each of a block's 4 waves, failing and empty ones among them
    (wave,) = bf.batches("wave")
    c = collections.Counter()
    for s in wave.strings:
        c.update(bf.census(wave.table, s))
    assert len(wave.strings) >= 32 and wave.strings.count([]) >= 5 and c["bad_before_flush"] >= 3 and c["bad_after_flush"] >= 3


def test_pair_table_lookups():
    """Every table through the host builder and the one probe function (dpt_debug_bpe_lookup): every pair answers with
    its (merged, rank), every other (l, r) of V x V misses."""
    from dptok.bpe import debug_lookup
    tables = all_tables()
    assert sorted(len(t.pairs[0]) for t in tables)[:4] == [1, 1, 1, 2] and any(len(t.pairs[0]) == 3 for t in tables)
    for t in tables:
        v = sorted(t.t2i.values())
        ql, qr = zip(*itertools.product(v, v))
        merged, rank = debug_lookup(*t.pairs, ql, qr)
        table = t.table
        assert len(table) == len(t.pairs[0])
        want = [table.get(q, (bpe_ref.NO_RANK, -1)) for q in zip(ql, qr)]
        assert merged.tolist() == [m for _, m in want] and rank.tolist() == [r for r, _ in want], t.name
