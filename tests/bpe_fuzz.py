"""TEST INFRASTRUCTURE: what the fuzz tests of dpt_bpe_encode share (tests/test_bpe_fuzz_ref.py on the CPU,
tests/test_gpu_bpe_fuzz.py on the device).  No torch, no device.

Pair tables that natural language does not make -- random tables over two to four symbols with many equal ranks, the
doubling table, and the two absorbing tables whose one merge marches across a whole word --, strings whose words sit
on every edge of the kernel's window (csrc/dpt_bpe.hip: W_LDS, WIN, FLUSH and the 64-byte round), directed strings for
the events random ones reach rarely, and ``schedule``: a plain-Python model of the kernel's bookkeeping that says
which of its paths a string takes.  All of it is deterministic: a table or a string is a function of its seed.

A string is a list of words, a word a list of atoms (str), as ``dptok.pack.pack_word_atoms`` takes them."""
from __future__ import annotations

import functools
import heapq
import random
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import bpe_ref

# csrc/dpt_bpe.hip (tests/test_bpe_fuzz_ref.py::test_constants_in_sync reads them from its text)
W_LDS = 256            # words of up to this many atoms always merge in LDS
WIN = W_LDS + 128      # slots of a wave's window
FLUSH = WIN - 64       # a window holding more than this merges before the next round
ROUND = 64             # bytes of a string per round, one lane each; also the slots of a window chunk

LENGTHS = (1, 2, 3, 5, 17, 40, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 300, 319, 320, 321, 383, 384, 385, 450, 700)
SHORT = (1, 2, 3, 5, 17, 40)
MAX_WORD = 700         # the in-place merge is quadratic; tests/test_gpu_bpe.py has the word of 5,000 atoms

# one-character symbols of 1, 2, 3 and 4 bytes; BIG is one atom of 70 bytes, longer than a round
POOLS = {1: "abcd", 2: "éèüö", 3: "中文字符", 4: "\U0001F600\U0001F601\U0001F602\U0001F603"}
BIG = "~" * 70
JUNK = ("Z", "Ω", "~~~~~", BIG + "~")   # no token; the last two leave the trie inside BIG and past its end

Str = List[List[str]]


class FuzzTable(NamedTuple):
    name: str
    t2i: Dict[str, int]
    pairs: Tuple[List[int], List[int], List[int], List[int]]   # left, right, merged, rank
    symbols: List[str]                                         # the atoms its words are made of (BIG apart)
    text_pairs: Optional[List[Tuple[str, str, int]]]           # (a, b, rank) where every pair merges into a + b

    @property
    def table(self) -> bpe_ref.Table:
        return bpe_ref.table_of(*self.pairs)


def _finish(name, tokens, text_pairs, symbols, rnd, merged_of=None) -> FuzzTable:
    """Ids in a shuffled order, BIG among them."""
    ids = list(range(len(tokens) + 1))
    rnd.shuffle(ids)
    t2i = dict(zip(list(tokens) + [BIG], ids))
    pairs = ([t2i[a] for a, b, _ in text_pairs], [t2i[b] for a, b, _ in text_pairs],
             [t2i[merged_of(a, b) if merged_of else a + b] for a, b, _ in text_pairs], [r for _, _, r in text_pairs])
    return FuzzTable(name, t2i, pairs, list(symbols), None if merged_of else list(text_pairs))


def random_table(seed: int, k: int, n_merges: int, span: int) -> FuzzTable:
    """k symbols of random byte widths; n_merges pairs of tokens made so far (the earlier ones more often), merging
    into a + b of at most 12 characters, each at a rank from range(span)."""
    rnd = random.Random(f"random-table-{seed}-{k}-{n_merges}-{span}")
    symbols = [POOLS[rnd.choice((1, 2, 3, 4))][i] for i in range(k)]
    tokens, pairs = list(symbols), {}
    while len(pairs) < n_merges:
        a = tokens[min(rnd.randrange(len(tokens)), rnd.randrange(len(tokens)))]
        b = tokens[min(rnd.randrange(len(tokens)), rnd.randrange(len(tokens)))]
        if (a, b) in pairs or len(a + b) > 12:
            continue
        if a + b not in tokens:
            tokens.append(a + b)
        pairs[(a, b)] = rnd.randrange(span)
    return _finish(f"random-{seed}-k{k}-m{n_merges}-s{span}", tokens, [(a, b, r) for (a, b), r in pairs.items()], symbols, rnd)


def doubling_table(descending: bool) -> FuzzTable:
    """a a -> aa, aa aa -> aaaa, ... up to 64 characters, the ranks ascending or descending (then every product
    outranks all that is live); a second symbol merges with nothing."""
    a, other = (POOLS[3][0], "b") if descending else ("a", POOLS[2][0])
    rnd = random.Random(f"doubling-{descending}")
    tokens = [a * (1 << i) for i in range(7)] + [other]
    text_pairs = [(a * (1 << i), a * (1 << i), 5 - i if descending else i) for i in range(6)]
    return _finish("doubling-" + ("descending" if descending else "ascending"), tokens, text_pairs, [a, other], rnd)


def absorb_table(right: bool) -> FuzzTable:
    """One pair whose product is one of its own halves: (x, b) -> x over words x b...b, or (b, y) -> y over b...b y.
    A word of n atoms takes n - 1 iterations of one merge each, and the merge marches through the word."""
    rnd = random.Random(f"absorb-{right}")
    if right:
        x, b = "x", "b"
        return _finish("absorb-right", [x, b], [(x, b, 7)], [x, b], rnd, merged_of=lambda l, r: l)
    b, y = POOLS[3][1], "y"
    return _finish("absorb-left", [b, y], [(b, y, 7)], [b, y], rnd, merged_of=lambda l, r: r)


# ------------------------------------------------------------------ strings

def make_word(t: FuzzTable, rnd: random.Random, n: int) -> List[str]:
    """n atoms: random symbols, or periodic with period 1, 2, 3 or 5; now and then BIG in place of one."""
    period = rnd.choice((0, 1, 2, 3, 5))
    if period:
        unit = [rnd.choice(t.symbols) for _ in range(period)]
        w = [unit[i % period] for i in range(n)]
    else:
        w = [rnd.choice(t.symbols) for _ in range(n)]
    if rnd.random() < 0.06:
        w[rnd.randrange(n)] = BIG
    return w


def absorb_word(t: FuzzTable, n: int) -> List[str]:
    x_or_b, b_or_y = t.symbols
    return [x_or_b] + [b_or_y] * (n - 1) if t.name == "absorb-right" else [x_or_b] * (n - 1) + [b_or_y]


def random_string(t: FuzzTable, rnd: random.Random, target: int) -> Str:
    """Words of the listed lengths, short ones more often, until the string holds about ``target`` atoms."""
    words, total = [], 0
    while total < target:
        n = rnd.choice(SHORT) if rnd.random() < 0.55 or total + 64 > target else rnd.choice(LENGTHS)
        words.append(make_word(t, rnd, n))
        total += n
    return words


def with_junk(words: Str, rnd: random.Random, late: bool) -> Str:
    """``words`` with one atom that is no token: among the first 40 atoms, or among the last 20."""
    n = sum(len(w) for w in words)
    k = n - 1 - rnd.randrange(20) if late else rnd.randrange(min(40, n))
    out = [list(w) for w in words]
    for w in out:
        if k < len(w):
            w[k] = rnd.choice(JUNK)
            break
        k -= len(w)
    return out


def strings_for(t: FuzzTable, seed: int, count: int, max_atoms: int = 1500) -> List[Str]:
    """``count`` strings of 64 to about max_atoms atoms; among them one empty string and two with an atom that is
    no token, before any flush and after the first."""
    rnd = random.Random(f"strings-{t.name}-{seed}")
    targets = [64, max_atoms] + [rnd.choice((64, 100, 200, 330, 400, 600, 900, 1200, 1500)) for _ in range(count - 5)]
    out = [random_string(t, rnd, min(n, max_atoms)) for n in targets]
    out += [[], with_junk(random_string(t, rnd, 600), rnd, False), with_junk(random_string(t, rnd, 600), rnd, True)]
    rnd.shuffle(out)
    return out


# ------------------------------------------------------------------ the model of the kernel's schedule

CENSUS = ("windows", "window_iterations", "cross_chunk_merges", "carried_flushes", "carry_then_long", "window_to_long",
          "long_rounds_no_start", "long_close_skip0", "long_close_mid", "long_close_end", "zero_atom_rounds",
          # beyond the list of the kernel's paths: window fills on the flush mark, strings that fail early and late
          "fill_eq_flush", "fill_eq_flush_plus_1", "zero_atom_rounds_long", "bad_before_flush", "bad_after_flush")


def merge_slots(sym: Sequence[int], base: int, table: bpe_ref.Table, rightmost: bool = False):
    """One word in window slots base .. base + len(sym), merged by the rule as the window merges it: the left slot
    keeps the product, the right one dies -> (tokens, merges, merges whose two slots lie in different 64-slot
    chunks).  ``rightmost``: the look-alike rule that takes the rightmost pair on equal rank."""
    sym = list(sym)
    n = len(sym)
    nxt, prv, alive = list(range(1, n + 1)), list(range(-1, n - 1)), [True] * n
    heap, merges, cross = [], 0, 0
    sign = -1 if rightmost else 1

    def push(i):
        j = nxt[i]
        if j < n:
            e = table.get((sym[i], sym[j]))
            if e is not None:
                heapq.heappush(heap, (e[0], sign * i, sym[i], sym[j], e[1]))

    for i in range(n - 1):
        push(i)
    while heap:
        _, i, a, b, m = heapq.heappop(heap)
        i *= sign
        j = nxt[i] if alive[i] else n
        if not alive[i] or j >= n or sym[i] != a or sym[j] != b:
            continue
        merges += 1
        cross += (base + i) // ROUND != (base + j) // ROUND
        sym[i], alive[j] = m, False
        nxt[i] = nxt[j]
        if nxt[j] < n:
            prv[nxt[j]] = i
        push(i)
        if prv[i] >= 0:
            push(prv[i])
    return [s for s, a in zip(sym, alive) if a], merges, cross


def model(nbytes: int, atoms: Sequence[Tuple[int, bool, int]], table: bpe_ref.Table):
    """The kernel's bookkeeping over one string of nbytes bytes; atoms: (first byte, opens a word, id or -1) in order
    -> (census, status, ids, tok_word)."""
    c = dict.fromkeys(CENSUS, 0)
    ids: List[int] = []
    words: List[int] = []
    win: List[List[int]] = []            # [symbol, slot of its word's first symbol]
    state = {"n_words": 0, "open_head": 0, "flushed": False}
    long: Optional[List[int]] = None     # the open word, once it lives in the output slots
    rounds: Dict[int, list] = {}
    for k, (pos, ws, tid) in enumerate(atoms):
        rounds.setdefault(pos // ROUND, []).append((ws or k == 0, tid))

    def emit(toks):
        ids.extend(toks)
        words.extend([state["n_words"]] * len(toks))
        state["n_words"] += 1

    def merge_window(L):
        c["windows"] += 1
        state["flushed"] = True
        i, iters = 0, 0
        while i < L:
            j = i + 1
            while j < L and win[j][1] == win[i][1]:
                j += 1
            toks, merges, cross = merge_slots([s for s, _ in win[i:j]], i, table)
            iters = max(iters, merges)      # one merge per word and iteration
            c["cross_chunk_merges"] += cross
            emit(toks)
            i = j
        c["window_iterations"] += iters
        del win[:L]
        for e in win:
            e[1] = 0
        state["open_head"] = 0

    def close_long():
        emit(bpe_ref.merge_word_fast(long, table))

    for k in range((nbytes + ROUND - 1) // ROUND):
        ra = rounds.get(k, [])
        if any(tid < 0 for _, tid in ra):
            c["bad_after_flush" if state["flushed"] else "bad_before_flush"] += 1
            return c, bpe_ref.NO_TOKENIZATION, [], []
        c["zero_atom_rounds"] += not ra
        c["zero_atom_rounds_long"] += not ra and long is not None
        starts = [i for i, (ws, _) in enumerate(ra) if ws]
        skip = 0
        if long is not None:
            skip = starts[0] if starts else len(ra)
            long += [tid for _, tid in ra[:skip]]
            if not starts:
                c["long_rounds_no_start"] += 1
                continue
            c["long_close_skip0" if skip == 0 else "long_close_mid"] += 1
            close_long()
            long = None
        for ws, tid in ra[skip:]:
            if ws:
                state["open_head"] = len(win)
            win.append([tid, state["open_head"]])
        assert len(win) <= WIN
        c["fill_eq_flush"] += len(win) == FLUSH
        c["fill_eq_flush_plus_1"] += len(win) == FLUSH + 1
        if len(win) > FLUSH:
            carried = state["open_head"] != 0
            if carried:
                c["carried_flushes"] += 1
                merge_window(state["open_head"])
            if len(win) > FLUSH:
                c["window_to_long"] += 1
                c["carry_then_long"] += carried
                state["flushed"] = True
                long = [s for s, _ in win]
                win.clear()
    if long is not None:
        c["long_close_end"] += 1
        close_long()
    elif win:
        merge_window(len(win))
    return c, 0, ids, words


def atoms_of(t: FuzzTable, words: Str):
    """(nbytes, atoms) of a string, as ``model`` takes them."""
    atoms, pos = [], 0
    for w in words:
        for k, a in enumerate(w):
            atoms.append((pos, k == 0, t.t2i.get(a, -1)))
            pos += len(a.encode("utf-8"))
    return pos, atoms


def schedule(nbytes: int, atoms, table: bpe_ref.Table) -> Dict[str, int]:
    """The census of one string: how often it takes each of the kernel's paths."""
    return model(nbytes, atoms, table)[0]


def census(t: FuzzTable, words: Str, table: Optional[bpe_ref.Table] = None) -> Dict[str, int]:
    return schedule(*atoms_of(t, words), table or t.table)


# ------------------------------------------------------------------ directed strings

DIRECTED_PER_EVENT = 3


def directed_strings(t: FuzzTable) -> List[Tuple[str, Str]]:
    """(census counter, string) pairs: for each event that random strings reach rarely, the first three strings of a
    seeded search that the model sends through it."""
    table = t.table
    word = lambda rnd, n: make_word(t, rnd, n)                                         # noqa: E731
    shorts = lambda rnd, total: [word(rnd, rnd.choice(SHORT[:5])) for _ in range(total // 4)]   # noqa: E731
    makers = {
        # a window whose fill lands on the flush mark, and one past it
        "fill_eq_flush": lambda rnd: shorts(rnd, rnd.randrange(330, 800)),
        "fill_eq_flush_plus_1": lambda rnd: shorts(rnd, rnd.randrange(330, 800)),
        # an open word that is carried to the front and is still too long for the window
        "carry_then_long": lambda rnd: [word(rnd, rnd.choice(SHORT)), word(rnd, rnd.randrange(FLUSH + 1, MAX_WORD)), word(rnd, 3)],
        # a long word closed by a word start that is its round's first atom, closed mid-round, and never closed
        "long_close_skip0": lambda rnd: [word(rnd, rnd.randrange(FLUSH + 1, 520)), word(rnd, 5)],
        "long_close_mid": lambda rnd: [word(rnd, rnd.randrange(FLUSH + 1, 520)), word(rnd, 5)],
        "long_close_end": lambda rnd: [word(rnd, 3), word(rnd, rnd.randrange(FLUSH + 1, 520))],
        # a round without an atom, in the window and inside a long word
        "zero_atom_rounds": lambda rnd: [word(rnd, rnd.randrange(1, 70)) + [BIG] + word(rnd, 9)],
        "zero_atom_rounds_long": lambda rnd: [word(rnd, rnd.randrange(FLUSH + 1, 400)) + [BIG] + word(rnd, 30), word(rnd, 2)],
    }
    out = []
    for key, make in makers.items():
        rnd = random.Random(f"directed-{t.name}-{key}")
        found = 0
        for _ in range(50000):
            words = make(rnd)
            if census(t, words, table)[key]:
                out.append((key, words))
                found += 1
                if found == DIRECTED_PER_EVENT:
                    break
        else:
            raise AssertionError(f"too few strings of table {t.name} reach {key}")
    return out


# ------------------------------------------------------------------ the corpus of the GPU tests

class Batch(NamedTuple):
    group: str            # "random", "adversarial", "directed", "wave"
    table: FuzzTable
    strings: List[Str]


N_RANDOM_TABLES = 12
K, N_MERGES, SPANS = (2, 3, 4), (3, 8, 20, 60), (1, 2, 4, 10 ** 6)


def random_tables() -> List[FuzzTable]:
    """Twelve tables: every (k, n_merges) once, every span three times."""
    return [random_table(i, K[i % 3], N_MERGES[i % 4], SPANS[(i // 3) % 4]) for i in range(N_RANDOM_TABLES)]


def small_tables() -> List[FuzzTable]:
    """Tables of 1, 2 and 3 pairs (the pair-table lookups)."""
    return [random_table(100 + n, 2, n, 10 ** 6) for n in (1, 2, 3)]


def _adversarial() -> List[Batch]:
    out = []
    for desc in (False, True):
        t = doubling_table(desc)
        a, other = t.symbols
        rnd = random.Random(t.name)
        strings = [[[a] * n] for n in LENGTHS]
        strings += [[[a] * 5, [other], [a] * n, [a] * 3] for n in (FLUSH - 6, FLUSH - 5, 450, MAX_WORD)]
        strings += [[[rnd.choice((a, a, a, other)) for _ in range(n)]] for n in (64, 300, 450)]
        out.append(Batch("adversarial", t, strings))
    for right in (True, False):
        t = absorb_table(right)
        strings = [[absorb_word(t, n)] for n in LENGTHS]
        # between short words: the word is carried to the window's front, and goes long where it is too long
        strings += [[absorb_word(t, 3)] * 20 + [absorb_word(t, n), absorb_word(t, 2)] for n in LENGTHS]
        out.append(Batch("adversarial", t, strings))
    return out


@functools.lru_cache(maxsize=None)
def corpus() -> Tuple[Batch, ...]:
    """Every string the GPU tests run, by test."""
    tables = random_tables()
    out = [Batch("random", t, strings_for(t, 0, 25)) for t in tables]
    out += _adversarial()
    # one table with span 1 and one with span 10^6
    for t in (tables[1], tables[10]):
        assert t.name.endswith(("-s1", "-s1000000"))
        out.append(Batch("directed", t, [s for _, s in directed_strings(t)]))
    # several strings per wave: empty and failing strings between the others
    t = tables[5]
    rnd = random.Random("wave")
    strings = strings_for(t, 1, 28, max_atoms=900)
    strings += [[]] * 5 + [with_junk(random_string(t, rnd, 500), rnd, late) for late in (False, True) * 3]
    rnd.shuffle(strings)
    out.append(Batch("wave", t, strings))
    return tuple(out)


def batches(group: str) -> List[Batch]:
    return [b for b in corpus() if b.group == group]
