"""TEST INFRASTRUCTURE: a plain reference for the by-products of dpt_dp_host / dpt_dp_host_far --
per-string status and lengths (capped and uncapped), the per-atom-end edge masks and the far pairs --
written from the wording of include/dpt.h alone.  Pure Python (numpy only packs the results); it shares
no code with the kernels or with dptok.

Per word, over its atoms a[0..n) and the token set V (both DPs from one candidate list per end):

    cand(i)   = { j < i : join(a[j:i]) in V }
    capped    cost[i] = min(i, min{cost[j] + 1 : j in cand(i)})          (dp_tokenize.py:27-47)
    uncapped  cost[i] = min{cost[j] + 1 : j in cand(i)}, inf when empty  (inspect_tokenizer.py:77-86)
    reach[i]  = a path of tokens leads from the word start to i (reach[0]; the same for both DPs)
    mask(i)   bit d (d < 64) iff j = i-1-d in cand(i), cost[j] + 1 == cost[i] and reach[j];
              the same condition with d >= 64 is the far pair (edges index of i, d)
    valid[i]  = some chain of such edges leads from 0 to i (capped costs): the reference's DFS
                (dp_tokenize.py:49-69) finds a tokenization iff valid[n]

Per string: status 2 for an empty word, else 1 when a word has no tokenization under that DP (capped:
not valid[n]; uncapped: cost[n] is inf), else 0; lengths = the sum over words of cost[n], 65535 for an
uncapped inf; the mask of atom end i (1-based within the string) at str_off[s] - str_off[0] + i - 1.
"""
import functools
import random

import numpy as np

MARK = "▁"
NEWLINE_ATOM = "<0x0A>"
RAW, PRESPLIT, ATOMS = 0, 1, 2
MODE_OF = {"raw": RAW, "presplit": PRESPLIT, "atoms": ATOMS}
INF = float("inf")
NO_TOK = 65535
PASS_CLASSES = (None, "mid", "big", "long")


class Voc:
    """A token set with the bound a span search needs: the longest token in code points."""

    def __init__(self, tokens):
        self.tokens = frozenset(t for t in tokens if t)
        self.lens = frozenset(len(t) for t in self.tokens)
        self.max_cp = max(self.lens)


# ------------------------------------------------------------------------------------ atomisation

def atomise(text, str_off, cut_mask, mode):
    """Per string the list of its words; a word is (atoms, bytes of the word in the caller's text).
    text / cut_mask correspond to str_off[0]."""
    base = int(str_off[0])
    raw = bytes(bytearray(text))
    out = []
    for s in range(len(str_off) - 1):
        b0, b1 = int(str_off[s]) - base, int(str_off[s + 1]) - base
        if mode == RAW:
            words, cur, nb = [], [], 0
            for k, ch in enumerate(raw[b0:b1].decode("utf-8")):
                n = len(ch.encode("utf-8"))
                if k == 0:
                    cur.append(MARK + ch)
                elif ch == " ":
                    words.append((cur, nb))
                    cur, nb = [MARK], 0
                elif ch == "\n":
                    cur.append(NEWLINE_ATOM)
                else:
                    cur.append(ch)
                nb += n
            words.append((cur, nb))       # the empty string: one empty word
            out.append(words)
            continue
        cm = cut_mask[b0:b1]
        if mode == PRESPLIT:
            atom_at = [k == 0 or (raw[b0 + k] & 0xC0) != 0x80 for k in range(b1 - b0)]
            word_at = [k == 0 or cm[k] != 0 for k in range(b1 - b0)]
        else:
            atom_at = [k == 0 or (cm[k] & 3) != 0 for k in range(b1 - b0)]
            word_at = [k == 0 or (cm[k] & 1) != 0 for k in range(b1 - b0)]
        starts = [k for k in range(b1 - b0) if atom_at[k]] + [b1 - b0]
        words = []
        for a in range(len(starts) - 1):
            k, e = starts[a], starts[a + 1]
            if word_at[k]:
                words.append(([], 0))
            atoms, nb = words[-1]
            atoms.append(raw[b0 + k:b0 + e].decode("utf-8"))
            words[-1] = (atoms, nb + e - k)
        out.append(words or [([], 0)])    # the empty string: one empty word, as in RAW
    return out


def pass_of(nbytes):
    """The pass that holds a word of nbytes (the limits stated in include/dpt.h and DESIGN.md)."""
    return None if nbytes <= 256 else "mid" if nbytes <= 512 else "big" if nbytes <= 2048 else "long"


# ------------------------------------------------------------------------------------ the DP of a word

class WordDP:
    __slots__ = ("n", "cost", "reach", "valid", "mask", "far")


def word_dp(atoms, voc):
    """-> (capped WordDP, uncapped WordDP); mask[i] for i in 1..n, far = [(i, d)]."""
    n = len(atoms)
    pos = [0]
    for a in atoms:
        pos.append(pos[-1] + len(a))
    s = "".join(atoms)
    toks, lens, max_cp = voc.tokens, voc.lens, voc.max_cp
    cc, cu = list(range(n + 1)), [0] + [INF] * n
    reach, valid = [True] + [False] * n, [True] + [False] * n
    mc_, mu_, fc, fu = [0] * (n + 1), [0] * (n + 1), [], []
    for i in range(1, n + 1):
        cand = []
        pi = pos[i]
        j = i - 1
        while j >= 0:
            L = pi - pos[j]       # a span of i-j atoms has at least i-j code points
            if L > max_cp:
                break
            if L in lens and s[pos[j]:pi] in toks:
                cand.append(j)
            j -= 1
        bc, bu = i, INF
        for j in cand:
            if cc[j] + 1 < bc:
                bc = cc[j] + 1
            if cu[j] + 1 < bu:
                bu = cu[j] + 1
        cc[i], cu[i] = bc, bu
        for j in cand:
            if valid[j] and cc[j] + 1 == bc:
                valid[i] = True
            if not reach[j]:
                continue
            reach[i] = True
            d = i - 1 - j
            if cc[j] + 1 == bc:
                if d < 64:
                    mc_[i] |= 1 << d
                else:
                    fc.append((i, d))
            if cu[j] + 1 == bu:
                if d < 64:
                    mu_[i] |= 1 << d
                else:
                    fu.append((i, d))
    c, u = WordDP(), WordDP()
    c.n = u.n = n
    c.reach = u.reach = reach
    c.cost, c.valid, c.mask, c.far = cc, valid, mc_, fc
    u.cost, u.valid, u.mask, u.far = cu, reach, mu_, fu
    return c, u


# ------------------------------------------------------------------------------------ a whole call

class Result:
    """What one call returns, for both DPs (index 0 capped, 1 uncapped), plus what the input conditions
    of tests/test_dp_ref.py count.  Arrays are read-only."""


def run(text, str_off, cut_mask, mode, voc):
    words = atomise(text, str_off, cut_mask, mode)
    base = int(str_off[0])
    n_str, n_bytes = len(str_off) - 1, int(str_off[-1]) - base
    r = Result()
    r.n_str, r.n_bytes, r.words = n_str, n_bytes, words
    r.status = [np.zeros(n_str, np.int32), np.zeros(n_str, np.int32)]
    r.lengths = [np.zeros(n_str, np.int32), np.zeros(n_str, np.int32)]
    edges = [[0] * max(n_bytes, 1), [0] * max(n_bytes, 1)]
    r.far = [[], []]
    r.is_end = np.zeros(max(n_bytes, 1), bool)          # an atom end's mask lives at this index
    r.end_str = np.full(max(n_bytes, 1), -1, np.int64)  # its string
    r.end_atom = np.zeros(max(n_bytes, 1), np.int64)    # its 1-based atom index within the string
    r.end_pass = np.zeros(max(n_bytes, 1), np.int8)     # index into PASS_CLASSES of its word
    r.end_unreach = np.zeros(max(n_bytes, 1), bool)
    r.first_index = np.zeros(n_str, np.int64)
    r.n_atoms = np.zeros(n_str, np.int64)
    r.n_words = np.zeros(n_str, np.int64)
    r.later_window_atoms = np.zeros(n_str, np.int64)    # atoms of words that start past byte 256 of a string
    r.index_differs = np.zeros(n_str, bool)             # some atom end's index differs from its byte end
    for s, ws in enumerate(words):
        sb = int(str_off[s]) - base
        r.first_index[s] = sb
        r.n_words[s] = len(ws)
        ai, byte_at = 0, 0
        st = [0, 0]
        for atoms, nb in ws:
            if not atoms:
                st = [2, 2]
                continue
            pc = PASS_CLASSES.index(pass_of(nb))
            res = word_dp(atoms, voc)
            if byte_at > 256:
                r.later_window_atoms[s] += len(atoms)
            wb = byte_at
            for k, w in enumerate(res):
                total = w.cost[w.n]
                ok = w.valid[w.n]
                if not ok and st[k] == 0:
                    st[k] = 1
                r.lengths[k][s] += NO_TOK if total == INF else total
                for i in range(1, w.n + 1):
                    edges[k][sb + ai + i - 1] = w.mask[i]
                r.far[k].extend((sb + ai + i - 1, d) for i, d in w.far)
            for i in range(1, len(atoms) + 1):
                x = sb + ai + i - 1
                r.is_end[x], r.end_str[x], r.end_atom[x], r.end_pass[x] = True, s, ai + i, pc
                r.end_unreach[x] = not res[0].reach[i]
                wb += len(atoms[i - 1].encode("utf-8")) if mode != RAW else 0
                if mode != RAW and ai + i != wb:
                    r.index_differs[s] = True
            ai += len(atoms)
            byte_at += nb
        if mode == RAW and ai != int(str_off[s + 1]) - int(str_off[s]):
            r.index_differs[s] = True     # RAW: one atom per code point, so fewer atoms than bytes
        r.n_atoms[s] = ai
        r.status[0][s], r.status[1][s] = st
    r.edges = [np.array(e, dtype=np.uint64) for e in edges]
    for a in (r.status + r.lengths + r.edges + [r.is_end, r.end_str, r.end_atom, r.end_pass, r.end_unreach]):
        a.setflags(write=False)
    r.far = [sorted(f) for f in r.far]
    return r


def rebase_slice(text, str_off, cut_mask, lo, hi):
    """Strings [lo, hi) as a call of their own with offsets from 0."""
    b0, b1 = int(str_off[lo]) - int(str_off[0]), int(str_off[hi]) - int(str_off[0])
    return (text[b0:b1], (str_off[lo:hi + 1] - str_off[lo]).astype(np.uint64),
            None if cut_mask is None else cut_mask[b0:b1])


def compare_masks(got, ref, k, strings=None):
    """None when ``got`` (uint64 per index) equals the reference's masks of DP k at every atom end of the
    given strings (default: all); else the first difference (string, atom, got, want)."""
    sel = ref.is_end if strings is None else ref.is_end & np.isin(ref.end_str, strings)
    g = np.asarray(got, dtype=np.uint64)[: len(sel)]
    bad = np.flatnonzero(sel & (g != ref.edges[k]))
    if not len(bad):
        return None
    x = int(bad[0])
    return int(ref.end_str[x]), int(ref.end_atom[x]), hex(int(g[x])), hex(int(ref.edges[k][x]))


def preds_from_masks(masks, far_by_end, first, i):
    """Ascending predecessors of atom end i (1-based within a string whose first index is ``first``)."""
    m = int(masks[first + i - 1])
    out = [i - 1 - d for d in far_by_end.get(first + i - 1, ())]
    d = 0
    while m:
        if m & 1:
            out.append(i - 1 - d)
        m >>= 1
        d += 1
    return sorted(out)


# ------------------------------------------------------------------------------------ cap-trap batch
#
# The cap (cost[i] <= i, i counted from the word start) binds only where every atom before i is a token
# of its own and no longer token ends at i: so a trap sits behind a "plain" prefix whose characters are
# tokens only by themselves, and bites once per word.  'x', 'y', 'z' and 'w' are tokens only inside
# longer tokens, and 'a' only inside "abc"-like ones:
#   xabc   V has xa, abc, b, c: the end after 'x' is unreachable but capped, so "abc" from it gives the end
#          after 'c' a capped cost one below any path, with no reachable predecessor (empty mask, status
#          1); uncapped: one more, bit 0, status 0
#   zabcd  V has za, abc, cd: the end after 'c' as in xabc, and the end after 'd' has the same cost from
#          "cd" (a reachable start on a shortest path) and from "d" after the capped end -- the capped and
#          the uncapped mask differ in a word of status 0
#   yabc   the whole of "yabc" is a token too: unreachable ends, nothing else
#   wb     'w' before anything but 'a': no tokenization at all (status 1 and 65535 under both DPs)
TRAP_FILLER = "bcdefghijk"
TRAP_MULTI = ["é", "中", "😀"]
TRAP_PLAIN = list("lmnop") * 3 + ["ß", "文"]


def trap_vocab(lanes64=False, seed=5):
    rnd = random.Random(seed)
    toks = set(TRAP_FILLER) | set(TRAP_MULTI) | set(TRAP_PLAIN) | {
        MARK, MARK + "b", "xa", "ya", "za", "wa", "abc", "yabc", "cd", "a中c", "ya中c", "b中", "é😀", "中é中"}
    while len(toks) < 80:
        toks.add("".join(rnd.choice(TRAP_FILLER) for _ in range(rnd.randint(2, 5))))
    if lanes64:
        toks.add("".join(rnd.choice(TRAP_FILLER) for _ in range(40)))
    return sorted(toks)


def trap_strings(tokens, seed=9):
    """Strings of several space-separated words; every string starts with 'b' (RAW's first atom is then
    the token '▁b').  Per pass class: strings whose words hold one zabcd trap each (capped status 0),
    strings with xabc traps (capped status 1, uncapped 0); then strings with a 'w' dead end (status 1
    under both) and an empty string."""
    rnd = random.Random(seed)
    long_tok = max(tokens, key=len)
    rich = list(TRAP_FILLER) * 3 + TRAP_MULTI

    def fill(nbytes, pool, extras=()):
        out, n = [], 0
        while n < nbytes:
            x = rnd.random()
            if extras and x < 0.06:
                p = rnd.choice(extras)
            elif extras and x < 0.08 and len(long_tok) > 16:
                p = long_tok[: rnd.randint(30, len(long_tok))]
            else:
                p = rnd.choice(pool)
            out.append(p)
            n += len(p.encode("utf-8"))
        return "".join(out)

    def word(nbytes, trap, where):
        """A plain prefix of about where * nbytes bytes, the trap, rich filler with harmless traps."""
        pre = int(where * nbytes)
        return fill(pre, TRAP_PLAIN) + trap + fill(max(nbytes - pre - 8, 1), rich, ("yabc", "ya中c", "zabcd", "xabc"))

    sizes = {None: (20, 200), "mid": (270, 460), "big": (530, 900), "long": (2060, 2200)}
    out = []
    for cls in PASS_CLASSES:
        lo, hi = sizes[cls]
        for trap, n in (("zabcd", 8), ("xabc", 2), ("xa中c", 1)):
            for _ in range(n):
                ws = ["b" + fill(rnd.randint(0, 30), TRAP_PLAIN)]
                for where in (0.0, rnd.uniform(0.1, 0.8), 0.9):
                    ws.append(word(rnd.randint(lo, hi), trap, where))
                ws.append(fill(rnd.randint(3, 30), rich))
                out.append(" ".join(ws))
    for k in range(3):
        out.append("b" + fill(10 * k, rich) + " " + fill(20, rich) + "wb" + fill(30 * k, rich) + " " + fill(5, rich))
    out.insert(7, "")
    return out


def atoms_form(strings):
    """ATOMS input for strings of space-separated words: each word opened by a '▁' atom, every code
    point an atom.  -> (text, offsets, cut mask)."""
    parts, cuts, offs = [], [], [0]
    for s in strings:
        n = 0
        for w in (s.split(" ") if s else []):
            for k, a in enumerate([MARK] + list(w)):
                e = a.encode("utf-8")
                parts.append(e)
                cuts.append(bytes([3 if k == 0 else 2] + [0] * (len(e) - 1)))
                n += len(e)
        offs.append(offs[-1] + n)
    return (np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(offs, np.uint64),
            np.frombuffer(b"".join(cuts), np.uint8).copy())


def raw_form(strings):
    enc = [s.encode("utf-8") for s in strings]
    offs = np.zeros(len(enc) + 1, np.uint64)
    offs[1:] = np.cumsum([len(e) for e in enc])
    return np.frombuffer(b"".join(enc) or b"\0", np.uint8).copy(), offs, None


def trap_batch(form, lanes64):
    """(tokens, text, offsets, cut mask) of the cap-trap batch in RAW or ATOMS form."""
    tokens = trap_vocab(lanes64)
    strings = trap_strings(tokens)
    return (tokens,) + (raw_form(strings) if form == "raw" else atoms_form(strings))


# ------------------------------------------------------------------------------------ far-pair batch

def far_vocab():
    """The vocabulary shape of test_gpu_parity.py::test_enumeration_with_tokens_longer_than_64_atoms:
    tokens of 65..300 atoms and several far predecessors at one end."""
    rnd = random.Random(11)
    longs = ["".join(rnd.choice("abc") for _ in range(L)) for L in (65, 66, 70, 80, 100, 150, 300)]
    u, w = longs[2], longs[3]
    toks = {"a", "b", "c", "x", "ab", "bc", "ca", MARK, MARK + "x"} | set(longs)
    toks |= {u + w[:3], w[3:], u[:-2], u[-2:] + w}
    # the zabcd trap of the cap-trap batch with far tokens: "qrst" + D has the end after 't' capped below any
    # path, and the end after D the same cost from D (a reachable start the cap binds at) and from 't' + D
    toks |= {"qr", "rst", "s", "t", "t" + longs[1], "t" + longs[4]}
    return sorted(toks), longs


def far_strings(n_str=56, seed=13):
    """Strings of several words (every string starts with 'x'); the words with far predecessors sit
    after other words, the batch holds more than 1024 far pairs, and every seventh string has none."""
    _, longs = far_vocab()
    rnd = random.Random(seed)
    u, w = longs[2], longs[3]
    out = []
    for s in range(n_str):
        ws = ["x" + "".join(rnd.choice("abc") for _ in range(rnd.randint(1, 30)))]
        if s % 7 == 3:      # no far token at all: status 0 with or without a far list
            ws += ["".join(rnd.choice("abc") for _ in range(rnd.randint(1, 60))) for _ in range(rnd.randint(2, 5))]
            out.append(" ".join(ws))
            continue
        for k in range(rnd.randint(3, 5)):
            kind = rnd.randrange(5)
            if kind == 0:
                ws.append(u + w)
            elif kind == 1:
                ws.append("".join(rnd.choice("abc") for _ in range(rnd.randint(1, 9))) + u + w + "ab")
            elif kind == 2:
                ws.append(rnd.choice(longs) + rnd.choice(longs))
            elif kind == 3:
                ws.append(longs[6] + "abc" + longs[5] + u + w)
            else:
                ws.append(rnd.choice(longs) + "".join(rnd.choice("abc") for _ in range(rnd.randint(0, 5))) + rnd.choice(longs)[:70])
        if s % 4 == 1:      # capped status 0, and far pairs the capped and the uncapped DP disagree on
            ws.insert(2, "qrst" + longs[1 if s % 8 == 1 else 4] + "ab")
        if s % 16 == 2:     # capped status 1: the far token's start is reachable, its capped cost is no path's
            ws.insert(1, "qrst" + longs[0])
        ws.append(u + w)
        out.append(" ".join(ws))
    return out


def far_batch(form):
    tokens, _ = far_vocab()
    strings = far_strings()
    return (tokens,) + (raw_form(strings) if form == "raw" else atoms_form(strings))


# ------------------------------------------------------------------------------------ shared results

@functools.lru_cache(maxsize=None)
def corpus_ref(vocab, form):
    """The reference on the whole corpus of tests/matrix_corpus.py in one form; ``vocab`` is "base" or
    "long" (the masks do not depend on the ids, so the +40000 vocabularies share them)."""
    import matrix_corpus as mc
    text, offs, cut = mc.form(form)
    return run(text, offs, cut, MODE_OF[form], Voc(mc.vocabularies()[vocab]))


@functools.lru_cache(maxsize=None)
def trap_ref(form, lanes64):
    tokens, text, offs, cut = trap_batch(form, lanes64)
    return run(text, offs, cut, MODE_OF[form], Voc(tokens))


@functools.lru_cache(maxsize=None)
def far_ref(form):
    tokens, text, offs, cut = far_batch(form)
    return run(text, offs, cut, MODE_OF[form], Voc(tokens))
