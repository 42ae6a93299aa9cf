"""TEST INFRASTRUCTURE: the vocabularies and the corpus of the kernel dispatch matrix.

``launch_encode`` picks an instantiation by lane variant (16- or 64-lane rows: the vocabulary's
``max_cp``), mode (RAW / PRESPLIT / ATOMS), staging width (int16 when every id is <= 32767), plain
call against by-product flags, and entry point; then come the 512-byte, the 2048-byte and the
unbounded pass.  Four vocabularies and one corpus in three forms reach every cell:

* ``base``: ``synth.llama_shaped_vocab()`` plus multi-byte tokens (ids 32000 and up, all <= 32767);
* ``long``: ``base`` plus 240 tokens of 17..64 code points (64-lane rows);
* ``base+40000`` / ``long+40000``: every id shifted by 40000 (int32 staging).

The corpus has words on both sides of the 256-, 512- and 2048-byte limits in every form, tokens
of 2-, 3- and 4-byte code points (also across the 256-byte window edge), characters outside every
vocabulary, and empty strings.  tests/test_matrix_corpus.py checks with the oracle alone that these
inputs do what this says.
"""
import functools
import random

import numpy as np

from dptok import pack_strings, synth

MULTIBYTE = ["é", "ß", "中", "文", "😀", "🤖", "中文", "é中", "😀😀", "▁中", "▁😀", "a中", "中a", "文😀é"]
LONG_LENGTHS = (17, 20, 24, 31, 40, 64)
ID_SHIFT = 40000
VOCAB_NAMES = ("base", "base+40000", "long", "long+40000")
FORMS = ("raw", "presplit", "atoms")
# a word's bytes (in the form's own text) -> the pass that holds it
PASSES = {"mid": (256, 512), "big": (512, 2048), "long": (2048, 1 << 62)}
NEWLINE_ATOM = "<0x0A>"


@functools.lru_cache(maxsize=None)
def vocabularies():
    """name -> t2i for the four vocabularies."""
    base = dict(synth.llama_shaped_vocab())
    assert len(base) == 32000 and max(base.values()) == 31999
    for t in MULTIBYTE:
        assert t not in base, t
        base[t] = len(base)
    long_ = dict(base)
    rng = np.random.default_rng(2)   # the recipe of test_gpu_parity.py::test_long_token_vocab_uses_64_lane_rows
    for L in LONG_LENGTHS:
        for _ in range(20):
            tok = "".join(chr(c) for c in rng.integers(0x61, 0x65, size=L))
            long_.setdefault(tok, len(long_))
            long_.setdefault("▁" + tok[:-1], len(long_))
    assert len(long_) == len(base) + 240 and max(long_.values()) <= 32767
    return {"base": base, "base+40000": {t: i + ID_SHIFT for t, i in base.items()},
            "long": long_, "long+40000": {t: i + ID_SHIFT for t, i in long_.items()}}


def long_token_list():
    """The long vocabularies' tokens of more than 16 code points without the '▁' siblings."""
    return sorted(t for t in vocabularies()["long"] if len(t) > 16 and not t.startswith("▁"))


def multibyte_ids(t2i):
    """ids of the tokens that contain a 3- or 4-byte code point other than '▁'."""
    return {i for t, i in t2i.items() if any(ord(c) >= 0x800 and c != "▁" for c in t)}


def long_ids(t2i):
    return {i for t, i in t2i.items() if len(t) > 16}


SHOWCASE = ["文😀é", "ab 文😀é cd", "中文 é中 😀😀 a中 中a", "x文😀é文😀éy 😀", "é ß 中 文 😀 🤖", "q 中文文😀é"]


@functools.lru_cache(maxsize=None)
def corpus(seed=1, long_tokens=None):
    """The strings, shuffled (a tuple; the same for every vocabulary).  ``long_tokens``: a tuple of
    long tokens, default ``long_token_list()``."""
    longs = list(long_tokens) if long_tokens is not None else long_token_list()
    rnd = random.Random(seed)
    abcd = "abcd"

    def ascii_word(n):
        return "".join(rnd.choice(synth.PRINTABLE) for _ in range(n))

    def abcd_word(n):
        return "".join(rnd.choice(abcd) for _ in range(n))

    out = []
    # A: ragged printable ASCII with spaces (a leading space fails in RAW: the atom '▁ ')
    for k in range(120):
        n = 0 if k == 0 else rnd.randint(0, 300)
        out.append("".join(" " if rnd.random() < 0.15 else rnd.choice(synth.PRINTABLE) for _ in range(n)))
    # B: words built from the long tokens
    for _ in range(120):
        ws = []
        for _ in range(rnd.randint(1, 11)):
            kind, t = rnd.randrange(5), rnd.choice(longs)
            if kind == 0:
                ws.append(t)
            elif kind == 1:
                ws.append(t + abcd_word(rnd.randint(1, 2)))
            elif kind == 2:
                ws.append(t[:-1])
            elif kind == 3:
                ws.append(t + rnd.choice(longs))
            else:
                ws.append(abcd_word(rnd.randint(1, 30)))
        out.append(" ".join(ws))
    # C: one word on each side of every pass limit, alone and inside a string
    for n in list(range(250, 259)) + list(range(509, 516)) + list(range(2044, 2051)) + [3000, 5000]:
        for w in (ascii_word(n), abcd_word(n)):
            out.append(w)
            out.append("ab cd " + w + " ef")
    # D: multi-byte tokens at and around the 256-byte window edge, and random mixes
    for k in range(250, 259):
        for ch in "é中😀":
            out.append(ascii_word(k) + ch + "xy " + ch * 3)
    pool = ["é", "ß", "ع", "中", "😀", " ", " ", "\n"] + list("etaoinshrdlu") + synth.PRINTABLE[:20]
    for _ in range(40):
        out.append(rnd.choice("etaoin") + "".join(rnd.choice(pool) for _ in range(rnd.randint(1, 120))))
    # E: characters outside every vocabulary (status 1 and its capped length)
    out += ["Ω", "abc Ω def", "字", "hello 字 world", "aΩb 中", ascii_word(300) + "字", "中文 Ω", "xy\nΩ"]
    # F: the smallest strings
    out += ["", " ", "   ", "\n", "a", " a", "a "]
    rnd.shuffle(out)
    # tokens of several code points, among them one of 9 bytes, at every tenth place: the ATOMS form
    # merges code points into one atom there
    for k, s in enumerate(SHOWCASE):
        out.insert(10 * k, s)
    return tuple(out)


def _trim(text, offs):
    return text[: int(offs[-1])].copy(), np.ascontiguousarray(offs, dtype=np.uint64)


def atoms_form(strings, seed=7):
    """ATOMS: words split at spaces, each opened by a '▁' atom, every code point an atom ('\\n' is the
    atom '<0x0A>').  Every tenth string merges adjacent pairs or triples of its atoms into one atom of
    2..12 bytes: up to three where the merged text is a ``base`` token, and sometimes one anywhere."""
    rnd = random.Random(seed)
    toks = set(vocabularies()["base"])
    parts, cuts, offs = [], [], [0]
    for si, s in enumerate(strings):
        words = [["▁"] + [NEWLINE_ATOM if c == "\n" else c for c in w] for w in s.split(" ")] if s else []
        if si % 10 == 0 and words:
            cands = [(wi, p, k) for wi, at in enumerate(words) for k in (2, 3) for p in range(len(at) - k + 1)
                     if NEWLINE_ATOM not in at[p:p + k]]
            good = [c for c in cands if "".join(words[c[0]][c[1]:c[1] + c[2]]) in toks]
            pick = rnd.sample(good, min(3, len(good)))
            if cands and rnd.random() < 0.3:
                pick.append(rnd.choice(cands))
            chosen, used = [], set()
            for wi, p, k in pick:
                span = {(wi, q) for q in range(p, p + k)}
                if not (span & used):
                    used |= span
                    chosen.append((wi, p, k))
            for wi, p, k in sorted(chosen, key=lambda c: (c[0], -c[1])):   # right to left within a word
                words[wi][p:p + k] = ["".join(words[wi][p:p + k])]
        n = 0
        for at in words:
            for k, a in enumerate(at):
                e = a.encode("utf-8")
                c = bytearray(len(e))
                c[0] = 3 if k == 0 else 2
                parts.append(e)
                cuts.append(bytes(c))
                n += len(e)
        offs.append(offs[-1] + n)
    text = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    cut = np.frombuffer(b"".join(cuts), dtype=np.uint8).copy()
    return text, np.array(offs, dtype=np.uint64), cut


@functools.lru_cache(maxsize=None)
def form(name, seed=1):
    """(text u8[n_bytes], offsets u64[n+1], cut mask u8[n_bytes] or None) of the corpus in one form."""
    strings = corpus(seed)
    text, offs = _trim(*pack_strings(strings))
    if name == "raw":
        return text, offs, None
    if name == "presplit":
        t, o, c = synth.llama_words(text, offs)
        return np.ascontiguousarray(t), np.ascontiguousarray(o, dtype=np.uint64), np.ascontiguousarray(c)
    if name == "atoms":
        return atoms_form(strings)
    raise KeyError(name)


def word_starts(name, text, cut):
    """bool per byte: a word starts here (string starts not included)."""
    if name == "raw":
        return text == 0x20
    if name == "presplit":
        return cut != 0
    return (cut & 1) != 0


def longest_words(name, text, offs, cut):
    """Per string the byte length of its longest word, in the form's own text (0: empty string)."""
    st = word_starts(name, text, cut).copy()
    o = offs.astype(np.int64)
    st[o[:-1][o[:-1] < o[-1]]] = True
    idx = np.flatnonzero(st)
    wl = np.diff(np.append(idx, o[-1]))
    out = np.zeros(len(o) - 1, dtype=np.int64)
    lo = np.searchsorted(idx, o[:-1], side="left")
    hi = np.searchsorted(idx, o[1:], side="left")
    for s in range(len(out)):
        if hi[s] > lo[s]:
            out[s] = wl[lo[s]:hi[s]].max()
    return out


def pass_of(nbytes):
    """The pass that holds a word of nbytes, or None for the first pass."""
    for k, (a, b) in PASSES.items():
        if a < nbytes <= b:
            return k
    return None


def oracle_mode(name):
    from oracle import oracle
    return {"raw": oracle.RAW, "presplit": oracle.PRESPLIT, "atoms": oracle.ATOMS}[name]


HEAD = np.frombuffer("Ω▁x".encode("utf-8"), dtype=np.uint8)          # 6 bytes; 5 are used below
TAIL = np.frombuffer(("Ω" * 32).encode("utf-8"), dtype=np.uint8)      # 64 bytes no vocabulary holds


def upload(name):
    """The form laid out as a sharded caller holds it: 5 foreign bytes, the corpus, 64 foreign bytes --
    (text, offsets of the corpus strings within it, cut mask or None).  No string starts at offset 0
    and none ends at the buffer's end."""
    text, offs, cut = form(name)
    head = HEAD[:5]
    t = np.concatenate([head, text, TAIL])
    c = None if cut is None else np.concatenate([np.full(5, 3, np.uint8), cut, np.full(len(TAIL), 3, np.uint8)])
    return t, offs + np.uint64(5), c


def shards(name):
    """Three (lo, hi) string ranges that partition the corpus, with the upload's offsets[lo] % 4 equal
    to 1, 2 and 3."""
    _, offs, _ = upload(name)
    n = len(offs) - 1
    cuts = [0]
    assert int(offs[0]) % 4 == 1
    for want, near in ((2, n // 3), (3, 2 * n // 3)):
        k = next(k for k in range(near, n) if int(offs[k]) % 4 == want and k > cuts[-1])
        cuts.append(k)
    cuts.append(n)
    return [(cuts[k], cuts[k + 1]) for k in range(3)]


# ------------------------------------------------------------------ device buffers (GPU tests only)

GUARD = 64


class Guarded:
    """A device array of n elements carved out of a larger tensor, GUARD sentinel elements before and
    after it.  ``fill`` runs on torch's current stream."""

    def __init__(self, torch, n, dtype, sentinel):
        self.n, self.sentinel = n, sentinel
        self.whole = torch.empty(n + 2 * GUARD, dtype=dtype, device="cuda")
        self.view = self.whole[GUARD:GUARD + n]

    def fill(self):
        self.whole.fill_(self.sentinel)

    def ptr(self):
        return self.view.data_ptr()

    def host(self):
        """(the array, True when both guard zones still hold the sentinel)."""
        w = self.whole.cpu().numpy()
        ok = bool((w[:GUARD] == self.sentinel).all() and (w[GUARD + self.n:] == self.sentinel).all())
        return w[GUARD:GUARD + self.n], ok
