"""TEST INFRASTRUCTURE: the builders of the adversarial raw-mode corpora of tests/test_gpu_parity.py, so that
tests/test_gpu_lean_edges.py can run the same inputs on a first-pass route of its choosing.  Every builder is seeded
and deterministic; tests/test_raw_corpora.py pins each to the SHA-256 of what the tests built inline before the move
(``corpus_digest`` / ``vocab_digest``)."""
import hashlib
import json

import numpy as np


def corpus_digest(text, offs, cut=None) -> str:
    """SHA-256 over the packed text as built (its padding byte included), '|', the offsets as uint64 (, '|', the mask)."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(text, dtype=np.uint8).tobytes())
    h.update(b"|")
    h.update(np.ascontiguousarray(offs).astype(np.uint64).tobytes())
    if cut is not None:
        h.update(b"|")
        h.update(np.ascontiguousarray(cut, dtype=np.uint8).tobytes())
    return h.hexdigest()


def vocab_digest(t2i) -> str:
    """conftest.vocab_sha's recipe: the (token, id) pairs in the dict's order."""
    return hashlib.sha256(json.dumps(list(t2i.items()), ensure_ascii=False).encode()).hexdigest()


def _csr(texts):
    from dptok import pack_strings
    return pack_strings(texts)


# ---------------------------------------------------------------- test_ascii_windows_phase_a0
def a0_corpus():
    """Control bytes, '\\n' next to spaces, runs of spaces, words cut by the 256-byte windows -> (text, offs)."""
    rng = np.random.default_rng(23)
    pool = [chr(c) for c in range(0x20, 0x7F)] * 3 + ["\n", "\t", "\x01", "\x7f", "  ", " \n", "\n "]
    texts = []
    for k in range(3000):
        n = int(rng.integers(0, 900)) if k % 4 else int(rng.integers(200, 320))
        texts.append("".join(rng.choice(pool, size=n)))
    texts += ["\n" * 300, " " * 300, "a" * 600, ("ab " * 200), "\t" * 257]
    return _csr(texts)


# ---------------------------------------------------------------- test_ascii_walker_and_token_hash
def walker_case(seed):
    """A vocabulary of long letter tokens and newline-bearing tokens (seed 32: without '▁' itself) and
    multi-window strings over its letters -> (t2i, text, offs)."""
    rng = np.random.default_rng(seed)
    letters = "etaoinsh"
    vocab = set(letters) | {"▁" + c for c in letters} | {"<0x0A>", "\n"}
    if seed == 31:
        vocab.add("▁")
    for _ in range(3000):
        L = int(rng.integers(2, 17))
        w = "".join(rng.choice(list(letters), size=L))
        r = rng.random()
        if r < 0.3:
            w = "▁" + w[:15]
        elif r < 0.4:
            k = int(rng.integers(0, len(w)))
            w = (w[:k] + "<0x0A>" + w[k:])[:16]
        vocab.add(w)
    vocab = sorted(vocab)
    t2i = {t: i for i, t in enumerate(vocab)}
    texts = []
    for k in range(2500):
        n = int(rng.integers(1, 700))
        ch = rng.choice(list(letters) + [" "] * 2 + ["\n"] * (1 if k % 3 else 0), size=n)
        texts.append("".join(ch))
    texts += ["\n" + "etao" * 50, " " + "e" * 300, "\n\n\n", "e\ne\ne", " \nabc"]
    text, offs = _csr(texts)
    return t2i, text, offs


# ---------------------------------------------------------------- test_tie_heavy_long_words_vs_oracle
def tie_heavy_cases(n_vocab=30, n_strings=400):
    """Tie-heavy capless vocabularies over {a,b,c}, each with ``n_strings`` long words: yields (t2i, text, offs).
    One generator runs through all of them, so the first k cases are the same whatever ``n_vocab`` is."""
    from test_lane_model import tie_heavy_case
    rng = np.random.default_rng(21)
    for _ in range(n_vocab):
        vocab, _ = tie_heavy_case(rng)
        t2i = {t: i for i, t in enumerate(vocab)}
        texts = [tie_heavy_case(rng, max_len=256)[1] for _ in range(n_strings)]
        text, offs = _csr(texts)
        yield t2i, text, offs


# ---------------------------------------------------------------- test_long_words_big_window
def long_word_texts():
    """Printable words of 255..20000 bytes (the 2048-byte and unbounded passes), alone and inside strings."""
    rng = np.random.default_rng(5)
    texts = []
    for L in (255, 256, 257, 300, 700, 1500, 2047, 2048, 2049, 3000, 5000, 20000):
        w = "".join(chr(c) for c in rng.integers(0x21, 0x7F, size=L))
        texts.append(w)
        texts.append("ab cd " + w + " ef")
        texts.append(w + " " + w[: L // 2])
        texts.append(("\n" + w[:L // 3] + " x\n").join([w[:100], w[100:]]))
    return texts


def long_words_corpus():
    return _csr(long_word_texts())


# ---------------------------------------------------------------- test_mid_pass_words_257_to_512_bytes
def mid_pass_strings():
    """600 strings of 1..3 words, 60 % of them 200..530 bytes long, every other string's later words with a
    '▁' marker -> list of word lists."""
    rng = np.random.default_rng(41)
    alpha = [chr(c) for c in range(0x21, 0x7F)]
    strings = []
    for k in range(600):
        words = []
        for _ in range(int(rng.integers(1, 4))):
            L = int(rng.integers(200, 531)) if rng.random() < 0.6 else int(rng.integers(1, 40))
            w = "".join(rng.choice(alpha, size=L))
            words.append(("▁" + w) if (words and k % 2) else w)
        strings.append(words)
    return strings


def mid_pass_presplit(strings):
    """PRESPLIT form: the words as UTF-8 text + a word-start mask -> (text, offs, cut)."""
    parts, cuts = [], []
    for words in strings:
        b = bytearray(); c = bytearray()
        for w in words:
            e = w.encode("utf-8")
            c += b"\x01" + b"\x00" * (len(e) - 1)
            b += e
        parts.append(bytes(b)); cuts.append(bytes(c))
    offs = np.zeros(len(parts) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    text = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    cut = np.frombuffer(b"".join(cuts), dtype=np.uint8).copy()
    return text, offs, cut


def mid_pass_atoms(strings):
    """ATOMS form: the same words, every code point an atom -> (text, offs, cut)."""
    from dptok.engine import pack_word_atoms
    return pack_word_atoms([[list(w) for w in words] for words in strings])


def mid_pass_raw(strings):
    """RAW form (the lean-route tests'; the parity test has none): each string's words joined by single spaces, so
    the 200..530-byte words meet the raw first pass's 256-byte windows and every '▁' marker is non-ASCII text."""
    return _csr([" ".join(words) for words in strings])


# ---------------------------------------------------------------- test_work_partitions_vs_oracle
def work_partition_parts(n):
    """n ragged strings of 0..64 random ASCII bytes, 2 % of them empty, as bytes."""
    from dptok import synth
    rng = np.random.default_rng(n)
    text, offs = synth.random_ascii_corpus(n, 64, seed=n)
    cut = rng.integers(0, 65, size=n)
    cut[rng.random(n) < 0.02] = 0
    return [text[i * 64:i * 64 + int(cut[i])].tobytes() for i in range(n)]


def pack_parts(parts):
    """bytes strings back to back, one padding NUL -> (text, offs)."""
    offs = np.zeros(len(parts) + 1, np.uint64)
    offs[1:] = np.cumsum([len(p) for p in parts])
    text = np.frombuffer(b"".join(parts) + b"\0", np.uint8)
    return text, offs


def work_partition_corpus(n):
    return pack_parts(work_partition_parts(n))
