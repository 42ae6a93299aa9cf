"""Device-side default (greedy BPE) encoding (include/dpt.h dpt_bpe_encode) against the plain-Python rule of
tests/bpe_ref.py and against the real tokenizers: ids, counts, status and tok_word, every output between 0xAA
canaries.  The certified llama texts, both BLOOM fixtures, the call shapes of the device contract, toy tables that
separate the rule from its look-alikes, words on the LDS window's edges and beyond it, and several strings per wave."""
import json
import os
import random
import tempfile

import numpy as np
import pytest

import bpe_harness
import bpe_ref
import bytelevel_ref as br
import pretok_ref as pr

pytestmark = pytest.mark.gpu

LITERALS = [b"<unk>", b"<s>", b"</s>"]
W = 256          # csrc/dpt_bpe.hip W_LDS: words of up to W atoms always merge in LDS
WIN = W + 128    # ... WIN: the window's slots


class Case:
    """A vocabulary and its pair table on the device, with the model's view of both."""

    def __init__(self, t2i, pairs):
        from dptok import Bpe, Vocab
        self.vocab, self.bpe = Vocab(t2i, 0), Bpe(*pairs, device=0)
        self.pid, self.table = bpe_ref.piece_ids(t2i), bpe_ref.table_of(*pairs)

    def check(self, lens, text2, cut, **kw):
        return bpe_harness.check(self.bpe, self.vocab, self.pid, self.table, np.asarray(lens, dtype=np.int64), text2, cut, **kw)

    def check_words(self, strings, **kw):
        """strings: words of atoms (str) per string."""
        from dptok.pack import pack_word_atoms
        text, offs, cut = pack_word_atoms(strings)
        nb = int(offs[-1])
        return self.check(np.diff(offs.astype(np.int64)), text.tobytes()[:nb], cut.tobytes()[:nb], **kw)


@pytest.fixture(scope="module")
def llama():
    pytest.importorskip("sentencepiece")
    from dptok.bpe import pairs_from_scores
    from sp_llama import SPLlama
    tok = SPLlama()
    sp, t2i = tok.sp, tok.get_vocab()
    n = sp.get_piece_size()
    exclude = [i for i in range(n) if sp.is_control(i) or sp.is_unknown(i) or sp.is_unused(i) or sp.is_byte(i)]
    pairs = pairs_from_scores(t2i, {sp.id_to_piece(i): sp.get_score(i) for i in range(n)}, exclude)
    return Case(t2i, pairs), pr.build_table(pr.vocab_pieces(t2i), b"<s>", LITERALS), tok


def _bloom(big):
    from bloom_fixture import SNAPSHOT, bloom_tokenizer, make_hf_cache
    from dptok.bpe import pairs_from_tokenizer_json
    with tempfile.TemporaryDirectory() as d:
        hf = make_hf_cache(d, big=big)
        tok = bloom_tokenizer(hf)
        with open(os.path.join(hf, SNAPSHOT, "tokenizer.json"), encoding="utf-8") as fh:
            doc = fh.read()
    return Case(json.loads(doc)["model"]["vocab"], pairs_from_tokenizer_json(doc)), tok


# ------------------------------------------------------------------ 1. the recorded texts

def test_llama_certified_texts(llama):
    from sp_llama import hf_llama, llama_texts
    case, table, tok = llama
    texts = llama_texts()
    st, ln, text2, cut = bpe_ref.atoms(table, [t.encode("utf-8", "surrogatepass") for t in texts])
    keep = [t for t, s in zip(texts, st) if s == 0]
    assert len(keep) == 292
    want = case.check(ln[st == 0], text2, cut)
    hf = hf_llama()
    for t, (status, ids, words) in zip(keep, want):
        assert status == 0 and ids == tok.encode(t) == list(hf.encode(t)), t
    assert max(len(w[1]) for w in want) > 100
    case.check(ln[st == 0], text2, cut, want=want, pad=1, off0=0, tok_word=False)


@pytest.mark.parametrize("big", [False, True])
def test_bloom_fixtures(big):
    from bloom_fixture import big_vocab, bloom_big_texts, bloom_texts
    case, tok = _bloom(big)
    texts = bloom_big_texts(big_vocab()) if big else bloom_texts()
    st, ln, text2, cut = br.split(br.build_table(br.BLOOM_SEPARATORS), [t.encode("utf-8") for t in texts])
    assert not st.any() and len(texts) == (400 if big else 300)
    want = case.check(ln, text2, cut)
    for t, (status, ids, words) in zip(texts, want):
        assert status == 0 and ids == list(tok.encode(t)), t
    assert sum(len(w[1]) for w in want) > 3000


# ------------------------------------------------------------------ 2. toy tables

def _toy(tokens, merges):
    """tokens: the vocabulary in id order; merges: (left, right, rank) by token text."""
    t2i = {t: i for i, t in enumerate(tokens)}
    pairs = ([t2i[a] for a, b, _ in merges], [t2i[b] for a, b, _ in merges], [t2i[a + b] for a, b, _ in merges], [r for _, _, r in merges])
    return Case(t2i, pairs), t2i


def test_toy_tables():
    # merging every local minimum at once is not the rule
    case, t2i = _toy(["p", "q", "r", "s", "pq", "pqr", "rs"], [("p", "q", 0), ("pq", "r", 1), ("r", "s", 2)])
    want = case.check_words([[list("pqrs")], [list("pqrs"), list("rs"), list("sr")], [list("qrs")]])
    assert want[0][1] == [t2i["pqr"], t2i["s"]] and want[1][2] == [0, 0, 1, 2, 2] and want[2][1] == [t2i["q"], t2i["rs"]]
    # the same pair overlapping itself
    case, t2i = _toy(["a", "aa", "aaaa"], [("a", "a", 0), ("aa", "aa", 1)])
    want = case.check_words([[["a"] * n] for n in range(2, 10)] + [[["a"] * 3, ["a"] * 5, ["a"]]])
    assert want[1][1] == [t2i["aa"], t2i["a"]] and want[2][1] == [t2i["aaaa"]] and want[7][1] == [t2i["aaaa"]] * 2 + [t2i["a"]]
    # two different pairs of equal rank in one word: the leftmost goes first
    case, t2i = _toy(["a", "b", "c", "ab", "bc"], [("a", "b", 5), ("b", "c", 5)])
    want = case.check_words([[list("abc")], [list("cbcabc")], [list("bcbc"), list("abab")]])
    assert want[0][1] == [t2i["ab"], t2i["c"]] and want[1][1] == [t2i["c"], t2i["bc"], t2i["ab"], t2i["c"]]
    case, t2i = _toy(["a", "b", "c", "ab", "bc"], [("b", "c", 5), ("a", "b", 5)])          # (whatever the table's order)
    assert case.check_words([[list("abc")]])[0][1] == [t2i["ab"], t2i["c"]]
    # a product that merges again with its left and with its right neighbour, and a new pair that ranks below all others
    case, t2i = _toy(["x", "b", "c", "y", "bc", "xbc", "xbcy", "bcy"],
                     [("b", "c", 3), ("x", "bc", 1), ("xbc", "y", 0), ("bc", "y", 2)])
    want = case.check_words([[list("xbcy")], [list("bcy")], [list("xbc")], [list("ybcx"), list("xbcybcy")]])
    assert [w[1] for w in want[:3]] == [[t2i["xbcy"]], [t2i["bcy"]], [t2i["xbc"]]]
    assert want[3][1] == [t2i["y"], t2i["bc"], t2i["x"], t2i["xbcy"], t2i["bcy"]]


# ------------------------------------------------------------------ 3. call shapes

def test_call_shapes(llama):
    import torch
    case, table, _ = llama
    strings = [b"", b"hello world", b"", b"", b"x", b"a b  c\n", "café 中".encode(), b""]
    st, ln, text2, cut = bpe_ref.atoms(table, strings)
    assert not st.any()
    for kw in ({}, {"pad": 1, "off0": 0}, {"pad": 2, "off0": (1 << 33) + 5}, {"tok_word": False}, {"pad": 5, "tok_word": False}):
        want = case.check(ln, text2, cut, **kw)
    assert want[0] == (0, [1], [0]) and want[4][1][0] == 1 and want[4][2][-1] == 1   # "": the BOS alone
    # empty strings, and a string of one atom
    no_bos = table._replace(bos=b"")
    st, ln, text2, cut = bpe_ref.atoms(no_bos, [b"", b"", b"abc", b""])
    assert ln.tolist()[:2] == [0, 0] and case.check(ln, text2, cut)[0] == (0, [], [])
    want = case.check([0, 0, 0], b"", b"")
    assert want == [(0, [], [])] * 3
    ws = pr.WS
    assert case.check([3, 1, 3], ws + b"a" + ws, bytes([3, 0, 0, 3, 3, 0, 0]))[1] == (0, [case.pid[b"a"]], [0])
    # an atom that is no token: status 1, count 0, the neighbours exact -- a long atom, a short one, one at the end
    junk = [(b"<s>" + ws + b"ab", bytes([3, 0, 0, 3, 0, 0, 2, 2])),
            (b"<s>" + ws + b"ab", bytes([3, 0, 0, 3, 0, 0, 2, 0])),                      # "ab" as one atom: a piece? no
            (b"<s>" + ws + b"\x01b", bytes([3, 0, 0, 3, 0, 0, 2, 2])),
            (b"<s>x" + ws + b"b", bytes([3, 0, 0, 0, 3, 0, 0, 2])),                       # "<s>x"
            (b"q" * 80 + ws, bytes([3] + [0] * 79 + [3, 0, 0])),                         # an 80-byte atom
            (ws + b"b\xff", bytes([3, 0, 0, 2, 2])),
            (b"<s>" + ws + b"hello", bytes([3, 0, 0, 3, 0, 0, 2, 2, 2, 2, 2]))]
    lens = [len(a) for a, _ in junk]
    want = case.check(lens, b"".join(a for a, _ in junk), b"".join(b for _, b in junk))
    assert [w[0] for w in want] == [0, 0 if b"ab" in case.pid else 1, 1, 1, 1, 1, 0]
    # a mask of zeros, of threes, of ones: a string's first byte opens a word whatever its mask says
    for m in (0, 3, 1, 2):
        case.check([3, 5], ws + b"hello", bytes([m] * 8))
    # n_str == 0 launches nothing
    canary = torch.full((64,), 0xAA, dtype=torch.uint8, device="cuda:0")
    p = canary.data_ptr()
    case.bpe.encode_padded_device(case.vocab, p, 8, p, p, 0, p, 8, p, p, p)
    torch.cuda.synchronize()
    assert bool((canary == 0xAA).all())
    from dptok import DptError
    with pytest.raises(DptError):
        case.bpe.encode_padded_device(case.vocab, p, 8, p, p, 1, p, 7, p, p, p)
    # from torch tensors, on a side stream
    s = torch.cuda.Stream()
    st, ln, text2, cut = bpe_ref.atoms(table, [b"the weather", b"", b"is fine"])
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(ln.astype(np.int64))])).cuda()
    with torch.cuda.stream(s):
        ids, counts, status, words = case.bpe.encode_atoms(case.vocab, torch.from_numpy(np.frombuffer(text2, dtype=np.uint8).copy()).cuda(),
                                                           offs, torch.from_numpy(np.frombuffer(cut, dtype=np.uint8).copy()).cuda(), tok_word=True)
    s.synchronize()
    want = bpe_ref.encode(case.pid, case.table, ln, text2, cut)
    o = offs.cpu().numpy()
    assert [ids[int(a):int(a) + int(c)].cpu().tolist() for a, c in zip(o[:-1], counts.cpu())] == [w[1] for w in want]
    assert not status.cpu().numpy().any() and words[:int(counts[0])].cpu().tolist() == want[0][2]


# ------------------------------------------------------------------ 4. window edges

def _word(table, letters):
    """The ATOMS form of one llama word of len(letters) + 1 atoms (U+2581 first), without BOS."""
    st, text2, cut = bpe_ref.atoms_one(table._replace(bos=b""), letters.encode())
    assert st == 0 and sum(1 for c in cut if c) == len(letters) + 1
    return text2, cut


def test_window_edges(llama):
    case, table, _ = llama
    rnd = random.Random(11)
    rand = lambda k: "".join(rnd.choice("etaoinshrdlucmfwypvbgkjqxz") for _ in range(k))   # noqa: E731
    items = []
    for atoms in (W - 1, W, W + 1, WIN - 64, WIN - 63, WIN - 1, WIN, WIN + 1, 2 * W + 3):
        items += [_word(table, "a" * (atoms - 1)), _word(table, rand(atoms - 1))]
    # words that straddle the window: short words up to its flush mark, then a word across it; a long word between
    # short ones; a long word that ends exactly on a round's edge
    for lead, tail in ((300, 40), (318, 5), (100, W), (0, 700), (319, 700)):
        sent = " ".join([rand(3)] * (lead // 4) + [rand(tail), rand(5), "a" * tail, rand(2)])
        st, text2, cut = bpe_ref.atoms_one(table, sent.encode())
        assert st == 0
        items.append((text2, cut))
    st, text2, cut = bpe_ref.atoms_one(table, ("ab " * 150 + rand(64 * 8 - 1) + " " + rand(64 * 7)).encode())
    items.append((text2, cut))
    lens = [len(a) for a, _ in items]
    t2, c2 = b"".join(a for a, _ in items), b"".join(b for _, b in items)
    want = case.check(lens, t2, c2)
    assert all(w[0] == 0 for w in want) and len(want[1][1]) > 50
    case.check(lens, t2, c2, want=want, pad=1, off0=0, tok_word=False)


@pytest.mark.parametrize("kind", ["a", "random"])
def test_word_of_5000_atoms(kind, llama):
    case, table, _ = llama
    rnd = random.Random(5)
    letters = "a" * 4999 if kind == "a" else "".join(rnd.choice("etaoinshrdlucmfwypvbgkjqxz") for _ in range(4999))
    st, text2, cut = bpe_ref.atoms_one(table, ("on " + letters + " off").encode())
    assert st == 0
    want = case.check([len(text2)], text2, cut)
    assert want[0][2][-1] == 3 and want[0][2].count(2) > 300


# ------------------------------------------------------------------ 5. several strings per wave

@pytest.mark.parametrize("cap", [1, 3])
def test_strings_share_a_wave(cap, llama, monkeypatch):
    from dptok import _lib
    from sp_llama import llama_texts
    case, table, _ = llama
    rnd = random.Random(cap)
    strings = [t.encode("utf-8", "surrogatepass") for t in llama_texts()]
    st, ln, text2, cut = bpe_ref.atoms(table, strings)
    items, o = [], 0
    for n in ln[st == 0].tolist():
        items.append((text2[o:o + n], cut[o:o + n]))
        o += n
    items += [(b"", b"")] * 20 + [(b"<s>\x01", bytes([3, 0, 0, 2]))] * 20 + [_word(table, "a" * 400)] * 3   # empty, failing, long
    rnd.shuffle(items)
    lens = [len(a) for a, _ in items]
    t2, c2 = b"".join(a for a, _ in items), b"".join(b for _, b in items)
    want = bpe_ref.encode(case.pid, case.table, lens, t2, c2)
    assert sum(w[0] for w in want) == 20
    monkeypatch.setenv("DPT_WAVE_GRID_BLOCKS", str(cap))
    assert _lib.wave_grid(len(items), 4) == cap and len(items) >= 8 * 4 * cap
    case.check(lens, t2, c2, want=want)
