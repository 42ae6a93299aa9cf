"""Token byte spans and word indices (include/dpt.h dpt_token_spans / dpt_token_spans_host) against
the pure-Python walk of tests/spans_ref.py, for equality: the corpus of tests/matrix_corpus.py in its
three forms, strings whose token counts sit on the kernel's 64-token and 64-byte chunk edges, the
device-path contract (a shard of a larger upload, offsets not rebased, unaligned text, a side
stream, no host synchronisation between the encode and the spans call, guarded outputs), ids that do
not tile their string, vocabularies without a per-id length table, and ``dp_tokenize.batch_spans``."""
import numpy as np
import pytest

import matrix_corpus as mc
import spans_ref

pytestmark = pytest.mark.gpu

SPAN_VOCABS = ("base", "long+40000")
HOLE = 20000   # the id no token of the holed vocabulary has


@pytest.fixture(scope="module")
def encoders():
    from dptok import Encoder, Vocab
    out = {name: Encoder(Vocab(mc.vocabularies()[name], 0)) for name in SPAN_VOCABS}
    assert min(out["long+40000"].vocab.t2i.values()) == mc.ID_SHIFT   # id_min != 0
    return out


def _assert_spans(got_end, got_word, got_ss, ref, what=""):
    rend, rword, rss = ref
    assert np.array_equal(got_ss, rss), (what, np.nonzero(got_ss != rss)[0][:10])
    assert np.array_equal(got_end, rend), (what, np.nonzero(got_end != rend)[0][:10])
    if got_word is not None:
        assert np.array_equal(got_word, rword), (what, np.nonzero(got_word != rword)[0][:10])


# ------------------------------------------------------------------ 1. the matrix corpus, host path

@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("vocab", SPAN_VOCABS)
def test_matrix_corpus_spans(vocab, form, encoders):
    enc = encoders[vocab]
    text, offs, cut = mc.form(form)
    ids, id_off, st, _, tok_end, tok_word, ss = enc.encode_csr_spans(text, offs, mode=form, cut_mask=cut)
    counts = np.diff(id_off.astype(np.int64))
    assert len(st) > 400 and counts.max() > 4000 and (st != 0).any()
    assert form != "raw" or (np.diff(offs.astype(np.int64)) == 0).any()   # (empty strings: status 2)
    assert tok_end.dtype == np.uint32 and tok_word.dtype == np.uint32 and len(tok_end) == len(tok_word) == len(ids)
    ref = spans_ref.expected(enc.vocab.t2i, form, text, offs, cut, ids, id_off, st)
    _assert_spans(tok_end, tok_word, ss, ref, (vocab, form))


# ------------------------------------------------------------------ 2. chunk edges

@pytest.fixture(scope="module")
def edge_batch():
    return build_edge_batch()


def build_edge_batch():
    """The strings, the llama-shaped engine, its whole-batch result and the walk's (test_gpu_wave_stride.py
    reorders them)."""
    from dptok import Encoder, Vocab, pack_strings, synth
    t2i = synth.llama_shaped_vocab()
    t, _ = synth.random_ascii_corpus(1, 400, seed=11)
    base = bytes(t).decode("ascii")
    strs = [base[:L] for L in range(1, 401)]
    strs += ["a" + "\n" * 300, "a" + " " * 300, "a" + " \n" * 150, "a\n", "a ", " x", "\nab"]
    strs += synth.unpack(*synth.arabic_corpus(64))
    text, offs = pack_strings(strs)
    enc = Encoder(Vocab(t2i, 0))
    got = enc.encode_csr_spans(text, offs)
    ids, id_off, st = got[:3]
    ref = spans_ref.expected(t2i, "raw", text, offs, None, ids, id_off, st)
    for a in ref:
        a.setflags(write=False)
    return {"strs": strs, "text": text, "offs": offs, "enc": enc, "got": got, "ref": ref, "t2i": t2i}


def test_chunk_edges_whole_batch(edge_batch):
    e = edge_batch
    ids, id_off, st, _, tok_end, tok_word, ss = e["got"]
    counts = np.diff(id_off.astype(np.int64))
    assert not st[:400].any()
    assert {63, 64, 65, 127, 128, 129} <= set(counts[:400].tolist())
    assert counts[400:405].tolist() == [301, 301, 301, 2, 2]
    assert st[405:407].tolist() == [1, 1] and counts[405:407].tolist() == [0, 0]   # " x", "\nab": nothing written
    assert not st[407:].any() and all(s.encode("utf-8")[0] >= 0x80 for s in e["strs"][407:])
    _assert_spans(tok_end, tok_word, ss, e["ref"])
    o = id_off.astype(np.int64)
    nl, sp = slice(o[400], o[401]), slice(o[401], o[402])
    assert tok_end[nl].tolist() == list(range(1, 302)) and not tok_word[nl].any()   # 6x expansion, one word
    assert tok_word[sp].tolist() == list(range(301))                                # 301 words


@pytest.mark.parametrize("n_str", [1, 5])
def test_chunk_edges_small_calls(n_str, edge_batch):
    """The 400 prefixes again, n_str strings per call: grids of one block with one to four busy waves
    and of two blocks, offsets that do not start at 0."""
    e = edge_batch
    ids, id_off, st = e["got"][:3]
    rend, rword, rss = e["ref"]
    o = id_off.astype(np.int64)
    for a in range(0, 400, n_str):
        b = a + n_str
        g = e["enc"].encode_csr_spans(e["text"], e["offs"][a:b + 1])
        assert np.array_equal(g[0], ids[o[a]:o[b]]), a
        _assert_spans(g[4], g[5], g[6], (rend[o[a]:o[b]], rword[o[a]:o[b]], rss[a:b]), a)


# ------------------------------------------------------------------ 3. the device-path contract

@pytest.fixture(scope="module")
def uploads():
    """form -> the upload of matrix_corpus in pinned host memory and its device buffers (offsets valid
    on the device, text and cut mask filled in by each call's own stream)."""
    torch = pytest.importorskip("torch")
    out = {}
    for f in mc.FORMS:
        text, offs, cut = mc.upload(f)
        h = {"text": torch.from_numpy(text.copy()).pin_memory(),
             "offs": torch.from_numpy(offs.view(np.int64).copy()).pin_memory(),
             "cut": None if cut is None else torch.from_numpy(cut.copy()).pin_memory()}
        d = {k: (None if t is None else torch.empty_like(t, device="cuda")) for k, t in h.items()}
        d["offs"].copy_(h["offs"])
        out[f] = (h, d, (text, offs, cut))
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def side_stream():
    torch = pytest.importorskip("torch")
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.default_stream().cuda_stream
    return s


S_END, S_WORD, S_SS = -0x5A5A5A5B, -0x3C3C3C3D, -0x2D2D2D2E


@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("vocab", SPAN_VOCABS)
def test_device_path_contract(vocab, form, encoders, uploads, side_stream):
    torch = pytest.importorskip("torch")
    enc = encoders[vocab]
    h, d, (text, offs, cut) = uploads[form]
    shards = mc.shards(form)
    assert {int(offs[lo]) % 4 for lo, _ in shards} >= {1, 2, 3}
    for lo, hi in shards:
        b0, b1 = int(offs[lo]), int(offs[hi])
        n, n_bytes = hi - lo, b1 - b0
        assert b0 != 0 and b1 < len(text)
        ids = torch.empty(n_bytes, dtype=torch.int32, device="cuda")
        id_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        st = torch.empty(n, dtype=torch.int32, device="cuda")
        # ids_cap elements each: the token count is not known before the encode has run
        end, word, ss = (mc.Guarded(torch, n_bytes, torch.int32, S_END), mc.Guarded(torch, n_bytes, torch.int32, S_WORD),
                         mc.Guarded(torch, n, torch.int32, S_SS))
        end2, ss2 = mc.Guarded(torch, n_bytes, torch.int32, S_END), mc.Guarded(torch, n, torch.int32, S_SS)
        enc.reserve(n_bytes, n)   # (the encode then allocates nothing: no implicit device synchronisation)
        d["text"].fill_(0x20)     # what the buffers held before must not survive
        if d["cut"] is not None:
            d["cut"].zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(side_stream):
            for k in ("text", "offs", "cut"):
                if d[k] is not None:
                    d[k].copy_(h[k], non_blocking=True)
            for g in (end, word, ss, end2, ss2):
                g.fill()
            tp, op = d["text"].data_ptr() + b0, d["offs"].data_ptr() + 8 * lo
            cp = 0 if d["cut"] is None else d["cut"].data_ptr() + b0
            sid = side_stream.cuda_stream
            enc.encode_device(tp, n_bytes, op, n, ids.data_ptr(), n_bytes, id_off.data_ptr(), st.data_ptr(), cut_ptr=cp,
                              stream=sid, mode=form)
            enc.spans_device(tp, n_bytes, op, n, ids.data_ptr(), id_off.data_ptr(), st.data_ptr(), end.ptr(), ss.ptr(),
                             tok_word_ptr=word.ptr(), cut_ptr=cp, stream=sid, mode=form)
            enc.spans_device(tp, n_bytes, op, n, ids.data_ptr(), id_off.data_ptr(), st.data_ptr(), end2.ptr(), ss2.ptr(),
                             tok_word_ptr=0, cut_ptr=cp, stream=sid, mode=form)
        side_stream.synchronize()   # that stream only
        h_ids, h_off, h_st = ids.cpu().numpy(), id_off.cpu().numpy().view(np.uint64), st.cpu().numpy()
        n_tok = int(h_off[-1])
        res = {}
        for k, g in (("end", end), ("word", word), ("ss", ss), ("end2", end2), ("ss2", ss2)):
            res[k], ok = g.host()
            assert ok, "guard zone of %s overwritten" % k
        for k, sentinel in (("end", S_END), ("word", S_WORD), ("end2", S_END)):
            assert (res[k][n_tok:] == sentinel).all(), "%s written past the last token" % k
        ref = spans_ref.expected(enc.vocab.t2i, form, text, offs[lo:hi + 1], cut, h_ids[:n_tok], h_off, h_st)
        _assert_spans(res["end"][:n_tok].view(np.uint32), res["word"][:n_tok].view(np.uint32), res["ss"], ref, (lo, hi))
        _assert_spans(res["end2"][:n_tok].view(np.uint32), None, res["ss2"], ref, (lo, hi, "tok_word NULL"))


# ------------------------------------------------------------------ 4. ids that do not tile their string

def test_foreign_ids_in_range():
    """One id of a string replaced by a token of another byte length, or by an id inside [id_min, id_max]
    that no token has: that string gets status 4, every other string its exact result, and nothing is
    stored outside the id ranges.  (Ids outside the table:
    test_gpu_wave_stride.py::test_spans_capped.)"""
    torch = pytest.importorskip("torch")
    from dptok import Encoder, Vocab
    t2i = {t: i + (1 if i >= HOLE else 0) for t, i in mc.vocabularies()["base"].items()}
    assert HOLE not in set(t2i.values()) and min(t2i.values()) < HOLE < max(t2i.values())
    enc = Encoder(Vocab(t2i, 0))
    text, offs, _ = mc.form("raw")
    ids, id_off, st, _ = enc.encode_csr(text, offs)
    ref = spans_ref.expected(t2i, "raw", text, offs, None, ids, id_off, st)
    o = id_off.astype(np.int64)
    counts = np.diff(o)
    inv = spans_ref.invert(t2i)
    by_len = {}
    for t, i in t2i.items():
        by_len.setdefault(len(t.encode("utf-8")), i)
    okc = np.where(st == 0, counts, 0)
    last = int(np.flatnonzero(okc > 0)[-1])
    big = np.flatnonzero(okc >= 130)
    small = np.flatnonzero((okc >= 2) & (okc <= 10))
    # (string, token index, "len": a token one byte longer or shorter / "hole")
    edits = [(int(big[0]), 100, "len"), (int(big[1]), 64, "hole"), (int(big[2]), int(okc[big[2]]) - 1, "len"),
             (int(small[0]), 0, "len"), (int(small[1]), 1, "hole"), (last, int(okc[last]) - 1, "hole"),
             (int(small[2]), 0, "hole")]
    assert len({s for s, _, _ in edits}) == len(edits)
    bad_ids = ids.copy()
    for s, k, kind in edits:
        n = len(inv[int(ids[o[s] + k])].encode("utf-8"))
        bad_ids[o[s] + k] = HOLE if kind == "hole" else by_len[n + 1 if n + 1 in by_len else n - 1]
    n_tok, n = len(ids), len(st)
    dev = {k: torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in
           (("text", text), ("offs", offs.view(np.int64)), ("ids", bad_ids), ("id_off", id_off.view(np.int64)), ("st", st))}
    end, word, ss = (mc.Guarded(torch, n_tok, torch.int32, S_END), mc.Guarded(torch, n_tok, torch.int32, S_WORD),
                     mc.Guarded(torch, n, torch.int32, S_SS))
    for g in (end, word, ss):
        g.fill()
    enc.spans_device(dev["text"].data_ptr(), len(text), dev["offs"].data_ptr(), n, dev["ids"].data_ptr(),
                     dev["id_off"].data_ptr(), dev["st"].data_ptr(), end.ptr(), ss.ptr(), tok_word_ptr=word.ptr())
    torch.cuda.synchronize()
    res = {}
    for k, g in (("end", end), ("word", word), ("ss", ss)):
        res[k], ok = g.host()
        assert ok, "guard zone of %s overwritten" % k
    victims = {s for s, _, _ in edits}
    want_ss = ref[2].copy()
    want_ss[sorted(victims)] = 4
    assert np.array_equal(res["ss"], want_ss), np.nonzero(res["ss"] != want_ss)[0][:10]
    keep = np.ones(n_tok, dtype=bool)
    for s in victims:
        keep[o[s]:o[s + 1]] = False   # (a status-4 string's entries are unspecified)
    assert np.array_equal(res["end"].view(np.uint32)[keep], ref[0][keep])
    assert np.array_equal(res["word"].view(np.uint32)[keep], ref[1][keep])


# ------------------------------------------------------------------ 5. vocabularies without a length table

@pytest.mark.parametrize("kind", ["two lengths on one id", "sparse ids"])
def test_unsupported_vocabulary(kind):
    torch = pytest.importorskip("torch")
    from dptok import DptError, Encoder, Vocab, pack_strings, synth
    from oracle import oracle
    t2i = dict(synth.toy_vocab())
    if kind == "sparse ids":
        t2i["▁th"] = 10_000_000                  # the id range exceeds 8 * n_tokens + 65536
    else:
        a, b = "e", "▁e"
        assert len(a.encode()) != len(b.encode()) and a in t2i and b in t2i
        t2i[b] = t2i[a]
    enc = Encoder(Vocab(t2i, 0))
    strs = synth.unpack(*synth.random_ascii_corpus(32, 64, seed=5)) + ["the tree", "e e", "then the"]
    assert enc.encode_strs(strs) == oracle.OracleVocab(t2i).encode_strs(strs)   # encodes as before
    text, offs = pack_strings(strs)
    with pytest.raises(DptError, match=r"dpt_token_spans_host failed \(-3\)"):
        enc.encode_csr_spans(text, offs)
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    with pytest.raises(DptError, match=r"dpt_token_spans failed \(-3\)"):
        enc.spans_device(z.data_ptr(), 1, z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr())


# ------------------------------------------------------------------ 6. the drop-in surface

def _raw_atomise(text, start, end):
    return "".join("▁" + c if i == 0 else "▁" if c == " " else "<0x0A>" if c == "\n" else c
                   for i, c in enumerate(text[:end]) if i >= start)


def _check_surface(dp_tokenize, cands, inv, atomise, same_text):
    """``batch_spans`` against ``batch`` on the candidates that tokenize; the others must raise what
    ``batch`` raises."""
    from dptok import TokenSpans
    good, bad = [], []
    for t in cands:
        try:
            dp_tokenize.batch([t])
            good.append(t)
        except (ValueError, IndexError) as exc:
            bad.append((t, type(exc)))
    assert len(good) >= 24 and any(not t.isascii() for t in good)
    spans = dp_tokenize.batch_spans(good)
    assert [s.ids for s in spans] == dp_tokenize.batch(good)
    for t, s in zip(good, spans):
        assert isinstance(s, TokenSpans) and len(s.ids) == len(s.offsets) == len(s.word_ids)
        if same_text:
            assert s.text == t
        if not s.ids:
            assert s.text == ""
            continue
        assert s.offsets[0][0] == 0 and s.offsets[-1][1] == len(s.text)
        assert all(a[1] == b[0] for a, b in zip(s.offsets, s.offsets[1:]))
        for i, (a, b) in zip(s.ids, s.offsets):
            assert atomise(s.text, a, b) == inv[i], (t, i, a, b)
        assert s.word_ids[0] == 0 and all(x <= y for x, y in zip(s.word_ids, s.word_ids[1:]))
    for t, exc in bad:
        with pytest.raises(exc):
            dp_tokenize.batch_spans([good[0], t])
    return good, bad, spans


SURFACE_TEXTS = ["the weather", "hello world", "ab\ncd  e", "OptimalLengthTokenization", "a", "two  spaces", "x\n\ny",
                 "trailing ", "tab\there", "1984 was a year, 2001 another."] + list(mc.SHOWCASE) + \
                ["a é ß 中文", "b 中a é中", "see 😀😀 now", "k 🤖 k", "one two three four", "Hello, World!", "x=y+z; // done",
                 "q 文😀é q", "it's 7:45", "under_score-dash", "A.B.C.", "zz 中文 zz", "é ß", "😀", "a😀b 🤖", "كتاب جديد", "ab 文😀é cd ef", "été 中", "ßß ßß", "the 中文 word", "q é q",
                 "mixed عربي text", "x 😀😀 y", "中", "文文 文", "é\né", "end 🤖"]


def test_batch_spans_raw():
    from fake_llama import FakeLlamaTokenizer
    from packages.tokenizer_utils import dp_tokenize_llama
    t2i = mc.vocabularies()["base"]
    dp_tokenize, _ = dp_tokenize_llama(FakeLlamaTokenizer(t2i), "raw")
    good, bad, spans = _check_surface(dp_tokenize, SURFACE_TEXTS + [" x", "", "abc Ω def"], spans_ref.invert(t2i), _raw_atomise,
                                      same_text=True)
    assert {exc for _, exc in bad} == {ValueError, IndexError}
    s = spans[good.index("ab\ncd  e")]
    assert s.word_ids == [0, 0, 0, 1, 2] and s.offsets == [(0, 2), (2, 3), (3, 5), (5, 6), (6, 8)]
    s = spans[good.index("a é ß 中文")]   # character offsets, not bytes
    assert s.offsets[-1][1] == 8 and s.word_ids[-1] == 3


def test_batch_spans_llama():
    from conftest import load_golden
    from fake_llama import FakeLlamaTokenizer
    from packages.tokenizer_utils import dp_tokenize_llama
    t2i = mc.vocabularies()["base"]
    dp_tokenize, _ = dp_tokenize_llama(FakeLlamaTokenizer(t2i))   # default 'llama'
    cands = SURFACE_TEXTS + [c["text"] for c in load_golden("compat_cases.json.gz")["llama_mode"]][:30]
    good, bad, spans = _check_surface(dp_tokenize, cands, spans_ref.invert(t2i), lambda text, a, b: text[a:b], same_text=False)
    s = spans[good.index("hello world")]
    assert s.text == "<s>▁hello▁world" and s.word_ids[0] == 0 and s.word_ids[-1] == 2   # the BOS piece is word 0


def test_batch_spans_bloom():
    import tempfile
    from bloom_fixture import bloom_texts, bloom_tokenizer, make_hf_cache
    from packages.tokenizer_utils import dp_tokenize_bloom
    with tempfile.TemporaryDirectory() as d:
        hf = make_hf_cache(d)
        tokz = bloom_tokenizer(hf)
        dp_tokenize, _ = dp_tokenize_bloom(tokz, hf)
        inv = {i: t for t, i in dp_tokenize.vocab_to_index.items()}
        good, bad, spans = _check_surface(dp_tokenize, bloom_texts(48), inv, lambda text, a, b: text[a:b], same_text=False)
        assert not bad and spans[good.index("")] == ([], [], [], "")
        words = [w for w, _ in tokz._tokenizer.pre_tokenizer.pre_tokenize_str("hello world")]
        s = spans[good.index("hello world")]
        assert s.text == "".join(words) and s.word_ids[-1] == len(words) - 1
