"""dpt_word_compare_sizes / dpt_word_compare_write (csrc/dpt_words.hip) against the numpy model of tests/words_ref.py:
every output array for equality, each between guard words that must survive.  Synthetic word-index streams built on
the host at the sizes where the 64-word windows and 64-token chunks of the merge meet, both layouts on both sides,
statuses, malformed streams and short output ranges, waves that take many strings, and the real streams of
dpt_encode + dpt_token_spans against dpt_bpe_encode."""
import numpy as np
import pytest

import matrix_corpus as mc
import words_cases as wc
import words_ref as wr

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5                                   # what the outputs hold before a call
TOKENS = (0, 1, 63, 64, 65, 127, 128, 129, 200)     # per-side token counts
WORDS = (0, 1, 63, 64, 65, 130)                     # word counts
LAYOUTS = {"csr-csr": (False, False), "csr-padded": (False, True), "padded-csr": (True, False), "padded-padded": (True, True)}
KNOB = "DPT_WAVE_GRID_BLOCKS"
WAVES = 4


# ------------------------------------------------------------------ running the two calls

def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    if len(a) == 0:
        a = np.zeros(1, dtype=a.dtype)
    return torch.from_numpy(a.copy()).cuda()


class DeviceSide:
    """A words_ref side on the device; ``ptrs(lo)``: the addresses of the shard that starts at string lo."""

    def __init__(self, side):
        self.side = side
        self.t = {k: None if v is None else _dev(v) for k, v in side.items()}

    def ptrs(self, lo=0):
        first = int(self.side["off"][lo]) - int(self.side["off"][0])
        def at(k, size, n):
            return 0 if self.t[k] is None else self.t[k].data_ptr() + size * n
        return at("off", 8, lo), at("counts", 8, lo), at("status", 4, lo), at("tok_word", 4, first), at("tok_end", 4, first)


def shard_of(side, lo, hi):
    """The model's side for strings [lo, hi) of ``side``, as DeviceSide.ptrs(lo) hands it to the calls."""
    first = int(side["off"][lo]) - int(side["off"][0])
    return {"off": side["off"][lo:hi + 1], "counts": None if side["counts"] is None else side["counts"][lo:hi],
            "status": None if side["status"] is None else side["status"][lo:hi], "tok_word": side["tok_word"][first:],
            "tok_end": None if side["tok_end"] is None else side["tok_end"][first:]}


def _guarded(n):
    """n uint32 outputs between guard words, all holding FILL (one spare element: an empty array still has an address)."""
    import torch
    g = mc.Guarded(torch, n + 1, torch.int32, int(np.uint32(FILL).view(np.int32)))
    g.fill()
    return g


def _host(g, what):
    got, fine = g.host()
    assert fine and got.view(np.uint32)[-1] == FILL, "guard words of %s overwritten" % what
    return got[:-1].copy().view(np.uint32)


def run(da, db, n, flags, lo=0, word_counts=None, sel_counts=None, off0=(0, 0)):
    """Both calls over strings [lo, lo + n) of the device sides -> (sizes outputs, write outputs, word_off, sel_off) as
    the model names them.  ``word_counts`` / ``sel_counts``: the counts the write's offsets are made of instead of the
    sizes pass's own; ``off0``: where the two offset arrays start."""
    import torch
    from dptok import words
    pa, pb = da.ptrs(lo), db.ptrs(lo)
    names = ("n_words", "n_sel", "len_a", "len_b", "wc_status")
    g = {k: _guarded(n) for k in names}
    words.sizes_device(pa, pb, n, flags, g["n_words"].ptr(), g["n_sel"].ptr(), g["wc_status"].ptr(), len_a_ptr=g["len_a"].ptr(),
                       len_b_ptr=g["len_b"].ptr())
    torch.cuda.synchronize()
    sz = {k: _host(g[k], k) for k in names}
    sz["wc_status"] = sz["wc_status"].view(np.int32)
    word_off = wr.offsets(sz["n_words"] if word_counts is None else word_counts, off0[0])
    sel_off = wr.offsets(sz["n_sel"] if sel_counts is None else sel_counts, off0[1])
    n_w, n_s = int(word_off[-1] - word_off[0]), int(sel_off[-1] - sel_off[0])
    d_wo, d_so = _dev(word_off), _dev(sel_off)
    want_spans = da.t["tok_end"] is not None
    out = {k: _guarded(n_w) for k in ("cnt_a", "cnt_b")}
    out.update({k: _guarded(n_s) for k in wr.SEL_FIELDS if want_spans or k not in ("sel_begin", "sel_end")})
    out["wc_status"] = _guarded(n)
    def p(k):
        return out[k].ptr() if k in out else 0
    words.write_device(pa, pb, n, flags, p("wc_status"), word_off_ptr=d_wo.data_ptr(), cnt_a_ptr=p("cnt_a"), cnt_b_ptr=p("cnt_b"),
                       sel_off_ptr=d_so.data_ptr(), sel_str_ptr=p("sel_str"), sel_word_ptr=p("sel_word"), sel_begin_ptr=p("sel_begin"),
                       sel_end_ptr=p("sel_end"), sel_a_first_ptr=p("sel_a_first"), sel_a_count_ptr=p("sel_a_count"),
                       sel_b_first_ptr=p("sel_b_first"), sel_b_count_ptr=p("sel_b_count"))
    torch.cuda.synchronize()
    wrt = {k: _host(v, k) for k, v in out.items()}
    wrt["wc_status"] = wrt["wc_status"].view(np.int32)
    for k in names:                                                          # the write pass leaves the sizes outputs alone
        again = _host(g[k], k)
        assert np.array_equal(again.view(sz[k].dtype), sz[k]), k
    return sz, wrt, word_off, sel_off


def assert_sizes(sz, want):
    for k in ("wc_status", "n_words", "n_sel", "len_a", "len_b"):
        assert np.array_equal(sz[k], want[k]), (k, np.flatnonzero(sz[k] != want[k])[:10], sz[k][sz[k] != want[k]][:10], want[k][sz[k] != want[k]][:10])


def assert_write(wrt, want):
    assert np.array_equal(wrt["wc_status"], want["wc_status"]), np.flatnonzero(wrt["wc_status"] != want["wc_status"])[:10]
    for k in ("cnt_a", "cnt_b") + wr.SEL_FIELDS:
        if want[k] is None:
            assert k not in wrt
            continue
        keep = want["word_keep"] if k.startswith("cnt_") else want["sel_keep"]
        bad = np.flatnonzero(keep & (wrt[k] != want[k]))
        assert len(wrt[k]) == len(want[k]) and not len(bad), (k, bad[:10], wrt[k][bad[:10]], want[k][bad[:10]])


def check(a, b, flags, lo=0, hi=None, da=None, db=None):
    """Strings [lo, hi) of the sides through both calls and the model -> the model's answers."""
    hi = wr.n_strings(a) if hi is None else hi
    da, db = da or DeviceSide(a), db or DeviceSide(b)
    sa, sb = shard_of(a, lo, hi), shard_of(b, lo, hi)
    want = wr.sizes(sa, sb, flags)
    sz, wrt, word_off, sel_off = run(da, db, hi - lo, flags, lo=lo, off0=(lo, 3 * lo))
    assert_sizes(sz, want)
    want_w = wr.write(sa, sb, flags, word_off, sel_off, fill=FILL)
    assert_write(wrt, want_w)
    return want, want_w


# ------------------------------------------------------------------ the edge batch

def edge_pairs():
    """-> (streams a, streams b, status a, status b, what each pair is): every pairing of TOKENS that shares a word
    count of WORDS, the named shapes, the malformed streams between good neighbours, the statuses; shuffled."""
    rng = np.random.default_rng(411)
    recs = []

    def add(ca, cb, what, sa=0, sb=0):
        recs.append((wc.stream_of(ca), wc.stream_of(cb), sa, sb, what))

    for words in WORDS:
        for na in TOKENS:
            for nb in TOKENS:
                if words <= min(na, nb) and (words == 0) == (na == 0) and (words == 0) == (nb == 0):
                    add(wc.split_counts(rng, na, words), wc.split_counts(rng, nb, words), "pairing")
    add([1], [200], "long run")                                              # one run across three chunks (and a fourth)
    add([200], [1], "long run")
    add([1, 1, 1], [1, 198, 1], "long run")
    for words in (63, 64, 65, 130):
        add([1] * words, [1] * words, "none selected")                       # all one-token words
        add([1] * words, [2] * words, "all selected")
        add([3] * words, [1] * words, "all selected")
    base = np.ones(130, dtype=np.int64)
    for at in ([0], [63], [64], [129], [0, 63, 64, 129], [62, 65, 128]):
        more = base.copy()
        more[at] += 1
        add(base, more, "selected at")
        add(more + 1, base, "selected at")
    good_a, good_b = wc.split_counts(rng, 129, 65), wc.split_counts(rng, 200, 65)
    for kind in wc.MALFORMED:
        for at in (0.0, 63.5 / 200, 64.5 / 200, 128.5 / 200, 0.995):
            wa, wb = wc.malformed(kind, wc.stream_of(good_a), wc.stream_of(good_b), at)
            recs.append((wa, wb, 0, 0, kind))
            recs.append((wb, wa, 0, 0, kind))
    recs.append((np.array([1]), np.array([0]), 0, 0, "first_is_1"))
    recs.append((np.array([0]), np.zeros(0, np.int64), 0, 0, "words_differ"))
    recs.append((np.zeros(0, np.int64), np.array([0, 1]), 0, 0, "words_differ"))
    # a stream that passes the claimed word count and comes back to it: the defect lies behind the last word's run end
    recs.append((np.concatenate([np.arange(70), np.full(70, 69), [68, 68, 5]]), wc.stream_of([1] * 6), 0, 0, "decrease"))
    recs.append((wc.stream_of([2] * 6), np.array([0, 1, 2, 3, 4, 5] + [6] * 100 + [5]), 0, 0, "decrease"))
    recs.append((np.array([0xFFFFFFFF]), np.array([0xFFFFFFFF]), 0, 0, "first_is_1"))
    for sa, sb in ((1, 0), (0, 2), (6, 3), (0, 6), (4, 0)):
        for _ in range(4):
            add(wc.split_counts(rng, 129, 64), wc.split_counts(rng, 65, 64), "status", sa, sb)
        recs.append((np.zeros(0, np.int64), wc.stream_of([2, 2]), sa, sb, "status"))
    recs = [recs[i] for i in rng.permutation(len(recs))]
    return ([r[0] for r in recs], [r[1] for r in recs], np.array([r[2] for r in recs], dtype=np.int32),
            np.array([r[3] for r in recs], dtype=np.int32), [r[4] for r in recs])


@pytest.fixture(scope="module")
def edge():
    sa, sb, st_a, st_b, what = edge_pairs()
    n = len(sa)
    assert 270 <= n <= 340 and what.count("pairing") == 176
    rng = np.random.default_rng(412)
    ends = [wc.fake_ends(rng, w) for w in sa]
    slack = rng.integers(0, 5, size=n)
    sides = {}
    for name, (pad_a, pad_b) in LAYOUTS.items():
        a = wc.pack_side(sa, pad_a, status=st_a, off0=1_000_003 if pad_a else 77, slack=slack, ends=ends)
        b = wc.pack_side(sb, pad_b, status=st_b, off0=5 if pad_b else 0, slack=slack[::-1])
        sides[name] = (a, b)
    return {"sides": sides, "what": what, "n": n, "st": (st_a, st_b)}


@pytest.mark.parametrize("flags", [wr.LESS, wr.GREATER, wr.LESS | wr.GREATER])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_edge_batch(layout, flags, edge):
    a, b = edge["sides"][layout]
    want, want_w = check(a, b, flags)
    what, st = np.array(edge["what"]), want["wc_status"]
    bad = np.isin(what, wc.MALFORMED)
    assert (st[bad] == wr.INTERNAL).all() and bad.sum() >= 40               # each malformed pair, and it alone
    clean = ~bad & (edge["st"][0] == 0) & (edge["st"][1] == 0)
    assert (st[clean] == 0).all() and clean.sum() >= 200
    assert {1, 2, 6, 4} <= set(st[what == "status"].tolist())
    assert (want["n_sel"][what == "none selected"] == 0).all()
    full = what == "all selected"
    assert int((want["n_sel"][full] == want["n_words"][full]).sum()) == (8 if flags == 3 else 4) and full.sum() == 8
    assert want_w["sel_keep"].all() and want_w["word_keep"].all()


def test_selected_at_the_window_edges(edge):
    a, b = edge["sides"]["csr-padded"]
    want, want_w = check(a, b, wr.LESS)
    so = wr.offsets(want["n_sel"]).astype(np.int64)
    seen = {tuple(want_w["sel_word"][so[s]:so[s + 1]].tolist()) for s in np.flatnonzero(np.array(edge["what"]) == "selected at")}
    assert {(0,), (63,), (64,), (129,), (0, 63, 64, 129), (62, 65, 128), ()} == seen


def test_without_optional_arrays(edge):
    """No statuses, no tok_end (so no byte spans), no lengths."""
    from dptok import words
    import torch
    a, b = edge["sides"]["padded-csr"]
    a2 = dict(a, status=None, tok_end=None)
    b2 = dict(b, status=None)
    want, want_w = check(a2, b2, wr.LESS | wr.GREATER)
    assert want_w["sel_begin"] is None and want_w["sel_end"] is None
    da, db = DeviceSide(a2), DeviceSide(b2)
    n = edge["n"]
    g = {k: _guarded(n) for k in ("n_words", "n_sel", "wc_status")}
    words.sizes_device(da.ptrs(), db.ptrs(), n, 3, g["n_words"].ptr(), g["n_sel"].ptr(), g["wc_status"].ptr())
    torch.cuda.synchronize()
    for k in g:
        assert np.array_equal(_host(g[k], k).view(want[k].dtype), want[k]), k
    # the statuses alone from the write pass
    st = _guarded(n)
    words.write_device(da.ptrs(), db.ptrs(), n, 3, st.ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_host(st, "wc_status").view(np.int32), want["wc_status"])


@pytest.mark.parametrize("layout", ["csr-padded", "padded-csr"])
def test_shard_from_the_middle(layout, edge):
    a, b = edge["sides"][layout]
    da, db = DeviceSide(a), DeviceSide(b)
    n = edge["n"]
    for lo, hi in ((n // 3, 2 * n // 3), (n - 5, n), (7, 8)):
        check(a, b, wr.LESS, lo=lo, hi=hi, da=da, db=db)


@pytest.mark.parametrize("which", ["word", "sel"])
def test_short_ranges(which, edge):
    """A word_off / sel_off range one too short (and one too long): status 4 for that string alone, the neighbours'
    results exact, nothing outside the arrays."""
    a, b = edge["sides"]["csr-padded"]
    da, db = DeviceSide(a), DeviceSide(b)
    sz = wr.sizes(a, b, 3)
    victims = np.flatnonzero((sz["n_sel"] >= 2) & (sz["n_words"] >= 64))[[0, 3, -1]]
    counts = {"word": sz["n_words"].astype(np.int64), "sel": sz["n_sel"].astype(np.int64)}
    counts[which][victims[:2]] -= 1
    counts[which][victims[2]] += 1
    empty = np.flatnonzero(sz["n_words"] == 0)[0]                            # a range where the string has nothing
    counts[which][empty] += 2
    _, wrt, word_off, sel_off = run(da, db, edge["n"], 3, word_counts=counts["word"], sel_counts=counts["sel"], off0=(11, 13))
    want = wr.write(a, b, 3, word_off, sel_off, fill=FILL)
    hit = np.zeros(edge["n"], dtype=bool)
    hit[victims] = True
    hit[empty] = sz["wc_status"][empty] == 0
    assert np.array_equal(want["wc_status"] == wr.INTERNAL, hit | (sz["wc_status"] == wr.INTERNAL))
    assert_write(wrt, want)


@pytest.mark.parametrize("cap", [1, 3])
def test_capped_grid(cap, edge, monkeypatch):
    """4 and 12 waves for the whole batch: every wave takes many strings, of every kind after each other."""
    from dptok import _lib
    a, b = edge["sides"]["padded-csr"]
    da, db = DeviceSide(a), DeviceSide(b)
    monkeypatch.delenv(KNOB, raising=False)
    assert _lib.wave_grid(edge["n"], WAVES) == (edge["n"] + WAVES - 1) // WAVES
    free = run(da, db, edge["n"], 3)
    monkeypatch.setenv(KNOB, str(cap))
    assert _lib.wave_grid(edge["n"], WAVES) == cap and edge["n"] >= 8 * WAVES * cap
    capped = run(da, db, edge["n"], 3)
    for f, c in zip(free[:2], capped[:2]):
        assert f.keys() == c.keys()
        for k in f:
            assert np.array_equal(f[k], c[k]), k
    check(a, b, 3, da=da, db=db)                                             # (and both equal the model)


# ------------------------------------------------------------------ real streams

def _bloom_pairs():
    import gzip
    import os
    from bloom_fixture import HERE
    from dptok.bpe import pairs_from_tokenizer_json
    with gzip.open(os.path.join(HERE, "golden", "bloom_synth_tokenizer.json.gz"), "rb") as fh:
        return pairs_from_tokenizer_json(fh.read().decode("utf-8"))


def test_real_streams():
    """dpt_encode + dpt_token_spans (CSR) against dpt_bpe_encode (padded) on the matrix corpus' ATOMS form, all three
    and compare_device queued on a side stream with nothing in between: the counts are the bincounts of the two
    tok_word arrays, the byte spans the words of the cut mask."""
    import torch
    from dptok import Bpe, Encoder, Vocab, words
    t2i = mc.vocabularies()["base"]
    enc, bpe = Encoder(Vocab(t2i, 0)), Bpe(*_bloom_pairs(), device=0)
    text, offs, cut = mc.form("atoms")
    n, nb = len(offs) - 1, len(text)
    d_text, d_offs, d_cut = _dev(text), _dev(offs), _dev(cut)
    side_stream = torch.cuda.Stream()
    side_stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side_stream):
        sp = side_stream.cuda_stream
        ids, end, word = (torch.empty(nb, dtype=torch.int32, device="cuda") for _ in range(3))
        id_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        st, sst = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
        enc.encode_device(d_text.data_ptr(), nb, d_offs.data_ptr(), n, ids.data_ptr(), nb, id_off.data_ptr(), st.data_ptr(),
                          cut_ptr=d_cut.data_ptr(), stream=sp, mode="atoms")
        enc.spans_device(d_text.data_ptr(), nb, d_offs.data_ptr(), n, ids.data_ptr(), id_off.data_ptr(), st.data_ptr(), end.data_ptr(),
                         sst.data_ptr(), tok_word_ptr=word.data_ptr(), cut_ptr=d_cut.data_ptr(), stream=sp, mode="atoms")
        b_ids, b_cnt, b_st, b_word = bpe.encode_atoms(enc.vocab, d_text, d_offs, d_cut, tok_word=True)
        got = words.compare_device(words.Side(id_off, word, status=sst, tok_end=end),
                                   words.Side(d_offs, b_word, counts=b_cnt, status=b_st), words.WORDS_LESS | words.WORDS_GREATER)
        a_sel, a_sel_off = words.selected_ids(ids, id_off, None, got.sel_str, got.sel_a_first, got.sel_a_count)
        b_sel, b_sel_off = words.selected_ids(b_ids, d_offs, b_cnt, got.sel_str, got.sel_b_first, got.sel_b_count)
    side_stream.synchronize()
    h = {k: None if v is None else v.cpu().numpy() for k, v in got._asdict().items()}
    io, o = id_off.cpu().numpy(), offs.astype(np.int64)
    a_word, b_word_h, b_cnt_h = word.cpu().numpy(), b_word.cpu().numpy(), b_cnt.cpu().numpy()
    ids_h, b_ids_h = ids.cpu().numpy(), b_ids.cpu().numpy()
    a_sel, a_sel_off, b_sel, b_sel_off = (x.cpu().numpy() for x in (a_sel, a_sel_off, b_sel, b_sel_off))
    sst_h, bst_h = sst.cpu().numpy(), b_st.cpu().numpy()
    assert np.array_equal(h["status"], np.where(sst_h != 0, sst_h, bst_h)) and (h["status"] == 0).sum() > 200 and (h["status"] != 0).any()
    assert not (h["status"] == wr.INTERNAL).any()
    starts = mc.word_starts("atoms", text, cut)
    n_checked = 0
    for s in range(n):
        wa, wb = a_word[io[s]:io[s + 1]], b_word_h[o[s] - o[0]:][:b_cnt_h[s]]
        assert h["len_a"][s] == (len(wa) if sst_h[s] == 0 else 0) and h["len_b"][s] == (len(wb) if bst_h[s] == 0 else 0)
        r = slice(h["word_off"][s], h["word_off"][s + 1])
        if h["status"][s] != 0:
            assert h["n_words"][s] == 0 and h["n_sel"][s] == 0
            continue
        ca, cb = np.bincount(wa, minlength=0), np.bincount(wb, minlength=0)
        assert np.array_equal(h["cnt_a"][r], ca) and np.array_equal(h["cnt_b"][r], cb), s
        sel = np.flatnonzero(ca != cb)
        q = slice(h["sel_off"][s], h["sel_off"][s + 1])
        assert np.array_equal(h["sel_word"][q], sel) and (h["sel_str"][q] == s).all(), s
        ws = np.flatnonzero(starts[o[s]:o[s + 1]])
        ws = np.concatenate([[0], ws[ws > 0], [o[s + 1] - o[s]]]) if o[s + 1] > o[s] else np.zeros(1, dtype=np.int64)
        assert np.array_equal(h["sel_begin"][q], ws[sel]) and np.array_equal(h["sel_end"][q], ws[sel + 1]), s
        for d, w in zip(range(q.start, q.stop), sel):
            assert a_sel[a_sel_off[d]:a_sel_off[d + 1]].tolist() == ids_h[io[s]:io[s + 1]][wa == w].tolist()
            assert b_sel[b_sel_off[d]:b_sel_off[d + 1]].tolist() == b_ids_h[o[s] - o[0]:][:b_cnt_h[s]][wb == w].tolist()
        n_checked += len(sel)
    assert n_checked > 100
