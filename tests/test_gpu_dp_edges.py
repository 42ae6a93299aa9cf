"""The DP by-products of dpt_dp_host / dpt_dp_host_far -- status, capped and uncapped lengths, the
per-atom-end edge masks and the far pairs -- bit-exact against tests/dp_ref.py (a plain Python reference;
tests/test_dp_ref.py pins it and the inputs' conditions without a GPU).

Cells: every vocabulary x form of tests/matrix_corpus.py x {capped, uncapped}, the whole corpus in one
call; then the calls with edges and no far list, uncapped lengths without edges, one sharded call per
form through the C ABI with str_off[0] != 0, small call shapes, the cap-trap batch (where the capped and
the uncapped DP differ in every pass) and the far-pair batch with the DPT_E_CAP protocol.

Masks are compared at every atom end of every string of status 0 or 1.  Entries of ``edges`` that are no
atom end of any string (the tail of a string with multi-byte atoms, a string of status 2) are not part of
the contract and stay unasserted."""
import ctypes
import time

import numpy as np
import pytest

import dp_ref
import matrix_corpus as mc

pytestmark = pytest.mark.gpu

CELLS = [(v, f, u) for v in mc.VOCAB_NAMES for f in mc.FORMS for u in (False, True)]
CANARY = 0xA5A5A5A5A5A5A5A5
TIMES = {"reference": 0.0, "start": time.time()}


def _base(vocab):
    return vocab.split("+")[0]


@pytest.fixture(scope="module")
def refs():
    """The reference on the corpus, once per (base | long, form): the +40000 vocabularies share it."""
    t0 = time.time()
    out = {(v, f): dp_ref.corpus_ref(v, f) for v in ("base", "long") for f in mc.FORMS}
    TIMES["reference"] += time.time() - t0
    yield out
    print("\ndp edges module: %.1f s wall, of which the reference fixtures %.1f s"
          % (time.time() - TIMES["start"], TIMES["reference"]))


@pytest.fixture(scope="module")
def encoders():
    from dptok import Encoder, Vocab
    out = {}
    for name, t2i in mc.vocabularies().items():
        v = Vocab(t2i, 0)
        assert (v.stats["max_cp"] > 16) == name.startswith("long"), (name, v.stats)
        out[name] = Encoder(v)
    return out


def _small_ref(fn, *args):
    t0 = time.time()
    r = fn(*args)
    TIMES["reference"] += time.time() - t0
    return r


def _check(ref, k, status, lengths, edges=None, tag=""):
    assert np.array_equal(status, ref.status[k]), (tag, np.flatnonzero(status != ref.status[k])[:10])
    assert np.array_equal(lengths, ref.lengths[k]), (tag, np.flatnonzero(lengths != ref.lengths[k])[:10])
    if edges is not None:
        assert edges.dtype == np.uint64 and len(edges) >= ref.n_bytes
        diff = dp_ref.compare_masks(edges, ref, k, np.flatnonzero(ref.status[k] <= 1))
        assert diff is None, (tag, "first differing (string, atom, got, want)", diff)


@pytest.mark.parametrize("vocab,form,uncapped", CELLS)
def test_corpus_cell(vocab, form, uncapped, encoders, refs):
    enc, ref, k = encoders[vocab], refs[_base(vocab), form], int(uncapped)
    text, offs, cut = mc.form(form)
    st, ln, ed, far = enc.dp(text, offs, mode=form, cut_mask=cut, uncapped=uncapped, edges=True, far=True)
    _check(ref, k, st, ln, ed, "dpt_dp_host_far")
    assert far.shape == (0, 2)      # no token of these vocabularies has more than 64 code points
    st, ln, ed = enc.dp(text, offs, mode=form, cut_mask=cut, uncapped=uncapped, edges=True)
    _check(ref, k, st, ln, ed, "dpt_dp_host")


@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("vocab", mc.VOCAB_NAMES)
def test_uncapped_lengths_without_edges(vocab, form, encoders, refs):
    text, offs, cut = mc.form(form)
    st, ln, ed = encoders[vocab].dp(text, offs, mode=form, cut_mask=cut, uncapped=True)
    assert ed is None
    _check(refs[_base(vocab), form], 1, st, ln)


def _dp_far_abi(enc, mode_flags, text, offs, cut, far_pairs):
    """dpt_dp_host_far through ctypes on host arrays whose offsets need not start at 0; text and cut
    are passed at offs[0]."""
    from dptok import _lib
    text = np.ascontiguousarray(text, np.uint8)
    offs = np.ascontiguousarray(offs, np.uint64)
    b0, n, n_bytes = int(offs[0]), len(offs) - 1, int(offs[-1] - offs[0])
    status = np.full(n, -7, np.int32)
    lengths = np.full(n, -7, np.int32)
    edges = np.zeros(max(n_bytes, 1), np.uint64)
    far = np.full(2 * max(far_pairs, 1), CANARY, np.uint64)
    nf = ctypes.c_uint64(12345)
    rc = _lib.lib().dpt_dp_host_far(enc.handle, enc.vocab.handle, mode_flags, text.ctypes.data + b0, n_bytes,
                                    offs.ctypes.data, None if cut is None else cut.ctypes.data + b0, n,
                                    status.ctypes.data, lengths.ctypes.data, edges.ctypes.data, far.ctypes.data,
                                    far_pairs, ctypes.byref(nf))
    return rc, status, lengths, edges, far, nf.value


@pytest.mark.parametrize("form,vocab,shard", [("raw", "base+40000", 0), ("presplit", "long", 1), ("atoms", "base", 2)])
def test_sharded_call_through_the_c_abi(form, vocab, shard, encoders):
    """A slice [lo, hi) of a larger upload, the offsets not rebased: the masks' indices are relative to
    str_off[0], and the result is the reference's on the rebased slice."""
    from dptok import _lib
    text, offs, cut = mc.upload(form)
    cut = None if cut is None else np.ascontiguousarray(cut)
    lo, hi = mc.shards(form)[shard]
    assert int(offs[lo]) != 0 and int(offs[lo]) % 4 == shard + 1
    voc = dp_ref.Voc(mc.vocabularies()[vocab])
    ref = _small_ref(dp_ref.run, *dp_ref.rebase_slice(text[int(offs[0]):], offs, None if cut is None else cut[int(offs[0]):],
                                                     lo, hi), dp_ref.MODE_OF[form], voc)
    assert {dp_ref.PASS_CLASSES[p] for p in np.unique(ref.end_pass[ref.is_end])} == set(dp_ref.PASS_CLASSES)
    for k, flag in ((0, _lib.DPT_FLAG_LEN_ONLY), (1, _lib.DPT_FLAG_UNCAPPED)):
        rc, st, ln, ed, far, nf = _dp_far_abi(encoders[vocab], dp_ref.MODE_OF[form] | flag, text, offs[lo:hi + 1], cut, 16)
        assert rc == 0 and nf == 0 and (far == CANARY).all()
        _check(ref, k, st, ln, ed, (form, k))


def _gather(form, idx):
    """The corpus strings idx of a form as a batch of their own."""
    text, offs, cut = mc.form(form)
    o = offs.astype(np.int64)
    t = np.concatenate([text[o[s]:o[s + 1]] for s in idx] + [np.zeros(0, np.uint8)])
    c = None if cut is None else np.concatenate([cut[o[s]:o[s + 1]] for s in idx] + [np.zeros(0, np.uint8)])
    no = np.zeros(len(idx) + 1, np.uint64)
    no[1:] = np.cumsum([o[s + 1] - o[s] for s in idx])
    if len(t) == 0:
        t = np.zeros(1, np.uint8)
        c = None if cut is None else np.zeros(1, np.uint8)
    return t, no, c


def _call_shapes(form, ref):
    """name -> string indices: one string; four; five with an empty one in the middle; a batch whose last
    string alone has a word over 2048 bytes."""
    text, offs, cut = mc.form(form)
    longest = mc.longest_words(form, text, offs, cut)
    nbytes = np.diff(offs.astype(np.int64))
    ok = ref.status[0] == 0
    several = np.flatnonzero(ok & (ref.n_words > 1) & ref.index_differs & (longest <= 256))
    small = np.flatnonzero(ok & (longest <= 2048) & (nbytes > 0))
    empty = int(np.flatnonzero(nbytes == 0)[0])
    big = int(np.flatnonzero(ok & (longest > 2048) & (ref.n_words > 1))[0])
    return {"one": [int(several[0])], "four": [int(s) for s in small[3:7]],
            "five, the middle one empty": [int(several[1]), int(small[8]), empty, int(several[2]), int(small[9])],
            "the last alone over 2048": [int(small[10]), int(several[3]), int(small[11]), big]}


@pytest.mark.parametrize("uncapped", (False, True))
@pytest.mark.parametrize("form", ("raw", "atoms"))
def test_call_shapes(form, uncapped, encoders, refs):
    voc = dp_ref.Voc(mc.vocabularies()["base"])
    for name, idx in _call_shapes(form, refs["base", form]).items():
        text, offs, cut = _gather(form, idx)
        ref = _small_ref(dp_ref.run, text, offs, cut, dp_ref.MODE_OF[form], voc)
        st, ln, ed, far = encoders["base"].dp(text, offs, mode=form, cut_mask=cut, uncapped=uncapped, edges=True, far=True)
        _check(ref, int(uncapped), st, ln, ed, name)
        assert far.shape == (0, 2)


@pytest.fixture(scope="module")
def small_encoders():
    """Engines of the cap-trap and the far-pair vocabularies, built on first use."""
    from dptok import Encoder, Vocab
    cache = {}

    def get(key, tokens):
        if key not in cache:
            cache[key] = Encoder(Vocab({t: i for i, t in enumerate(tokens)}, 0))
        return cache[key]
    return get


@pytest.mark.parametrize("uncapped", (False, True))
@pytest.mark.parametrize("lanes64", (False, True))
@pytest.mark.parametrize("form", ("raw", "atoms"))
def test_cap_trap_batch(form, lanes64, uncapped, small_encoders):
    """Where the cap binds: capped and uncapped status, lengths and masks differ in words of every pass
    (tests/test_dp_ref.py::test_cap_trap_batch_conditions counts them)."""
    tokens, text, offs, cut = dp_ref.trap_batch(form, lanes64)
    ref = _small_ref(dp_ref.trap_ref, form, lanes64)
    enc = small_encoders(("trap", lanes64), tokens)
    assert (enc.vocab.stats["max_cp"] > 16) == lanes64
    st, ln, ed, far = enc.dp(text, offs, mode=form, cut_mask=cut, uncapped=uncapped, edges=True, far=True)
    _check(ref, int(uncapped), st, ln, ed, "dpt_dp_host_far")
    assert far.shape == (0, 2)
    st, ln, ed = enc.dp(text, offs, mode=form, cut_mask=cut, uncapped=uncapped, edges=True)
    _check(ref, int(uncapped), st, ln, ed, "dpt_dp_host")
    st, ln, _ = enc.dp(text, offs, mode=form, cut_mask=cut, uncapped=uncapped)
    _check(ref, int(uncapped), st, ln, None, "no edges")


@pytest.mark.parametrize("uncapped", (False, True))
@pytest.mark.parametrize("form", ("raw", "atoms"))
def test_far_pairs_in_a_batch(form, uncapped, small_encoders):
    """More than 1024 far pairs in one call (Encoder.dp's first capacity): its retry after DPT_E_CAP
    runs, and pairs, masks and lengths equal the reference's."""
    tokens, text, offs, cut = dp_ref.far_batch(form)
    ref, k = _small_ref(dp_ref.far_ref, form), int(uncapped)
    assert len(ref.far[k]) > 1024
    enc = small_encoders("far", tokens)
    st, ln, ed, far = enc.dp(text, offs, mode=form, cut_mask=cut, uncapped=uncapped, edges=True, far=True)
    _check(ref, k, st, ln, ed, form)
    assert sorted(map(tuple, far.tolist())) == ref.far[k]      # the header promises no order
    # without a far list: status 3 for exactly the strings with a far pair, the others as before
    st, ln, ed = enc.dp(text, offs, mode=form, cut_mask=cut, uncapped=uncapped, edges=True)
    want = ref.status[k].copy()
    want[[int(ref.end_str[e]) for e, _ in ref.far[k]]] = 3
    assert (want == 0).sum() >= 5 and np.array_equal(st, want), np.flatnonzero(st != want)[:10]
    others = np.flatnonzero(want == 0)
    assert np.array_equal(ln[others], ref.lengths[k][others])
    assert dp_ref.compare_masks(ed, ref, k, others) is None


@pytest.mark.parametrize("form", ("raw", "atoms"))
def test_far_capacity_protocol(form, small_encoders):
    """dpt_dp_host_far's DPT_E_CAP answer: the count without the pairs, nothing at or beyond pair far_cap,
    and no state left behind for the next call on the context."""
    from dptok import _lib
    from oracle import oracle
    tokens, text, offs, cut = dp_ref.far_batch(form)
    ref = _small_ref(dp_ref.far_ref, form)
    need = len(ref.far[0])
    enc = small_encoders("far", tokens)
    m = dp_ref.MODE_OF[form] | _lib.DPT_FLAG_LEN_ONLY
    L = _lib.lib()
    n, n_bytes = ref.n_str, ref.n_bytes
    st, ln, ed = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n_bytes, np.uint64)
    nf = ctypes.c_uint64(7)
    p_cut = None if cut is None else cut.ctypes.data
    rc = L.dpt_dp_host_far(enc.handle, enc.vocab.handle, m, text.ctypes.data, n_bytes, offs.ctypes.data, p_cut, n,
                           st.ctypes.data, ln.ctypes.data, ed.ctypes.data, None, 0, ctypes.byref(nf))
    assert rc == _lib.DPT_E_CAP and nf.value == need
    room = need + 64        # the host array is larger than any far_cap passed
    for cap in (need - 1, need):
        far = np.full(2 * room, CANARY, np.uint64)
        nf = ctypes.c_uint64(7)
        rc = L.dpt_dp_host_far(enc.handle, enc.vocab.handle, m, text.ctypes.data, n_bytes, offs.ctypes.data, p_cut, n,
                               st.ctypes.data, ln.ctypes.data, ed.ctypes.data, far.ctypes.data, cap, ctypes.byref(nf))
        assert nf.value == need
        assert (far[2 * cap:] == CANARY).all(), cap
        if cap < need:
            assert rc == _lib.DPT_E_CAP
        else:
            assert rc == 0
            assert sorted(map(tuple, far[: 2 * need].reshape(-1, 2).tolist())) == ref.far[0]
            _check(ref, 0, st, ln, ed, "far_cap = need")
    t2i = {t: i for i, t in enumerate(tokens)}
    if form == "raw":
        got = enc.encode_csr(text, offs, mode="raw")
        want = oracle.OracleVocab(t2i).encode_csr(text, offs, mode=oracle.RAW)
    else:
        got = enc.encode_csr(text, offs, mode="atoms", cut_mask=cut)
        want = oracle.OracleVocab(t2i).encode_csr(text, offs, mode=oracle.ATOMS, cut_mask=cut)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
