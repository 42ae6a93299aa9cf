"""Every cell of launch_encode's dispatch -- lane variant x mode x staging width x plain / by-product
call x entry point -- and the device-path contract of include/dpt.h, bit-exact against the C oracle
on the corpus of tests/matrix_corpus.py (DESIGN.md lists which cell reaches which instantiation).

The device entries run the way a sharded caller does: a slice [lo, hi) of a larger upload with the
offsets NOT rebased (str_off[0] != 0), text / cut-mask pointers that are not 4-byte aligned, on a side
stream with the inputs produced on that stream and no host synchronisation before the call,
capped_len given, ids_cap == n_bytes, and every output carved out of a larger tensor whose guard
zones must come back untouched."""
import numpy as np
import pytest

import matrix_corpus as mc
from test_gpu_parity import _cmp_csr

pytestmark = pytest.mark.gpu

N_BINS = 258
# (dp in ATOMS mode too: the 16-lane runtime-mode ATOMS kernel with int32 staging has no other caller)
CELLS = [(v, f, e) for v in mc.VOCAB_NAMES for f in mc.FORMS for e in ("host", "device", "padded", "dp")]


@pytest.fixture(scope="module")
def encoders():
    from dptok import Encoder, Vocab
    out = {}
    for name, t2i in mc.vocabularies().items():
        v = Vocab(t2i, 0)
        assert (v.stats["max_cp"] > 16) == name.startswith("long"), (name, v.stats)
        out[name] = Encoder(v)
    return out


@pytest.fixture(scope="module")
def expected():
    """(vocabulary, form, shard or None) -> the oracle's (ids, id_off, status, capped), computed once.
    A shard's result is the oracle run on that shard's rebased slice."""
    from oracle import oracle
    orc = {k: oracle.OracleVocab(v) for k, v in mc.vocabularies().items()}
    cache = {}

    def get(vocab, form, shard=None):
        key = (vocab, form, shard)
        if key not in cache:
            text, offs, cut = mc.form(form)
            if shard is not None:
                lo, hi = shard
                b0, b1 = int(offs[lo]), int(offs[hi])
                text, offs = text[b0:b1], offs[lo:hi + 1] - offs[lo]
                cut = None if cut is None else cut[b0:b1]
            res = orc[vocab].encode_csr(text, offs, mode=mc.oracle_mode(form), cut_mask=cut)
            for a in res:
                a.setflags(write=False)
            cache[key] = res
        return cache[key]
    return get


@pytest.fixture(scope="module")
def uploads():
    """form -> the upload in pinned host memory and its device buffers (offsets valid on the device,
    text and cut mask filled in by each call's own stream)."""
    torch = pytest.importorskip("torch")
    out = {}
    for f in mc.FORMS:
        text, offs, cut = mc.upload(f)
        h = {"text": torch.from_numpy(text.copy()).pin_memory(),
             "offs": torch.from_numpy(offs.view(np.int64).copy()).pin_memory(),
             "cut": None if cut is None else torch.from_numpy(cut.copy()).pin_memory()}
        d = {k: (None if t is None else torch.empty_like(t, device="cuda")) for k, t in h.items()}
        d["offs"].copy_(h["offs"])
        out[f] = (h, d, offs)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def side_stream():
    torch = pytest.importorskip("torch")
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0 and s.cuda_stream != torch.cuda.default_stream().cuda_stream
    return s


def _device_shard(torch, enc, form, upload, shard, padded, stream, with_hist):
    """One dpt_encode / dpt_encode_padded call on strings [lo, hi) of the upload under the device-path
    conditions; returns the outputs on the host."""
    h, d, offs = upload
    lo, hi = shard
    b0, b1 = int(offs[lo]), int(offs[hi])
    n, n_bytes = hi - lo, b1 - b0
    assert b0 != 0 and b1 < len(h["text"])
    ids = mc.Guarded(torch, n_bytes, torch.int32, -0x5A5A5A5B)
    aux = mc.Guarded(torch, n if padded else n + 1, torch.int64, -0x5A5A5A5A5A5A5A5B)   # counts / id_off
    st = mc.Guarded(torch, n, torch.int32, -0x3C3C3C3D)
    cap = mc.Guarded(torch, n, torch.int32, -0x2D2D2D2E)
    folded = torch.empty(N_BINS + 8, dtype=torch.int64, device="cuda")
    sep = torch.empty(N_BINS + 8, dtype=torch.int64, device="cuda")
    enc.reserve(n_bytes, n)   # (the call itself then allocates nothing: no implicit device synchronisation)
    # what the buffers held before must not survive: a call that ran ahead of its producer reads this
    d["text"].fill_(0x20)
    if d["cut"] is not None:
        d["cut"].zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for k in ("text", "offs", "cut"):
            if d[k] is not None:
                d[k].copy_(h[k], non_blocking=True)
        for g in (ids, aux, st, cap):
            g.fill()
        folded.zero_()
        sep.zero_()
        kw = dict(capped_ptr=cap.ptr(), cut_ptr=0 if d["cut"] is None else d["cut"].data_ptr() + b0,
                  stream=stream.cuda_stream, mode=form)
        args = (d["text"].data_ptr() + b0, n_bytes, d["offs"].data_ptr() + 8 * lo, n, ids.ptr(), n_bytes, aux.ptr(),
                st.ptr())
        if padded:
            enc.encode_device_padded(*args, **kw)
        else:
            if with_hist:
                enc.set_histogram(folded.data_ptr(), N_BINS)
            enc.encode_device(*args, **kw)
            if with_hist:
                enc.histogram_device(aux.ptr(), st.ptr(), n, sep.data_ptr(), N_BINS, stream=stream.cuda_stream)
    stream.synchronize()   # that stream only
    res = {}
    for k, g in (("ids", ids), ("aux", aux), ("status", st), ("capped", cap)):
        res[k], ok = g.host()
        assert ok, "guard zone of %s overwritten" % k
    res["folded"], res["sep"] = folded.cpu().numpy(), sep.cpu().numpy()
    return res


@pytest.mark.parametrize("vocab,form,entry", CELLS)
def test_dispatch_cell(vocab, form, entry, encoders, expected, request):
    enc = encoders[vocab]
    text, offs, cut = mc.form(form)
    if entry == "host":
        got = enc.encode_csr(text, offs, mode=form, cut_mask=cut)
        ref = expected(vocab, form)
        _cmp_csr(got, ref)
        assert np.array_equal(got[3], ref[3])
        return
    if entry == "dp":   # LEN_ONLY: the runtime-mode kernels
        st, lens, _ = enc.dp(text, offs, mode=form, cut_mask=cut)
        ref = expected(vocab, form)
        assert np.array_equal(st, ref[2]), np.nonzero(st != ref[2])[0][:10]
        assert np.array_equal(lens, ref[3]), np.nonzero(lens != ref[3])[0][:10]
        return
    torch = pytest.importorskip("torch")
    uploads, stream = request.getfixturevalue("uploads"), request.getfixturevalue("side_stream")
    up = uploads[form]
    shards = mc.shards(form)
    assert len(shards) >= 3 and {int(up[2][lo]) % 4 for lo, _ in shards} >= {1, 2, 3}
    longest = mc.longest_words(form, text, offs, cut)
    for k, sh in enumerate(shards):
        lo, hi = sh
        assert {mc.pass_of(int(x)) for x in longest[lo:hi]} >= {None, "mid", "big", "long"}, sh
        rids, roff, rst, rcap = expected(vocab, form, sh)
        got = _device_shard(torch, enc, form, up, sh, entry == "padded", stream, with_hist=(k == 0))
        assert np.array_equal(got["status"], rst), (sh, np.nonzero(got["status"] != rst)[0][:10])
        assert np.array_equal(got["capped"], rcap), (sh, np.nonzero(got["capped"] != rcap)[0][:10])
        if entry == "device":
            off = got["aux"].view(np.uint64)
            assert np.array_equal(off, roff), (sh, np.nonzero(off != roff)[0][:10])
            assert np.array_equal(got["ids"][: int(roff[-1])], rids), sh
            need, arena = enc.long_need()
            assert need > 0 and need <= arena, (need, arena)   # the shard has a word over 2048 bytes
            if k == 0:
                assert np.array_equal(got["folded"], got["sep"]), (got["folded"][-8:], got["sep"][-8:])
                assert got["sep"][N_BINS + 1] == hi - lo and got["sep"][N_BINS] == int(roff[-1])
        else:
            counts = got["aux"]
            rcount = np.diff(roff.astype(np.int64))
            assert np.array_equal(counts, rcount), (sh, np.nonzero(counts != rcount)[0][:10])
            so = (offs[lo:hi] - offs[lo]).astype(np.int64)
            for s in range(hi - lo):
                c = int(rcount[s])
                assert np.array_equal(got["ids"][so[s]:so[s] + c], rids[int(roff[s]):int(roff[s]) + c]), (sh, s)
