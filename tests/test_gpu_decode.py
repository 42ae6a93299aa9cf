"""Device-side decode and round trip (include/dpt.h dpt_decode_sizes / dpt_decode / dpt_roundtrip and their
host forms) against the pure-Python rules of tests/decode_ref.py, for byte equality: the corpus of
tests/matrix_corpus.py in its three forms, strings on the kernel's 64-id and 64-byte round edges, the
device-path contract (a shard of a larger upload, offsets not rebased, unaligned outputs, a side stream, no
host synchronisation from the encode to the round trip, guarded outputs), ids that do not belong to their
string, and the drop-in's ``decode_dp_tokenization.batch`` / ``dp_tokenize.batch_roundtrip``."""
import numpy as np
import pytest

import decode_ref
import matrix_corpus as mc

pytestmark = pytest.mark.gpu

DEC_VOCABS = ("base", "long+40000")
HOLE = 20000   # the id no token of the holed vocabulary has


@pytest.fixture(scope="module")
def engines():
    """vocab name -> (Encoder, {rule: Detok}, {rule: decode_ref's id -> piece})."""
    from dptok import Detok, Encoder, Vocab
    out = {}
    for name in DEC_VOCABS:
        t2i = mc.vocabularies()[name]
        out[name] = (Encoder(Vocab(t2i, 0)), {r: Detok(t2i, r) for r in ("pieces", "sp")},
                     {r: decode_ref.pieces_by_id(decode_ref.pairs_of(t2i), r) for r in ("pieces", "sp")})
    assert min(mc.vocabularies()["long+40000"].values()) == mc.ID_SHIFT   # id_min != 0
    return out


def _assert_decode(got, want, what=""):
    """decode_csr's result against decode_ref.expected_decode's; the bytes of a string with an id that has
    no piece are unspecified (as is its length, so such batches are compared string by string elsewhere)."""
    raw, off, st = got
    wraw, woff, wst, ok = want
    assert ok.all()
    assert np.array_equal(st, wst), (what, np.nonzero(st != wst)[0][:10])
    assert np.array_equal(off, woff), (what, np.nonzero(off != woff)[0][:10])
    assert raw.dtype == np.uint8 and off.dtype == np.uint64 and np.array_equal(raw, wraw), (what, np.nonzero(raw != wraw)[0][:10])


def _assert_rt(got, want, what=""):
    rt, fd = got
    wrt, wfd = want
    assert np.array_equal(rt, wrt), (what, np.nonzero(rt != wrt)[0][:10], rt[rt != wrt][:10], wrt[rt != wrt][:10])
    assert np.array_equal(fd, wfd), (what, np.nonzero(fd != wfd)[0][:10], fd[fd != wfd][:10], wfd[fd != wfd][:10])


def _raw_expand(b: bytes) -> bytes:
    """pretokenize_raw's atoms of a string, joined: the word mark before byte 0, ' ' -> the mark, '\\n' -> <0x0A>."""
    if not b:
        return b""
    mark = "▁".encode("utf-8")
    return mark + b[:1] + b[1:].replace(b" ", mark).replace(b"\n", b"<0x0A>")


# ------------------------------------------------------------------ 1. the matrix corpus, host path

@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("vocab", DEC_VOCABS)
def test_matrix_corpus_decode(vocab, form, engines):
    enc, detok, by_id = engines[vocab]
    text, offs, cut = mc.form(form)
    ids, id_off, st, _ = enc.encode_csr(text, offs, mode=form, cut_mask=cut)
    counts = np.diff(id_off.astype(np.int64))
    assert len(st) > 400 and counts.max() > 4000 and (st != 0).any() and (st == 0).sum() > 200
    o = offs.astype(np.int64)
    assert form != "raw" or (np.diff(o) == 0).any()   # (empty strings: status 2)
    # pieces: the atom-expanded string -- the input bytes themselves in PRESPLIT / ATOMS
    raw, out_off, dst = detok["pieces"].decode_csr(ids, id_off, st)
    _assert_decode((raw, out_off, dst), decode_ref.expected_decode(by_id["pieces"], ids, id_off, st), (vocab, form, "pieces"))
    oo, blob, tb = out_off.astype(np.int64), raw.tobytes(), text.tobytes()
    for s in np.flatnonzero(st == 0):
        src = tb[o[s]:o[s + 1]]
        assert blob[oo[s]:oo[s + 1]] == (_raw_expand(src) if form == "raw" else src), (vocab, form, s)
    # the verdicts: RAW against SentencePiece's decode without the dummy-prefix space, the other forms against
    # their own bytes
    rule, strip = ("sp", True) if form == "raw" else ("pieces", False)
    if form == "raw":
        _assert_decode(detok["sp"].decode_csr(ids, id_off, st, strip_space=True),
                       decode_ref.expected_decode(by_id["sp"], ids, id_off, st, strip=True), (vocab, form, "sp"))
    want = decode_ref.expected_roundtrip(by_id[rule], text, offs, ids, id_off, st, strip=strip)
    _assert_rt(detok[rule].roundtrip_csr(text, offs, ids, id_off, st, strip_space=strip), want, (vocab, form))
    if form != "raw":
        assert not want[0][st == 0].any()
    else:
        assert (want[0][st == 0] == 0).sum() > 200


# ------------------------------------------------------------------ 2. round edges

SKIP = 1   # "<s>" of the llama-shaped vocabulary
LONG_A, LONG_B = "Q" * 300, "Z" * 5000


@pytest.fixture(scope="module")
def edge_batch():
    return build_edge_batch()


def build_edge_batch():
    """Strings on the walk's edges as one CSR batch (ids, id_off, the texts to compare with), the Detok and
    decode_ref's expectations, computed once; "lists" / "texts" / "by_id": the batch string by string and
    decode_ref's table (test_gpu_wave_stride.py reorders them)."""
    from dptok import Detok, Encoder, Vocab, pack_strings, synth
    t2i = dict(synth.llama_shaped_vocab())
    assert t2i["<s>"] == SKIP and LONG_A not in t2i and max(t2i.values()) == 31999
    t, _ = synth.random_ascii_corpus(1, 400, seed=11)
    base = bytes(t).decode("ascii")
    strs = [base[:L] for L in range(1, 401)] + ["a" + "\n" * 300]
    enc = Encoder(Vocab(t2i, 0))
    text, offs = pack_strings(strs)
    ids, id_off, st, _ = enc.encode_csr(text, offs)
    counts = np.diff(id_off.astype(np.int64))
    assert not st.any() and {63, 64, 65, 127, 128, 129} <= set(counts[:400].tolist())
    assert counts[400] == 301 and set(ids[int(id_off[400]) + 1:].tolist()) == {t2i["<0x0A>"]}   # the 6-to-1 piece
    lists = [ids[int(id_off[s]):int(id_off[s + 1])].tolist() for s in range(len(strs))]
    texts = [s.encode() for s in strs]
    # hand-made id lists over the vocabulary plus a 300-byte and a 5000-byte token
    dt2i = dict(t2i)
    dt2i[LONG_A], dt2i[LONG_B] = 32000, 32001
    a, b, sp_the = t2i["a"], t2i["b"], t2i["▁a"]
    by_id = decode_ref.pieces_by_id(decode_ref.pairs_of(dt2i), "sp", [SKIP])
    assert by_id[a] == b"a" and by_id[sp_the] == b" a"
    made = [[SKIP], [SKIP] * 64, [SKIP] * 70, [SKIP] + [a] * 62 + [SKIP, SKIP] + [b] * 65,       # skips at 0, 63, 64
            [], [a], [a] * 63, [a] * 64, [a] * 65,                                                # 0, 1, 63, 64, 65 bytes
            [sp_the], [SKIP, sp_the], [SKIP, sp_the, a], [SKIP] * 64 + [sp_the, b], [a, sp_the],  # the ' ' of a later id
            [a, 32000, b, 32001, a, 32000], [32001], [b] * 60 + [32001] + [a] * 10 + [32000] * 3]
    for ml in made:
        dec, ok = decode_ref.decode_ids(by_id, ml, strip=True)
        assert ok
        lists.append(ml)
        texts.append(dec)
    assert [len(x) for x in texts[405:410]] == [0, 1, 63, 64, 65] and texts[411] == b"a" and texts[413] == b"ab" and texts[414] == b"a a"
    # the same decodes against texts that differ at, before and after a round's edge
    for ml, edit in ((made[8], lambda x: x[:63] + b"X" + x[64:]), (made[8], lambda x: x[:64] + b"X"), (made[8], lambda x: x[:64]),
                     (made[8], lambda x: x + b"a"), (made[7], lambda x: x[:-1]), (made[14], lambda x: x[:4000] + b"q" + x[4001:]),
                     (made[14], lambda x: x[:302]), (made[11], lambda x: b" " + x), (made[0], lambda x: b"a"), (made[3], lambda x: x[:62] + b"a" + x[63:])):
        lists.append(ml)
        texts.append(edit(decode_ref.decode_ids(by_id, ml, strip=True)[0]))
    flat = np.array([i for ml in lists for i in ml], dtype=np.int32)
    io = np.zeros(len(lists) + 1, dtype=np.uint64)
    io[1:] = np.cumsum([len(ml) for ml in lists], dtype=np.uint64)
    tx = np.frombuffer(b"".join(texts) + b"\0", dtype=np.uint8)
    to = np.zeros(len(texts) + 1, dtype=np.uint64)
    to[1:] = np.cumsum([len(x) for x in texts], dtype=np.uint64)
    want_dec = decode_ref.expected_decode(by_id, flat, io, strip=True)
    want_rt = decode_ref.expected_roundtrip(by_id, tx, to, flat, io, strip=True)
    for arr in want_dec + want_rt:
        arr.setflags(write=False)
    n_made = len(made)
    assert not want_rt[0][:401 + n_made].any()
    assert want_rt[0][401 + n_made:].tolist() == [5] * 10 and want_rt[1][401 + n_made:].tolist() == [63, 64, 64, 65, 63, 4000, 302, 0, 0, 62]
    return {"detok": Detok(dt2i, "sp", [SKIP]), "ids": flat, "id_off": io, "text": tx, "offs": to, "dec": want_dec, "rt": want_rt,
            "lists": lists, "texts": texts, "by_id": by_id}


def test_round_edges_whole_batch(edge_batch):
    e = edge_batch
    _assert_decode(e["detok"].decode_csr(e["ids"], e["id_off"], strip_space=True), e["dec"])
    _assert_rt(e["detok"].roundtrip_csr(e["text"], e["offs"], e["ids"], e["id_off"], strip_space=True), e["rt"])
    # without the strip every decode that began with ' ' keeps it
    raw, off, st = e["detok"].decode_csr(e["ids"], e["id_off"])
    lens, wlens = np.diff(off.astype(np.int64)), np.diff(e["dec"][1].astype(np.int64))
    assert not st.any() and set((lens - wlens).tolist()) == {0, 1} and (lens - wlens)[:401].all()


@pytest.mark.parametrize("n_str", [1, 5])
def test_round_edges_small_calls(n_str, edge_batch):
    """The batch again, n_str strings per call: grids of one block with one to four busy waves and of two
    blocks, id and text offsets that do not start at 0."""
    e = edge_batch
    wraw, woff, wst, _ = e["dec"]
    wrt, wfd = e["rt"]
    wo = woff.astype(np.int64)
    n = len(wst)
    for a in range(0, n, n_str):
        b = min(a + n_str, n)
        raw, off, st = e["detok"].decode_csr(e["ids"], e["id_off"][a:b + 1], strip_space=True)
        assert np.array_equal(off.astype(np.int64), wo[a:b + 1] - wo[a]) and not st.any(), a
        assert np.array_equal(raw, wraw[wo[a]:wo[b]]), a
        _assert_rt(e["detok"].roundtrip_csr(e["text"], e["offs"][a:b + 1], e["ids"], e["id_off"][a:b + 1], strip_space=True),
                   (wrt[a:b], wfd[a:b]), a)


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


S_OUT, S_ST, S_FD, S_LEN = 0xA5, -0x2D2D2D2E, -0x3C3C3C3D, -0x5A5A5A5A5A5A5A5B
OUT_START = 1000003   # out_off[0] of every shard's decode


@pytest.mark.parametrize("form", mc.FORMS)
@pytest.mark.parametrize("vocab", DEC_VOCABS)
def test_device_path_contract(vocab, form, engines, uploads, side_stream):
    torch = pytest.importorskip("torch")
    enc, detok, by_id = engines[vocab]
    rule, strip = ("sp", True) if form == "raw" else ("pieces", False)
    dk, pieces = detok[rule], by_id[rule]
    h, d, (text, offs, cut) = uploads[form]
    shards = mc.shards(form)
    for shard, (lo, hi) in enumerate(shards):
        b0, b1 = int(offs[lo]), int(offs[hi])
        n, n_bytes = hi - lo, b1 - b0
        assert b0 != 0 and b1 < len(text)
        # the larger upload the decode calls read: the encode's outputs behind `pad` foreign entries, so that
        # id_off[0] != 0 and the ids do not start their buffer
        pad = 7 + shard
        ids = torch.full((n_bytes + pad,), -1, dtype=torch.int32, device="cuda")
        id_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        st = torch.empty(n, dtype=torch.int32, device="cuda")
        out_cap = 6 * n_bytes + 64   # (RAW: a '\n' is six bytes under "pieces"; "sp" is never longer than that)
        byte_off = 1 + shard         # out at byte offsets 1, 2 and 3 of its buffer
        lens, out_off = mc.Guarded(torch, n, torch.int64, S_LEN), torch.empty(n + 1, dtype=torch.int64, device="cuda")
        out, dst = mc.Guarded(torch, out_cap + 4, torch.uint8, S_OUT), mc.Guarded(torch, n, torch.int32, S_ST)
        out2, dst2 = mc.Guarded(torch, out_cap + 4, torch.uint8, S_OUT), mc.Guarded(torch, n, torch.int32, S_ST)
        rt, fd = mc.Guarded(torch, n, torch.int32, S_ST), mc.Guarded(torch, n, torch.int32, S_FD)
        rt2 = mc.Guarded(torch, n, torch.int32, S_ST)
        enc.reserve(n_bytes, n)   # (the encode then allocates nothing: no implicit device synchronisation)
        d["text"].fill_(0x20)     # what the buffers held before must not survive
        if d["cut"] is not None:
            d["cut"].zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(side_stream):
            for k in ("text", "offs", "cut"):
                if d[k] is not None:
                    d[k].copy_(h[k], non_blocking=True)
            for g in (lens, out, dst, out2, dst2, rt, fd, rt2):
                g.fill()
            tp, op = d["text"].data_ptr() + b0, d["offs"].data_ptr() + 8 * lo
            cp = 0 if d["cut"] is None else d["cut"].data_ptr() + b0
            sid = side_stream.cuda_stream
            ip = ids.data_ptr() + 4 * pad
            enc.encode_device(tp, n_bytes, op, n, ip, n_bytes, id_off.data_ptr(), st.data_ptr(), cut_ptr=cp, stream=sid, mode=form)
            id_off += 12345   # the decode calls rebase by id_off[0]
            dk.sizes_device(ip, id_off.data_ptr(), n, lens.ptr(), status_ptr=st.data_ptr(), strip_space=strip, stream=sid)
            out_off[0] = OUT_START
            torch.cumsum(lens.view, 0, out=out_off[1:])
            out_off[1:] += OUT_START
            dk.decode_device(ip, id_off.data_ptr(), n, out.ptr() + byte_off, out_off.data_ptr(), dst.ptr(), status_ptr=st.data_ptr(),
                             strip_space=strip, stream=sid)
            dk.roundtrip_device(ip, id_off.data_ptr(), tp, op, n, rt.ptr(), first_diff_ptr=fd.ptr(), status_ptr=st.data_ptr(),
                                strip_space=strip, stream=sid)
            # status == NULL: every string counts as encoded (a failed one has no ids and decodes to nothing)
            dk.decode_device(ip, id_off.data_ptr(), n, out2.ptr() + byte_off, out_off.data_ptr(), dst2.ptr(), strip_space=strip,
                             stream=sid)
            dk.roundtrip_device(ip, id_off.data_ptr(), tp, op, n, rt2.ptr(), strip_space=strip, stream=sid)
        side_stream.synchronize()   # that stream only
        h_ids, h_off, h_st = ids.cpu().numpy()[pad:], id_off.cpu().numpy().view(np.uint64), st.cpu().numpy()
        assert int(h_off[0]) == 12345
        n_tok = int(h_off[-1] - h_off[0])
        res = {}
        for k, g in (("lens", lens), ("out", out), ("dst", dst), ("out2", out2), ("dst2", dst2), ("rt", rt), ("fd", fd), ("rt2", rt2)):
            res[k], ok = g.host()
            assert ok, "guard zone of %s overwritten" % k
        wraw, woff, wst, ok = decode_ref.expected_decode(pieces, h_ids[:n_tok], h_off, h_st, strip=strip)
        assert ok.all() and len(wraw) <= out_cap
        assert np.array_equal(res["lens"].view(np.uint64), np.diff(woff)), (lo, hi)
        assert np.array_equal(out_off.cpu().numpy().view(np.uint64), woff + np.uint64(OUT_START))
        for k, ks, want_st in (("out", "dst", wst), ("out2", "dst2", np.zeros(n, np.int32))):
            assert np.array_equal(res[ks], want_st), (lo, hi, ks)
            assert (res[k][:byte_off] == S_OUT).all() and (res[k][byte_off + len(wraw):] == S_OUT).all(), "%s written outside its range" % k
            assert np.array_equal(res[k][byte_off:byte_off + len(wraw)], wraw), (lo, hi, k)
        wrt, wfd = decode_ref.expected_roundtrip(pieces, text, offs[lo:hi + 1], h_ids[:n_tok], h_off, h_st, strip=strip)
        assert np.array_equal(res["rt"], wrt), (lo, hi)
        assert np.array_equal(np.where(wrt == 5, res["fd"].view(np.uint32).astype(np.int64), -1), wfd), (lo, hi)
        assert (res["fd"][wrt != 5] == S_FD).all(), "first_diff written where the verdict is not 5"
        wrt2, _ = decode_ref.expected_roundtrip(pieces, text, offs[lo:hi + 1], h_ids[:n_tok], h_off, None, strip=strip)
        assert np.array_equal(res["rt2"], wrt2), (lo, hi)


# ------------------------------------------------------------------ 4. ids that do not belong to their string

def test_foreign_ids_in_range():
    """One id of a string replaced by a token of another byte length, or by an id inside [id_min, id_max]
    that no token has: decode gives that string status 4 and the round trip 4 or 5 as decode_ref says, every
    other string its exact result, and nothing is stored outside the output ranges.  (Ids outside the table:
    test_gpu_wave_stride.py::test_decode_capped.)"""
    torch = pytest.importorskip("torch")
    from dptok import Detok, Encoder, Vocab
    t2i = {t: i + (1 if i >= HOLE else 0) for t, i in mc.vocabularies()["base"].items()}
    assert HOLE not in set(t2i.values()) and min(t2i.values()) < HOLE < max(t2i.values())
    enc, dk = Encoder(Vocab(t2i, 0)), Detok(t2i, "sp")
    by_id = decode_ref.pieces_by_id(decode_ref.pairs_of(t2i), "sp")
    text, offs, _ = mc.form("raw")
    ids, id_off, st, _ = enc.encode_csr(text, offs)
    wraw, woff, wst, ok = decode_ref.expected_decode(by_id, ids, id_off, st, strip=True)
    assert ok.all()
    o = id_off.astype(np.int64)
    counts = np.diff(o)
    by_len = {}
    for t, i in t2i.items():
        by_len.setdefault(len(by_id[i]), i)
    okc = np.where(st == 0, counts, 0)
    last = int(np.flatnonzero(okc > 0)[-1])
    big = np.flatnonzero(okc >= 130)
    small = np.flatnonzero((okc >= 2) & (okc <= 10))
    # (string, token index, "len": a token whose piece is one byte longer or shorter / "hole")
    edits = [(int(big[0]), 100, "len"), (int(big[1]), 64, "hole"), (int(big[2]), int(okc[big[2]]) - 1, "len"),
             (int(small[0]), 0, "len"), (int(small[1]), 1, "hole"), (last, int(okc[last]) - 1, "hole"),
             (int(small[2]), 0, "hole"), (int(big[3]), 63, "len"), (int(big[4]), 0, "hole")]
    assert len({s for s, _, _ in edits}) == len(edits)
    bad_ids = ids.copy()
    for s, k, kind in edits:
        n = len(by_id[int(ids[o[s] + k])])
        bad_ids[o[s] + k] = HOLE if kind == "hole" else by_len[n + 1 if n + 1 in by_len else n - 1]
    n = len(st)
    dev = {k: torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in
           (("text", text), ("offs", offs.view(np.int64)), ("ids", bad_ids), ("id_off", id_off.view(np.int64)), ("st", st),
            ("out_off", woff.view(np.int64)))}   # the output ranges of the ids as they were
    out, dst = mc.Guarded(torch, len(wraw), torch.uint8, S_OUT), mc.Guarded(torch, n, torch.int32, S_ST)
    rt, fd = mc.Guarded(torch, n, torch.int32, S_ST), mc.Guarded(torch, n, torch.int32, S_FD)
    for g in (out, dst, rt, fd):
        g.fill()
    dk.decode_device(dev["ids"].data_ptr(), dev["id_off"].data_ptr(), n, out.ptr(), dev["out_off"].data_ptr(), dst.ptr(),
                     status_ptr=dev["st"].data_ptr(), strip_space=True)
    dk.roundtrip_device(dev["ids"].data_ptr(), dev["id_off"].data_ptr(), dev["text"].data_ptr(), dev["offs"].data_ptr(), n, rt.ptr(),
                        first_diff_ptr=fd.ptr(), status_ptr=dev["st"].data_ptr(), strip_space=True)
    torch.cuda.synchronize()
    res = {}
    for k, g in (("out", out), ("dst", dst), ("rt", rt), ("fd", fd)):
        res[k], ok = g.host()
        assert ok, "guard zone of %s overwritten" % k
    victims = sorted({s for s, _, _ in edits})
    want_st = wst.copy()
    want_st[victims] = 4
    assert np.array_equal(res["dst"], want_st), np.nonzero(res["dst"] != want_st)[0][:10]
    keep = np.ones(len(wraw), dtype=bool)
    wo = woff.astype(np.int64)
    for s in victims:
        keep[wo[s]:wo[s + 1]] = False   # (a status-4 string's bytes are unspecified)
    assert np.array_equal(res["out"][keep], wraw[keep])
    wrt, wfd = decode_ref.expected_roundtrip(by_id, text, offs, bad_ids, id_off, st, strip=True)
    assert set(wrt[victims].tolist()) == {4, 5}
    others = np.setdiff1d(np.arange(n), victims)
    assert np.array_equal(wrt[others], decode_ref.expected_roundtrip(by_id, text, offs, ids, id_off, st, strip=True)[0][others])
    assert np.array_equal(res["rt"], wrt), np.nonzero(res["rt"] != wrt)[0][:10]
    assert np.array_equal(np.where(wrt == 5, res["fd"].view(np.uint32).astype(np.int64), -1), wfd)


# ------------------------------------------------------------------ 5. the round trip finds what it should

def test_roundtrip_finds_differences():
    from dptok import RT_DIFFERS, RT_EQUAL, Detok, Encoder, Vocab, pack_strings, synth
    t2i = synth.llama_shaped_vocab()
    strs = ["a<0x41>b", "x▁y", "plain text", " lead", "tab\there"]
    text, offs = pack_strings(strs)
    ids, id_off, st, _ = Encoder(Vocab(t2i, 0)).encode_csr(text, offs)
    by_id = decode_ref.pieces_by_id(decode_ref.pairs_of(t2i), "sp")
    want = decode_ref.expected_roundtrip(by_id, text, offs, ids, id_off, st, strip=True)
    got = Detok(t2i, "sp").roundtrip_csr(text, offs, ids, id_off, st, strip_space=True)
    _assert_rt(got, want)
    assert got[0][:3].tolist() == [RT_DIFFERS, RT_DIFFERS, RT_EQUAL] and got[1][:3].tolist() == [1, 1, -1]
    assert got[0][3] == st[3] != 0   # the leading space does not encode in raw mode: its status, no verdict


# ------------------------------------------------------------------ 6. the drop-in surface

def test_dropin_llama_sentencepiece():
    from conftest import load_golden
    from packages.tokenizer_utils import dp_tokenize_llama
    from sp_llama import SPLlama
    cases = [c for c in load_golden("sp_llama_cases.json.gz")["cases"] if c["tokenizer"] == "sp"]
    assert len(cases) == 565
    dp_tokenize, decode_dp_tokenization = dp_tokenize_llama(SPLlama())
    got = decode_dp_tokenization.batch([c["ids"] for c in cases])        # one call
    assert got == [c["decoded"] for c in cases]
    assert decode_dp_tokenization(cases[23]["ids"]) == cases[23]["decoded"]   # the per-string closure is the tokenizer's own
    texts = [c["text"] for c in cases]
    rt = dp_tokenize.batch_roundtrip(texts)
    assert dp_tokenize.batch(texts) == [c["ids"] for c in cases]
    equal = [c["decoded"] == c["text"] for c in cases]
    assert [r is None for r in rt] == equal and 0 < sum(equal) < 565
    for c, r in zip(cases, rt):
        if r is not None:
            a, b = c["text"].encode("utf-8"), c["decoded"].encode("utf-8")
            if "\ufffd" not in c["decoded"]:   # (bytes that are not UTF-8 read back as U+FFFD: the offset is in the bytes)
                assert r == next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b))), c["text"]


def test_dropin_raw_and_errors():
    from fake_llama import FakeLlamaTokenizer
    from packages.tokenizer_utils import dp_tokenize_llama
    t2i = mc.vocabularies()["base"]
    dp_tokenize, decode_dp_tokenization = dp_tokenize_llama(FakeLlamaTokenizer(t2i), "raw")
    texts = ["the weather", "a<0x41>b", "x\n\ny", "a é 中文", "x▁y", "a"]
    by_id = decode_ref.pieces_by_id(decode_ref.pairs_of(t2i), "sp", [t2i["<s>"]])
    lists = dp_tokenize.batch(texts)
    want = [decode_ref.roundtrip_one(by_id, ids, t.encode("utf-8"), strip=True)[1] for ids, t in zip(lists, texts)]
    assert dp_tokenize.batch_roundtrip(texts) == want == [None, 1, None, None, 1, None]
    assert decode_dp_tokenization.batch(lists) == ["the weather", "aAb", "x\n\ny", "a é 中文", "x y", "a"]
    assert decode_dp_tokenization.batch([]) == []
    for bad, exc in ((" x", ValueError), ("", IndexError)):   # what ``batch`` raises
        with pytest.raises(exc):
            dp_tokenize.batch(["a", bad])
        with pytest.raises(exc):
            dp_tokenize.batch_roundtrip(["a", bad])


def test_dropin_bloom():
    import tempfile
    from bloom_fixture import bloom_texts, bloom_tokenizer, make_hf_cache
    from packages.tokenizer_utils import dp_tokenize_bloom
    with tempfile.TemporaryDirectory() as d:
        hf = make_hf_cache(d)
        dp_tokenize, decode_dp_tokenization = dp_tokenize_bloom(bloom_tokenizer(hf), hf)
        texts = bloom_texts(48)
        assert dp_tokenize.batch_roundtrip(texts) == [None] * 48
        assert decode_dp_tokenization.batch(dp_tokenize.batch(texts)) == texts
