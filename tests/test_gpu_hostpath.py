"""Small host-path calls (round 4): dpt_encode_host skips the 2048-byte and unbounded passes' launches
when its own scan of the text shows no string can need them (dpt_host.cpp no_fallback_needed), and
brings the counter block back inside its one device-to-host copy.  The scan must agree with the
kernels' routing exactly, so the cases sit on both sides of every limit -- words of 256 / 257 bytes
(raw and pre-split), word starts exactly 256 bytes apart, atoms of 4 / 5 bytes (malformed UTF-8),
leading continuation bytes -- each as its own small call, checked against the C oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _cases():
    rng = np.random.default_rng(21)

    def rnd(n):
        return bytes(int(c) for c in rng.integers(0x21, 0x7F, size=n))
    cases = []
    for L in (255, 256, 257, 300):
        cases.append(rnd(L))                                   # one word of L bytes
        cases.append(rnd(100) + b" " + rnd(L - 1))             # a second word of L bytes (space included)
        cases.append(rnd(L) + b" " + rnd(10))
    cases.append(rnd(256) + b" yy")                            # a word start exactly 256 bytes in
    cases.append(rnd(200) + b" " + rnd(255) + b" " + rnd(255))
    cont = bytes([0x80])
    for k in (2, 3, 4, 5):                                     # atoms of a lead byte + k-1 continuations
        cases.append(b"ab " + bytes([0xF0]) + cont * (k - 1) + b" cd")
    cases.append(cont * 4 + b"x y")                            # leading continuation bytes (the first atom)
    cases.append(cont * 5 + b"x y")
    cases.append("é中😀 x".encode() * 10)
    return cases


def test_small_calls_at_the_fallback_limits(vocabs):
    from dptok import Encoder, Vocab, pack_strings
    from oracle import oracle
    t2i = vocabs["llama32k"]
    enc, orc = Encoder(Vocab(t2i, 0)), oracle.OracleVocab(t2i)
    for b in _cases():
        offs = np.array([0, len(b)], dtype=np.uint64)
        text = np.frombuffer(b + b"\0", dtype=np.uint8)
        got = enc.encode_csr(text, offs)
        ref = orc.encode_csr(text, offs)
        for g, r, what in zip(got, ref, ("ids", "offsets", "status", "capped")):
            assert np.array_equal(g, r), (what, b[:40], len(b))
    # and all of them in one call (bytes: malformed UTF-8 does not round-trip through str)
    blob = b"".join(_cases())
    lens = [len(b) for b in _cases()]
    offs = np.zeros(len(lens) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    text = np.frombuffer(blob + b"\0", dtype=np.uint8)
    got, ref = enc.encode_csr(text, offs), orc.encode_csr(text, offs)
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)


def test_presplit_small_calls(vocabs):
    """Pre-split words (llama mode's layout) of 256 / 257 bytes and more, one small call each."""
    from dptok import Encoder, Vocab
    from dptok.engine import pack_presplit_words
    from oracle import oracle
    t2i = vocabs["llama32k"]
    enc, orc = Encoder(Vocab(t2i, 0)), oracle.OracleVocab(t2i)
    rng = np.random.default_rng(5)
    for L in (200, 256, 257, 400, 3000):
        words = ["\u2581" + "".join(chr(int(c)) for c in rng.integers(0x61, 0x7B, size=L - 3)), "\u2581ab", "c"]
        text, offs, cut, _, _ = pack_presplit_words([words])
        got = enc.encode_csr(text, offs, mode="presplit", cut_mask=cut)
        ref = orc.encode_csr(text, offs, mode=oracle.PRESPLIT, cut_mask=cut)
        for g, r, what in zip(got, ref, ("ids", "offsets", "status", "capped")):
            assert np.array_equal(g, r), (what, L)


def test_one_string_calls(vocabs):
    """One-string host-path calls run the first pass alone (EncodeLaunch::solo: ids straight into the
    output, id_off and the counter reset by the lone wave): every mode, empty and untokenizable
    strings, the 64-lane kernel's vocabulary, interleaved with multi-string calls on the same context
    (a counter the lone wave failed to reset would show in the next call)."""
    from dptok import Encoder, Vocab, pack_strings
    from oracle import oracle
    rng = np.random.default_rng(8)
    t2i_long = dict(vocabs["llama32k"])
    for L in (17, 24, 40):
        for _ in range(10):
            tok = "".join(chr(c) for c in rng.integers(0x61, 0x65, size=L))
            t2i_long.setdefault(tok, len(t2i_long))
    pool = [chr(c) for c in range(0x21, 0x7F)] + ["é", "中", "😀", "\n", " ", "  "]
    texts = ["", " ", "a", "\n", "中文 😀", "abcd" * 40] + \
            ["".join(rng.choice(pool, size=int(rng.integers(1, 250)))) for _ in range(40)] + \
            ["".join(chr(c) for c in rng.integers(0x61, 0x65, size=200))]
    for name, t2i in (("llama32k", vocabs["llama32k"]), ("toy1k", vocabs["toy1k"]), ("long", t2i_long)):
        enc, orc = Encoder(Vocab(t2i, 0)), oracle.OracleVocab(t2i)
        for k, s in enumerate(texts):
            text, offs = pack_strings([s])
            got, ref = enc.encode_csr(text, offs), orc.encode_csr(text, offs)
            for g, r, what in zip(got, ref, ("ids", "offsets", "status", "capped")):
                assert np.array_equal(g, r), (name, k, what, s[:30])
            if k % 7 == 3:   # a multi-string call between one-string calls
                text, offs = pack_strings(texts[:k + 2])
                got, ref = enc.encode_csr(text, offs), orc.encode_csr(text, offs)
                for g, r in zip(got, ref):
                    assert np.array_equal(g, r), (name, k, "batch")


def test_zero_copy_calls_after_the_spans_path_moved_the_pinned_buffers(vocabs):
    """The host paths share one pair of pinned staging buffers (dpt_host.cpp Stager::stage), and the
    one-string zero-copy call addresses them from the device: a spans host call that outgrows them moves
    them, and the next one-string encode must look their device addresses up again.  One Encoder: a
    one-string call (4096-byte pinned buffers, addresses looked up), a dpt_token_spans_host call on 64
    strings of 200 bytes whose ids come from the oracle (so no encode call has grown the buffers: both
    move here), one-string calls, then the same through encode_csr_spans, one-string calls again (empty,
    ASCII, multi-byte) and a PRESPLIT one -- each exact against the oracle, the spans against the walk of
    tests/spans_ref.py."""
    import spans_ref
    from dptok import Encoder, Vocab, _lib, pack_strings, synth
    from dptok.engine import pack_presplit_words
    from oracle import oracle
    t2i = vocabs["llama32k"]
    enc, orc = Encoder(Vocab(t2i, 0)), oracle.OracleVocab(t2i)

    def one(s, what):
        text, offs = pack_strings([s])
        for g, r, part in zip(enc.encode_csr(text, offs), orc.encode_csr(text, offs), ("ids", "offsets", "status", "capped")):
            assert np.array_equal(g, r), (what, part, s[:30])

    one("the first call", "before")
    text, offs = pack_strings(synth.unpack(*synth.random_ascii_corpus(64, 200, seed=13)))
    ids, id_off, st, _ = orc.encode_csr(text, offs)
    ids, id_off, st = (np.ascontiguousarray(a, dtype=t) for a, t in ((ids, np.int32), (id_off, np.uint64), (st, np.int32)))
    n, n_tok, n_bytes = len(st), len(ids), int(offs[-1])
    assert n == 64 and n_bytes > 4096 and 4 * n_tok > 4096 and not st.any()   # more than the first buffers, in and out
    ref = spans_ref.expected(t2i, "raw", text, offs, None, ids, id_off, st)
    end, word, ss = np.zeros(n_tok, np.uint32), np.zeros(n_tok, np.uint32), np.full(n, -1, np.int32)
    rc = _lib.lib().dpt_token_spans_host(enc.handle, enc.vocab.handle, _lib.DPT_MODE_RAW, text.ctypes.data, n_bytes,
                                         offs.ctypes.data, None, n, ids.ctypes.data, id_off.ctypes.data, st.ctypes.data,
                                         end.ctypes.data, word.ctypes.data, ss.ctypes.data)
    _lib.check(rc, "dpt_token_spans_host")
    for g, r in zip((end, word, ss), ref):
        assert np.array_equal(g, r)
    for s in ("", "after the spans call", "é中😀 x"):
        one(s, "after the spans call")
    got = enc.encode_csr_spans(text, offs)
    assert np.array_equal(got[0], ids) and np.array_equal(got[1], id_off) and np.array_equal(got[2], st)
    for g, r in zip(got[4:], ref):
        assert np.array_equal(g, r)
    for s in ("", "plain ascii words", "naïve 中文 😀 end"):
        one(s, "after encode_csr_spans")
    text, offs, cut, _, _ = pack_presplit_words([["▁pre", "▁split", "words", "▁é中"]])
    for g, r, part in zip(enc.encode_csr(text, offs, mode="presplit", cut_mask=cut),
                          orc.encode_csr(text, offs, mode=oracle.PRESPLIT, cut_mask=cut), ("ids", "offsets", "status", "capped")):
        assert np.array_equal(g, r), ("presplit", part)


def test_zero_copy_calls_between_the_decode_roundtrip_and_spans_paths(vocabs):
    """Every host path of one ctx stages in the same buffers (dpt_host.cpp Stager), and two rules hold them
    together: a side that does not grow stays where it is, and a one-string zero-copy encode looks the pinned
    buffers' device addresses up again after a call moved them.  dpt_decode_host is the one call that stages
    twice -- its out side grows, and moves, between the sizes pass and the decode pass while the in side, ids
    included, must stay put.  One Encoder's ctx throughout, the decode calls through the C-ABI with that ctx: a
    one-string encode (4096-byte pinned buffers, addresses looked up), dpt_decode_host on 64 strings of 200 bytes
    whose ids come from the oracle (so no encode call has grown the buffers), one-string encodes,
    dpt_roundtrip_host on the same batch, one-string encodes, dpt_token_spans_host, one-string encodes and a
    PRESPLIT one -- encodes and spans exact against the oracle and tests/spans_ref.py, the decode against
    tests/decode_ref.py, every round-trip verdict RT_EQUAL."""
    import decode_ref
    import spans_ref
    from dptok import Detok, Encoder, Vocab, _lib, pack_strings, synth
    from dptok.engine import pack_presplit_words
    from oracle import oracle
    t2i = vocabs["llama32k"]
    enc, orc, detok = Encoder(Vocab(t2i, 0)), oracle.OracleVocab(t2i), Detok(t2i, "sp")
    L, STRIP = _lib.lib(), _lib.DPT_DECODE_STRIP_SPACE

    def ones(what, strs=("", "plain ascii words", "naïve 中文 😀 end")):
        for s in strs:
            text, offs = pack_strings([s])
            for g, r, part in zip(enc.encode_csr(text, offs), orc.encode_csr(text, offs), ("ids", "offsets", "status", "capped")):
                assert np.array_equal(g, r), (what, part, s[:30])

    ones("before", ("the first call",))
    text, offs = pack_strings(synth.unpack(*synth.random_ascii_corpus(64, 200, seed=13)))
    ids, id_off, st, _ = orc.encode_csr(text, offs)
    ids, id_off, st = (np.ascontiguousarray(a, dtype=t) for a, t in ((ids, np.int32), (id_off, np.uint64), (st, np.int32)))
    n, n_tok, n_bytes = len(st), len(ids), int(offs[-1])
    assert n == 64 and n_bytes > 4096 and 4 * n_tok > 4096 and not st.any()   # more than the first buffers, in and out
    by_id = decode_ref.pieces_by_id(decode_ref.pairs_of(t2i), "sp")
    wraw, woff, wst, ok = decode_ref.expected_decode(by_id, ids, id_off, st, strip=True)
    assert ok.all() and len(wraw) == n_bytes and 8 * n + 4 * n + 16 < 4096   # the sizes pass fits the first out buffer, the bytes do not

    out, out_off, dst = np.zeros(n_bytes + 64, np.uint8), np.full(n + 1, 7, np.uint64), np.full(n, -1, np.int32)
    _lib.check(L.dpt_decode_host(enc.handle, detok.handle, ids.ctypes.data, id_off.ctypes.data, st.ctypes.data, n, STRIP,
                                 out.ctypes.data, len(out), out_off.ctypes.data, dst.ctypes.data), "dpt_decode_host")
    assert np.array_equal(out_off, woff) and np.array_equal(dst, wst) and np.array_equal(out[:n_bytes], wraw)
    assert out[:n_bytes].tobytes() == text[:n_bytes].tobytes()
    ones("after the decode call")

    rt, fd = np.full(n, -1, np.int32), np.zeros(n, np.uint32)
    _lib.check(L.dpt_roundtrip_host(enc.handle, detok.handle, ids.ctypes.data, id_off.ctypes.data, st.ctypes.data,
                                    text.ctypes.data, offs.ctypes.data, n, STRIP, rt.ctypes.data, fd.ctypes.data), "dpt_roundtrip_host")
    assert (rt == _lib.RT_EQUAL).all()
    ones("after the round trip")

    ref = spans_ref.expected(t2i, "raw", text, offs, None, ids, id_off, st)
    end, word, ss = np.zeros(n_tok, np.uint32), np.zeros(n_tok, np.uint32), np.full(n, -1, np.int32)
    _lib.check(L.dpt_token_spans_host(enc.handle, enc.vocab.handle, _lib.DPT_MODE_RAW, text.ctypes.data, n_bytes,
                                      offs.ctypes.data, None, n, ids.ctypes.data, id_off.ctypes.data, st.ctypes.data,
                                      end.ctypes.data, word.ctypes.data, ss.ctypes.data), "dpt_token_spans_host")
    for g, r in zip((end, word, ss), ref):
        assert np.array_equal(g, r)
    ones("after the spans call")
    text, offs, cut, _, _ = pack_presplit_words([["▁pre", "▁split", "words", "▁é中"]])
    for g, r, part in zip(enc.encode_csr(text, offs, mode="presplit", cut_mask=cut),
                          orc.encode_csr(text, offs, mode=oracle.PRESPLIT, cut_mask=cut), ("ids", "offsets", "status", "capped")):
        assert np.array_equal(g, r), ("presplit", part)


TOY = {"a": 0, "b": 1, "ab": 2, "▁a": 3}   # (the vocabulary of test_llama_sp.py test_encode_presplit_empty_word_order)


def test_encode_word_atoms_lists():
    """Encoder.encode_word_atoms ends in csr_lists: per string the oracle's ids and status, ([], ok) for a
    string of no words; a word with no tokenization fails its whole string."""
    from dptok import Encoder, STATUS_NO_TOKENIZATION, STATUS_OK, Vocab
    from dptok.engine import pack_word_atoms
    from oracle import oracle
    strings = [[], [["a", "b"]], [["a"], ["z"], ["b"]], [["▁", "a"]], [["a", "b"], ["▁", "a"], ["b"]], [["b"]]]
    got = Encoder(Vocab(TOY, 0)).encode_word_atoms(strings)
    text, offs, cut = pack_word_atoms(strings)
    ids, id_off, st, _ = oracle.OracleVocab(TOY).encode_csr(text, offs, mode=oracle.ATOMS, cut_mask=cut)
    want = [([], STATUS_OK) if not words else (ids[int(id_off[i]):int(id_off[i + 1])].tolist(), int(st[i]))
            for i, words in enumerate(strings)]
    assert got == want
    assert got[0] == ([], STATUS_OK) and got[1] == ([2], STATUS_OK) and got[2][1] == STATUS_NO_TOKENIZATION
    assert got[3] == ([3], STATUS_OK) and got[4] == ([2, 3, 1], STATUS_OK)


def test_encode_csr_spans_from_a_nonzero_offset():
    """A host batch may start anywhere in its buffers: three pre-split strings packed after 5 junk bytes, the
    cut mask moved the same way, give what the batch packed at offset 0 gives (and its ids are the oracle's)."""
    from dptok import Encoder, Vocab
    from dptok.engine import pack_presplit_words
    from oracle import oracle
    text, offs, cut, _, _ = pack_presplit_words([["ab", "▁a"], ["▁a", "b", "a"], ["a", "b", "ab"]])
    enc = Encoder(Vocab(TOY, 0))
    at0 = enc.encode_csr_spans(text, offs, mode="presplit", cut_mask=cut)
    ref = oracle.OracleVocab(TOY).encode_csr(text, offs, mode=oracle.PRESPLIT, cut_mask=cut)
    for g, r in zip(at0[:4], ref):
        assert np.array_equal(g, r)
    assert at0[0].tolist() == [2, 3, 3, 1, 0, 0, 1, 2] and not at0[2].any() and not at0[6].any()
    junk = np.frombuffer(b"zz zz", dtype=np.uint8)
    at5 = enc.encode_csr_spans(np.concatenate([junk, text]), offs + np.uint64(5), mode="presplit",
                               cut_mask=np.concatenate([np.ones(5, np.uint8), cut]))
    assert len(at5) == 7
    for g, r in zip(at5, at0):
        assert g.dtype == r.dtype and np.array_equal(g, r)


def test_encode_device_null_pointers_as_plain_ints():
    """The device-pointer methods pass plain ints to the void* arguments: 0 must arrive as NULL (no capped
    output, no cut mask, the default stream)."""
    import torch
    from dptok import Encoder, Vocab, pack_strings
    from oracle import oracle
    text, offs = pack_strings(["ab", "", "a ab", "b"])
    n, n_bytes = len(offs) - 1, int(offs[-1])
    dev = torch.device("cuda", 0)
    d_text = torch.tensor(text, device=dev)
    d_offs = torch.tensor(offs.view(np.int64), device=dev)
    d_ids = torch.full((n_bytes + 1,), -1, dtype=torch.int32, device=dev)
    d_idoff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    Encoder(Vocab(TOY, 0)).encode_device(d_text.data_ptr(), n_bytes, d_offs.data_ptr(), n, d_ids.data_ptr(), n_bytes + 1,
                                         d_idoff.data_ptr(), d_st.data_ptr(), 0, 0, 0)
    torch.cuda.synchronize()
    ids, id_off, st, _ = oracle.OracleVocab(TOY).encode_csr(text, offs)
    assert d_idoff.cpu().numpy().tolist() == id_off.tolist() and d_st.cpu().numpy().tolist() == st.tolist()
    assert d_ids.cpu().numpy()[:len(ids)].tolist() == ids.tolist() and ids.tolist() == [3, 1, 3, 3, 1]
    assert st.tolist() == [0, 2, 0, 1]   # ("" is the reference's IndexError, "b" has no tokenization)
