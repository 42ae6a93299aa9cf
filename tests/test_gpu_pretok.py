"""Device-side llama-mode pre-tokenization (include/dpt.h dpt_pretok_sizes / dpt_pretok_write) against the
plain-Python rule of tests/pretok_ref.py, byte for byte: out_len, pre_status, the pre-split text and the cut
mask, every output between 0xAA canaries.  The recorded SentencePiece texts on two tables, strings on the
kernel's 64-byte round edges, malformed and refused input, the call shapes of the device contract, the chain into
dpt_encode, and the drop-in with ``device_pretokenize=True`` against the recorded ids."""
import numpy as np
import pytest

from conftest import load_golden

import pretok_ref as pr
import split_harness

pytestmark = pytest.mark.gpu

WS = pr.WS
LITERALS = ["<unk>", "<s>", "</s>"]
# a known set in every length class: most of ASCII ('\n', '\t', '~' and '^' are not in it), accented Latin, half of
# the Arabic block the texts use, some CJK, some emoji
KNOWN = (set(range(0x20, 0x7E)) - {ord("^")}) | {ord(c) for c in "éèüßñçàâîœ€"} | set(range(0x0621, 0x0636)) | \
    set(range(0x4E00, 0x4F00)) | set(range(0x1F600, 0x1F620))


def _t2i(known=KNOWN, runs_ok=True, bos="<s>"):
    pieces = ["<0x%02X>" % b for b in range(256)] + LITERALS + [chr(cp) for cp in sorted(known)] + ["▁", "▁the"]
    if not runs_ok:
        pieces.append("▁▁")
    return {p: i for i, p in enumerate(dict.fromkeys(pieces))}


def _pair(known=KNOWN, runs_ok=True, bos="<s>", literals=LITERALS):
    """(Pretok on device 0, the model's table) of one toy vocabulary."""
    from dptok import Pretok
    t2i = _t2i(known, runs_ok, bos)
    table = pr.build_table(pr.vocab_pieces(t2i), bos.encode(), [x.encode() for x in literals])
    assert isinstance(table, pr.Table) and table.runs_ok == runs_ok and table.known >= set(known)
    return Pretok(t2i, bos, literals, 0), table


@pytest.fixture(scope="module")
def tables():
    return {"runs_ok": _pair(), "no_runs": _pair(runs_ok=False), "no_bos": _pair(bos="")}


def _check(pair, strings, **kw):
    pretok, table = pair
    return split_harness.check(pretok, lambda strs: pr.presplit(table, strs), strings, **kw)


def _ascii(n, length, seed):
    from dptok import synth
    text, offs = synth.random_ascii_corpus(n, length, seed=seed)
    raw = text.tobytes()
    return [raw[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]


# ------------------------------------------------------------------ 1. the recorded texts

@pytest.mark.parametrize("which", ["runs_ok", "no_runs"])
def test_fixture_batch(which, tables):
    texts = [c["text"] for c in load_golden("sp_llama_cases.json.gz")["cases"] if c["tokenizer"] == "sp"]
    assert len(texts) == 565
    strings = [t.encode("utf-8", "surrogatepass") for t in texts]
    st, ln, text2, _ = _check(tables[which], strings)
    n_ok = int((st == 0).sum())
    assert (n_ok == 292) if which == "runs_ok" else (100 < n_ok < 292)       # "  " is refused without runs_ok
    assert b"<0xF0><0x9F>" in text2 and "😀".encode() in text2 and b"<0xD9>" in text2 and "中".encode() in text2
    assert int(ln.max()) > 500


# ------------------------------------------------------------------ 2. round edges

EDGE_CHARS = ["é", "ö", "中", "龍", "😀", "𝄞", "ب", "ي", "€", "…"]          # known and unknown, 2 to 4 bytes


def edge_length_strings():
    """Strings on the kernel's 64-byte round edges, none refused with runs_ok (also run by test_gpu_wave_stride.py)."""
    base = _ascii(1, 200, seed=21)[0].replace(b"<", b"(")
    strings = [base[:L] for L in (0, 1, 63, 64, 65, 127, 128, 129, 200)]
    for c in EDGE_CHARS:
        for at in (61, 62, 63, 125, 126, 127):
            strings.append(b"a" * at + c.encode() + b"bc")
            strings.append(b"a" * at + c.encode())                           # ... and ending the string
    strings.append("𝄞".encode() * 50)                                        # 24-byte expansions across many output rounds
    strings.append(("😀" * 37 + " " + "𝄞é" * 20).encode())
    strings.append(b" ".join([b"x"] * 100))                                  # 3-byte expansions, a word per character
    strings.append(b"\n" * 130)
    return strings


def test_edge_length_strings(tables):
    strings = edge_length_strings()
    table = tables["runs_ok"][1]
    assert {(len(c.encode()), ord(c) in table.known) for c in EDGE_CHARS} == {(L, k) for L in (2, 3, 4) for k in (True, False)}
    st, ln, _, _ = _check(tables["runs_ok"], strings)
    assert not st.any() and int(ln.max()) == 6 + 50 * 24
    _check(tables["no_bos"], strings, pad=1, off0=0, out0=0)


# ------------------------------------------------------------------ 3. malformed and refused input

MALFORMED = [b"a\xc3", b"\xe2\x82", b"ab\xf0\x9f\x98", b"\xf0", b"\xc0\xaf", b"\xc1\xbf", b"\xe0\x80\xaf", b"\xe0\x9f\xbf",
             b"\xf0\x80\x80\xaf", b"\xf0\x8f\xbf\xbf", b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80",
             b"\xff", b"\xfe\xfe", b"\x80", b"a\xbfb", b"\xc3\xa9\xa9", b"\xe2\x82\xac\x80", b"\xc3\x28", b"\xe2\x28\xa1",
             b"\xe2\x82\x28", b"\xf0\x28\x8c\xbc", b"\xf0\x9f\x28\xbc", b"\xf0\x9f\x98\x28"]


WELL_FORMED = ["é€😀".encode(), b"\xed\x9f\xbf", b"\xee\x80\x80", b"\xf4\x8f\xbf\xbf", b"\xf0\x90\x80\x80", b"\xe0\xa0\x80", b"\xc2\x80"]
# two spaces: refused only without runs_ok -- inside a round, across its boundary, at the end
SPACES = [b"a  b", b"a b", b"a" * 63 + b"  b", b"a" * 62 + b"  b", b"ab  ", b"a" * 127 + b"  ", b"a \n b", b"a" * 63 + b" b c"]


def malformed_and_refused_strings():
    """MALFORMED in its paddings, truncated characters before continuation bytes, WELL_FORMED, refused strings and
    the special-token literals on and off the round edges (also run by test_gpu_wave_stride.py)."""
    strings = []
    for m in MALFORMED:
        strings += [m, b"ok " + m, m + b" ok", b"a" * 62 + m, b"a" * 63 + m + b"z" * 70]
    # a truncated character directly followed by the next string's continuation bytes: never completed
    for a, b in ((b"a\xe2\x82", b"\xac b"), (b"ab\xf0\x9f", b"\x98\x80"), (b"x" * 63 + b"\xc3", b"\xa9"), (b"q\xe2", b"\x82\xac")):
        strings += [a, b, b"fine"]
    strings += WELL_FORMED
    # refused though well-formed
    strings += [b" x", b" ", "a▁b".encode(), "▁".encode(), b"x" * 63 + "▁".encode(), b"x" * 62 + "▁".encode()]
    # the literals: at the start, at the end, across a round boundary; a proper prefix at the string's end
    lits = [b"<s>", b"</s>", b"<unk>"]
    for x in lits:
        strings += [x, x + b"a", b"a" + x, b"ab " + x + b" cd", b"a" * 62 + x + b"b", b"a" * 63 + x, b"a" * 60 + x + b"c" * 70,
                    b"a" * 126 + x]
        for k in range(1, len(x)):
            strings += [b"abc" + x[:k], b"a" * (64 - k) + x[:k], x[:k] + b"<"]
    strings += [b"abc<s", b">x", b"<<s", b"<<s>", b"a < b > c", b"<s >", b"< s>", b"<S>"]
    return strings


def test_malformed_and_refused(tables):
    strings, well = malformed_and_refused_strings(), WELL_FORMED
    want = _check(tables["runs_ok"], strings)
    st = dict(zip(strings, want[0].tolist()))
    assert all(st[m] == pr.NEEDS_HOST for m in MALFORMED) and all(st[w] == 0 for w in well)
    assert st[b"abc<s"] == 0 and st[b">x"] == 0 and st[b"<<s>"] == 6 and st[b"a" * 126 + b"<unk>"] == 6 and st[b"\xac b"] == 6
    assert not _check(tables["runs_ok"], SPACES)[0].any()
    assert _check(tables["no_runs"], SPACES)[0].tolist() == [6, 0, 6, 6, 6, 6, 0, 0]


# ------------------------------------------------------------------ 4. call shapes

def test_call_shapes(tables):
    import torch
    rng = np.random.default_rng(5)
    pool = _ascii(64, 256, seed=33)
    extra = ["é", "中", "😀", "𝄞", "\n", "ö", " ", "  "]
    strings = []
    for i in range(5000):                                                    # more strings than waves in the grid
        s = pool[i % 64][int(rng.integers(0, 200)):][:int(rng.integers(0, 41))]
        if i % 7 == 0:
            s += extra[(i // 7) % len(extra)].encode() + s[:3]
        strings.append(s)
    st, _, _, _ = _check(tables["runs_ok"], strings, pad=5, off0=(1 << 33) + 1, out0=(1 << 32) + 3)
    assert 0 < int((st != 0).sum()) < 2500 and b"" in strings
    _check(tables["no_bos"], strings[:300] + [b"", b"", b"x"], pad=1, off0=9, out0=0)
    assert _check(tables["no_bos"], [b"", b""])[1].tolist() == [0, 0]        # nothing at all, status 0
    assert _check(tables["runs_ok"], [b""])[2] == b"<s>"
    # n_str == 0 launches nothing (and needs no valid pointers beyond non-null ones)
    pretok = tables["runs_ok"][0]
    canary = torch.full((64,), 0xAA, dtype=torch.uint8, device="cuda:0")
    p = canary.data_ptr()
    pretok.sizes_device(p, p, 0, p, p)
    pretok.write_device(p, p, 0, p, p, p, p)
    torch.cuda.synchronize()
    assert bool((canary == 0xAA).all())
    from dptok import DptError
    with pytest.raises(DptError):
        pretok.sizes_device(p, 0, 1, p, p)
    with pytest.raises(DptError):
        pretok.write_device(p, p, 1, p, p, p, 0)
    # on a side stream, from torch tensors
    s = torch.cuda.Stream()
    blob = np.frombuffer(b"".join(strings[:500]), dtype=np.uint8).copy()
    offs = np.concatenate([[0], np.cumsum([len(x) for x in strings[:500]])]).astype(np.int64)
    with torch.cuda.stream(s):
        text2, offs2, cut, pre = pretok.presplit(torch.from_numpy(blob).cuda(), torch.from_numpy(offs).cuda())
    s.synchronize()
    want = pr.presplit(tables["runs_ok"][1], strings[:500])
    assert pre.cpu().numpy().tolist() == want[0].tolist() and np.diff(offs2.cpu().numpy()).tolist() == want[1].tolist()
    assert text2.cpu().numpy().tobytes() == want[2] and cut.cpu().numpy().tobytes() == want[3]


# ------------------------------------------------------------------ 5. chained into dpt_encode

def test_presplit_feeds_encode_on_the_device(vocabs):
    import torch
    from dptok import Encoder, Pretok, Vocab, synth
    from dptok.engine import csr_lists
    t2i = vocabs["llama32k"]
    lits = [x for x in LITERALS if x in t2i]
    assert "<s>" in t2i
    pretok = Pretok(t2i, "<s>", lits, 0)
    table = pr.build_table(pr.vocab_pieces(t2i), b"<s>", [x.encode() for x in lits])
    text, offs = synth.s2orc_like_corpus(2000)
    raw, o = text.tobytes(), offs.astype(np.int64)
    strings = [raw[o[i]:o[i + 1]] for i in range(2000)]
    st, ln, text2, cut = pr.presplit(table, strings)
    assert int((st == 0).sum()) > 1900
    enc = Encoder(Vocab(t2i, 0))
    offs2 = np.concatenate([[0], np.cumsum(ln.astype(np.int64))]).astype(np.uint64)
    want = enc.encode_packed_presplit(np.frombuffer(text2 + b"\0", dtype=np.uint8), offs2,
                                      np.frombuffer(cut + b"\0", dtype=np.uint8), (ln > 0).astype(np.int64))
    d_text2, d_offs2, d_cut, d_pre = pretok.presplit(torch.from_numpy(text.copy()).cuda(), torch.from_numpy(o.copy()).cuda())
    assert d_pre.cpu().numpy().tolist() == st.tolist() and d_text2.cpu().numpy().tobytes() == text2
    n, n2 = 2000, int(d_text2.numel())
    ids = torch.empty(n2, dtype=torch.int32, device="cuda:0")
    id_off = torch.empty(n + 1, dtype=torch.int64, device="cuda:0")
    status = torch.empty(n, dtype=torch.int32, device="cuda:0")
    enc.encode_device(d_text2.data_ptr(), n2, d_offs2.data_ptr(), n, ids.data_ptr(), n2, id_off.data_ptr(), status.data_ptr(),
                      cut_ptr=d_cut.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, mode="presplit")
    id_off_h = id_off.cpu().numpy().view(np.uint64)
    got = csr_lists(ids[:int(id_off_h[-1])].cpu().numpy(), id_off_h, status.cpu().numpy(), none=(ln == 0), keep_failed=False)
    assert got == want and sum(len(g[0]) for g in got) > 300_000


# ------------------------------------------------------------------ 6. the drop-in

def test_self_check_stops_a_normalising_tokenizer():
    pytest.importorskip("sentencepiece")
    import unicodedata
    from dptok import DptError
    from sp_llama import SPLlama
    from packages.tokenizer_utils import dp_tokenize_llama

    class Normalising(SPLlama):
        def encode(self, text):
            return super().encode(unicodedata.normalize("NFKC", text))

    with pytest.raises(DptError, match="probe"):
        dp_tokenize_llama(Normalising(), "llama", device_pretokenize=True)
    dp_tokenize_llama(Normalising(), "llama")                                # the default path takes any tokenizer

    class Folding(SPLlama):                                                  # whitespace folding
        def encode(self, text):
            return super().encode(text.replace("  ", " "))

    with pytest.raises(DptError, match="a  b"):
        dp_tokenize_llama(Folding(), "llama", device_pretokenize=True)


@pytest.mark.parametrize("kind", ["sp", "hf"])
def test_drop_in_with_device_pretokenize(kind):
    pytest.importorskip("sentencepiece")
    import torch
    from sp_llama import SPLlama, hf_llama
    from packages.tokenizer_utils import dp_tokenize_llama
    tok = SPLlama() if kind == "sp" else hf_llama()
    cases = [c for c in load_golden("sp_llama_cases.json.gz")["cases"] if c["tokenizer"] == kind]
    texts = [c["text"] for c in cases]
    on, _ = dp_tokenize_llama(tok, "llama", device_pretokenize=True)
    off, _ = dp_tokenize_llama(tok, "llama")
    assert not hasattr(off, "pretok_stats") and on.pretok_stats == (0, 0)
    good = [c for c in cases if c["status"] == 0]
    assert len(good) > 500
    assert on.batch([c["text"] for c in good]) == [c["ids"] for c in good]
    for c in cases:
        if c["status"] != 0:                                                 # the same exception as the default path
            with pytest.raises(Exception) as want:
                off.batch([c["text"]])
            with pytest.raises(type(want.value)):
                on.batch([c["text"]])
    # the whole batch in order: the default path's outcome, exception included
    try:
        want = off.batch(texts)
    except Exception as e:   # noqa: BLE001
        with pytest.raises(type(e)) as got:
            on.batch(texts)
        assert str(got.value) == str(e)
    else:
        assert on.batch(texts) == want
        assert on.pretok_stats == (292, 273) and tuple(on.pretok_stats) == (292, 273)   # the device path produced them
    assert on("a b") == off("a b") and on.pretok_stats == (1, 0)
    assert on(" a") == off(" a") and on.pretok_stats == (0, 1)
    assert on.batch([]) == [] and on.pretok_stats == (0, 0)
    sub = [c["text"] for c in good][:200]
    assert on.batch_roundtrip(sub) == off.batch_roundtrip(sub)
    a, b = on.batch_model_inputs(sub, max_length=64, labels=True), off.batch_model_inputs(sub, max_length=64, labels=True)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    sa, sb = on.batch_spans(sub[:50]), off.batch_spans(sub[:50])
    assert sa == sb
