"""Device-side byte-level (BLOOM) pre-tokenization (include/dpt.h dpt_bytelevel_sizes / dpt_bytelevel_write) against
the plain-Python rule of tests/bytelevel_ref.py, byte for byte: out_len, pre_status, the ATOMS text and the cut mask,
every output between 0xAA canaries.  The recorded texts, strings on the kernel's 64-byte round edges, malformed
input, the call shapes of the device contract, the chain into dpt_encode, and the drop-in with
``device_pretokenize=True`` against the recorded ids."""
import tempfile

import numpy as np
import pytest

from conftest import load_golden

import bytelevel_ref as br
import split_harness

pytestmark = pytest.mark.gpu

TABLE = br.build_table(br.BLOOM_SEPARATORS)


@pytest.fixture(scope="module")
def splitter():
    from dptok import ByteLevelSplit
    return ByteLevelSplit(device=0)


def _check(split, strings, **kw):
    return split_harness.check(split, lambda strs: br.split(TABLE, strs), strings, **kw)


# ------------------------------------------------------------------ 1. the recorded texts

def test_fixture_batch(splitter):
    cases = load_golden("bloom_pretok_cases.json.gz")["cases"]
    cases = cases[:300] + cases[700:]                                        # bloom_texts() and the random strings
    strings = [c["text"].encode("utf-8") for c in cases]
    st, ln, text2, cut = _check(splitter, strings)
    assert not st.any() and int(ln.max()) > 150 and b"" in strings
    # ... which are the recorded words, atom by atom
    o = np.concatenate([[0], np.cumsum(ln.astype(np.int64))])
    for i in range(0, len(cases), 5):
        words = br.words_of(text2[o[i]:o[i + 1]], cut[o[i]:o[i + 1]])
        assert ["".join(w) for w in words] == cases[i]["words"] and all(len(a) == 1 for w in words for a in w)


# ------------------------------------------------------------------ 2. round edges

def round_edge_strings():
    """Strings on the kernel's 64-byte round edges, all well-formed (also run by test_gpu_wave_stride.py)."""
    base = (b"abcdefghij klmno,pqrst. uvwxyz [01234] 56789! " * 5)
    strings = [base[:L] for L in (0, 1, 63, 64, 65, 127, 128, 129, 200)]
    strings += [b"a" * L for L in (1, 63, 64, 65, 127, 128, 129)]
    sep3, emoji = "。".encode(), "😀".encode()
    for at in (63, 127):                                                     # byte `at` is lane 63 of a round
        strings += [b"a" * at + b" b", b"a" * at + b" bcd e",                # a space in lane 63, then a non-separator
                    b"a" * at + b" .", b"a" * at + b"  b", b"a" * at + b" " + sep3 + b"x", b"a" * at + b" \xc2\xa0",   # ... a separator
                    b"a" * at + b" " + "é".encode(), b"a" * at + b" " + emoji,
                    b"a" * at + b" ",                                        # ... the string's last byte
                    b"a" * at + b".b", b"a" * at + b". b", b"a" * (at - 2) + sep3 + b"b", b"a" * (at - 2) + sep3 + b" b",   # a separator ends the round
                    b"a" * (at - 1) + b"  b", b"a" * (at - 1) + b". b"]
        for k in range(1, 3 + 1):                                            # U+3002 with k bytes before the edge (k = 3: ending it)
            strings += [b"a" * (at + 1 - k) + sep3 + b"b", b"a" * (at + 1 - k) + sep3, b"a" * (at - k) + b" " + sep3 + b" b",
                        b"a" * (at + 1 - k) + sep3 + sep3 + b"b", b"a" * (at + 1 - k) + "、".encode() + b" b"]
        for k in range(1, 4 + 1):                                            # a four-byte character likewise
            strings += [b"a" * (at + 1 - k) + emoji + b"b", b"a" * (at + 1 - k) + emoji + b" b", b"a" * (at + 1 - k) + emoji,
                        b"a" * (at - k) + b" " + emoji + b"."]
        strings += [b"a" * (at - 1) + "\u0085".encode() + b"b", b"a" * at + "\u00a0".encode() + b"b", b"a" * at + "é".encode() + b" b"]
    strings += [b" " * L for L in (1, 2, 3, 63, 64, 65, 130)]                # runs of spaces
    strings += [b"a" + b" " * L + b"b" for L in (1, 2, 3, 62, 63, 64, 127)]
    strings += [b" a", b"  a", b"a ", b"a  ", b" a b ", b"x  y   z    w"]
    strings += ["".join(chr(c) for c in br.BLOOM_SEPARATORS).encode() * 3, b". , ! ? ( ) |" * 12, sep3 * 50, b"\n" * 130]   # only separators
    strings += ["中文字龍".encode() * 20, emoji * 40, "éüßñ".encode() * 33, "ءبي".encode() * 30, ("。" + "中" * 21).encode() * 3]   # only bytes >= 0x80
    strings += ["a[b]c (d|e) f.g,h!i?j".encode(), bytes(range(0x80)) * 2, bytes(range(0x7F, -1, -1))]
    return strings


def test_round_edges(splitter):
    strings, emoji = round_edge_strings(), "😀".encode()
    st, ln, text2, cut = _check(splitter, strings)
    assert not st.any()
    d = dict(zip(strings, zip(ln.tolist(), range(len(strings)))))
    assert d[b"a" * 64][0] == 64 and d[b" " * 64][0] == 128 and d[b""][0] == 0 and d[emoji * 40][0] == 320
    o = np.concatenate([[0], np.cumsum(ln.astype(np.int64))])
    words = lambda s: ["".join(w) for w in br.words_of(text2[o[d[s][1]]:o[d[s][1] + 1]], cut[o[d[s][1]]:o[d[s][1] + 1]])]   # noqa: E731
    assert words(b"a" * 63 + b" b") == ["a" * 63, "Ġb"] and words(b"a" * 63 + b" .") == ["a" * 63, "Ġ."]
    assert words(b"a" * 63 + b" ") == ["a" * 63, "Ġ"] and words(b"a" * 63 + b".b") == ["a" * 63, ".", "b"]
    _check(splitter, strings, pad=1, off0=0, out0=0)


# ------------------------------------------------------------------ 3. malformed input

MALFORMED = [b"a\xc3", b"\xe2\x82", b"ab\xf0\x9f\x98", b"\xf0", b"\xc0\xaf", b"\xc1\xbf", b"\xe0\x80\xaf", b"\xe0\x9f\xbf",
             b"\xf0\x80\x80\xaf", b"\xf0\x8f\xbf\xbf", b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80",
             b"\xff", b"\xfe\xfe", b"\x80", b"a\xbfb", b"\xc3\xa9\xa9", b"\xe2\x82\xac\x80", b"\xc3\x28", b"\xe2\x28\xa1",
             b"\xe2\x82\x28", b"\xf0\x28\x8c\xbc", b"\xf0\x9f\x28\xbc", b"\xf0\x9f\x98\x28"]


WELL_FORMED = ["é€😀".encode(), b"\xed\x9f\xbf", b"\xee\x80\x80", b"\xf4\x8f\xbf\xbf", b"\xf0\x90\x80\x80", b"\xe0\xa0\x80", b"\xc2\x80"]


def malformed_strings():
    """MALFORMED in its paddings, truncated characters before continuation bytes, and WELL_FORMED (also run by
    test_gpu_wave_stride.py)."""
    strings = []
    for m in MALFORMED:
        strings += [m, b"ok " + m, m + b" ok", b"a" * 62 + m, b"a" * 63 + m + b"z" * 70, b"a" * 130 + m]
    # a truncated character directly followed by the next string's continuation bytes: never completed
    for a, b in ((b"a\xe2\x82", b"\xac b"), (b"ab\xf0\x9f", b"\x98\x80"), (b"x" * 63 + b"\xc3", b"\xa9"), (b"q\xe2", b"\x82\xac"),
                 (b"x" * 62 + b"\xe3\x80", b"\x82")):
        strings += [a, b, b"fine"]
    return strings + WELL_FORMED


def test_malformed(splitter):
    strings, well = malformed_strings(), WELL_FORMED
    want = _check(splitter, strings)
    st = dict(zip(strings, want[0].tolist()))
    assert all(st[m] == br.NEEDS_HOST for m in MALFORMED) and all(st[w] == 0 for w in well)
    assert st[b"\xac b"] == 6 and st[b"fine"] == 0 and st[b"x" * 62 + b"\xe3\x80"] == 6 and int((want[0] != 0).sum()) > 150


# ------------------------------------------------------------------ 4. call shapes

OTHER_SEPARATORS = [0x20, ord("o"), 0x4E2D, 0x1F600, 0xF6]   # a second separator set: one in every length class


def test_call_shapes(splitter):
    import torch
    rng = np.random.default_rng(5)
    pool = ("the quick (brown) fox, jumps. over | the lazy dog! " * 8).encode()
    extra = ["é", "中", "😀", "。", "\n", "ö", " ", "  ", "、 ", "\u2003"]
    strings = []
    for i in range(3000):
        a = int(rng.integers(0, 200))
        s = pool[a:a + int(rng.integers(0, 41))]
        if i % 7 == 0:
            s += extra[(i // 7) % len(extra)].encode() + s[:3]
        strings.append(s)
    st, _, _, _ = _check(splitter, strings, pad=5, off0=(1 << 33) + 1, out0=(1 << 32) + 3)
    assert not st.any() and b"" in strings
    assert _check(splitter, [b"", b""])[1].tolist() == [0, 0]
    # n_str == 0 launches nothing (and needs no valid pointers beyond non-null ones)
    canary = torch.full((64,), 0xAA, dtype=torch.uint8, device="cuda:0")
    p = canary.data_ptr()
    splitter.sizes_device(p, p, 0, p, p)
    splitter.write_device(p, p, 0, p, p, p, p)
    torch.cuda.synchronize()
    assert bool((canary == 0xAA).all())
    from dptok import DptError
    for args in ((0, p, 1, p, p), (p, 0, 1, p, p), (p, p, 1, 0, p), (p, p, 1, p, 0)):
        with pytest.raises(DptError):
            splitter.sizes_device(*args)
    for k in range(7):
        args = [p, p, 1, p, p, p, p]
        if k != 2:
            args[k] = 0
            with pytest.raises(DptError):
                splitter.write_device(*args)
    with pytest.raises(DptError):
        from dptok import ByteLevelSplit
        ByteLevelSplit([0x2E])                                               # a set without U+0020
    # on a side stream, from torch tensors; another separator set
    s = torch.cuda.Stream()
    blob = np.frombuffer(b"".join(strings[:500]), dtype=np.uint8).copy()
    offs = np.concatenate([[0], np.cumsum([len(x) for x in strings[:500]])]).astype(np.int64)
    from dptok import ByteLevelSplit
    other = ByteLevelSplit(OTHER_SEPARATORS)
    with torch.cuda.stream(s):
        text2, offs2, cut, pre = other.split(torch.from_numpy(blob).cuda(), torch.from_numpy(offs).cuda())
    s.synchronize()
    want = br.split(br.build_table(OTHER_SEPARATORS), strings[:500])
    assert pre.cpu().numpy().tolist() == want[0].tolist() and np.diff(offs2.cpu().numpy()).tolist() == want[1].tolist()
    assert text2.cpu().numpy().tobytes() == want[2] and cut.cpu().numpy().tobytes() == want[3]
    empty = splitter.split(torch.zeros(0, dtype=torch.uint8, device="cuda:0"), torch.zeros(1, dtype=torch.int64, device="cuda:0"))
    assert [int(t.numel()) for t in empty] == [0, 1, 0, 0]


# ------------------------------------------------------------------ 5. chained into dpt_encode; 6. the drop-in

@pytest.fixture(scope="module")
def bloom():
    from bloom_fixture import bloom_tokenizer, make_hf_cache
    with tempfile.TemporaryDirectory() as d:
        hf = make_hf_cache(d)
        yield bloom_tokenizer(hf), hf


def test_split_feeds_encode_on_the_device(splitter, bloom):
    import torch
    from bloom_fixture import bloom_texts
    from dptok.engine import csr_lists
    from packages.tokenizer_utils import dp_tokenize_bloom
    tokz, hf = bloom
    off, _ = dp_tokenize_bloom(tokz, hf)
    texts = bloom_texts()
    want = off.batch(texts)
    from dptok import pack_strings
    text, offs = pack_strings(texts)
    d_text2, d_offs2, d_cut, d_pre = splitter.split(torch.from_numpy(text.copy()).cuda(), torch.from_numpy(offs.view(np.int64)).cuda())
    st, ln, text2, cut = br.split(TABLE, [t.encode("utf-8") for t in texts])
    assert not d_pre.cpu().numpy().any() and d_text2.cpu().numpy().tobytes() == text2 and d_cut.cpu().numpy().tobytes() == cut
    n, n2 = len(texts), int(d_text2.numel())
    ids = torch.empty(n2, dtype=torch.int32, device="cuda:0")
    id_off = torch.empty(n + 1, dtype=torch.int64, device="cuda:0")
    status = torch.empty(n, dtype=torch.int32, device="cuda:0")
    off.engine.encode_device(d_text2.data_ptr(), n2, d_offs2.data_ptr(), n, ids.data_ptr(), n2, id_off.data_ptr(), status.data_ptr(),
                             cut_ptr=d_cut.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, mode="atoms")
    id_off_h = id_off.cpu().numpy().view(np.uint64)
    got = csr_lists(ids[:int(id_off_h[-1])].cpu().numpy(), id_off_h, status.cpu().numpy(), none=(ln == 0))
    assert [g[0] for g in got] == want and not any(g[1] for g in got) and sum(len(g[0]) for g in got) > 3000


def test_drop_in_with_device_pretokenize(bloom):
    import torch
    from packages.tokenizer_utils import dp_tokenize_bloom
    tokz, hf = bloom
    on, dec_on = dp_tokenize_bloom(tokz, hf, device_pretokenize=True)
    off, _ = dp_tokenize_bloom(tokz, hf)
    assert not hasattr(off, "pretok_stats") and on.pretok_stats == (0, 0)
    cases = load_golden("bloom_cases.json.gz")["cases"]
    assert on.batch([c["text"] for c in cases]) == [c["ids"] for c in cases] and on.pretok_stats == (len(cases), 0)
    assert on("hello  world, café 😀") == off("hello  world, café 😀") and on.pretok_stats == (1, 0)
    assert on("") == [] and on.batch([]) == [] and on.pretok_stats == (0, 0)
    sub = [c["text"] for c in cases][:60]
    assert on.batch_spans(sub) == off.batch_spans(sub)
    assert on.batch_roundtrip(sub) == off.batch_roundtrip(sub) == [None] * 60
    a, b = on.batch_model_inputs(sub, max_length=48, labels=True), off.batch_model_inputs(sub, max_length=48, labels=True)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert dec_on.batch(on.batch(sub[:20])) == sub[:20]
    # text that is not well-formed UTF-8 (a lone surrogate in a Python str) takes the host path: the same outcome
    texts = ["fine", "bad \udc80 here", "also fine"]
    try:
        want = off.batch(texts)
    except Exception as e:   # noqa: BLE001
        with pytest.raises(type(e)):
            on.batch(texts)
    else:
        assert on.batch(texts) == want
    assert on.pretok_stats == (2, 1)


def test_drop_in_on_the_bloom_scale_vocabulary():
    from bloom_fixture import bloom_tokenizer, make_hf_cache
    from packages.tokenizer_utils import dp_tokenize_bloom
    cases = load_golden("bloom_big_cases.json.gz")["cases"][:100]
    with tempfile.TemporaryDirectory() as d:
        hf = make_hf_cache(d, big=True)
        on, _ = dp_tokenize_bloom(bloom_tokenizer(hf), hf, device_pretokenize=True)
        assert on.batch([c["text"] for c in cases]) == [c["ids"] for c in cases]


def test_self_check_stops_another_pre_tokenizer(bloom):
    import json
    import os
    from tokenizers import Regex, pre_tokenizers
    from bloom_fixture import SNAPSHOT, bloom_tokenizer, make_hf_cache
    from dptok import DptError
    from packages.tokenizer_utils import dp_tokenize_bloom
    with tempfile.TemporaryDirectory() as d:
        hf = make_hf_cache(d)
        tokz = bloom_tokenizer(hf)
        level = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)
        tokz._tokenizer.pre_tokenizer = pre_tokenizers.Sequence([pre_tokenizers.Split(Regex(r" ?[^\s]+"), behavior="isolated"), level])
        with pytest.raises(DptError, match="pattern"):
            dp_tokenize_bloom(tokz, hf, device_pretokenize=True)
        dp_tokenize_bloom(tokz, hf)                                          # the default path takes any tokenizer
        tokz._tokenizer.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
        with pytest.raises(DptError, match="Sequence"):
            dp_tokenize_bloom(tokz, hf, device_pretokenize=True)
        # an alphabet character missing from tokenizer.json's vocabulary
        tokz = bloom_tokenizer(hf)
        p = os.path.join(hf, SNAPSHOT, "tokenizer.json")
        with open(p) as fh:
            tj = json.load(fh)
        tj["model"]["vocab"] = {t: i for t, i in tj["model"]["vocab"].items() if t != "Ń"}
        with open(p, "w") as fh:
            json.dump(tj, fh)
        with pytest.raises(DptError, match="0xAD"):
            dp_tokenize_bloom(tokz, hf, device_pretokenize=True)
