"""The grid-stride trips of the one-wave-per-string kernels: decode_kernel<SIZES|BYTES|ROUNDTRIP>, spans_kernel<RAW|
PRESPLIT|ATOMS>, pretok_kernel<false|true> and bytelevel_kernel<false|true> run ``for (s = wave; s < n_str; s +=
n_waves)`` on a grid that gives every string a wave of its own up to 2^20 blocks of four waves, so a wave takes a
second string -- and must start it from a clean state -- only in calls of more than 4 * 2^20 strings.

1. Under a capped grid (DPT_WAVE_GRID_BLOCKS = 1 and 3: 4 and 12 waves) the adversarial batches of test_gpu_bytelevel,
   test_gpu_pretok, test_gpu_decode and test_gpu_spans, in a fixed shuffled order, so that every wave walks at least
   eight strings and meets a refused or failed string, an empty one, a one-round and a multi-round one after each
   other in every order.
2. At the shipped grid, batches of 4 * 2^20 + 3 * 4099 + 5 short strings, a period of 4099 distinct ones repeated: the
   real second trip.  The reference is computed for one period and tiled.
3. hist_kernel's stride (more than 256 * 1024 strings).

Every call first asks dpt_debug_wave_grid for the grid its launches get, so a cap that is not in force cannot pass.
Outputs lie between canaries as in the tests the inputs come from."""
import numpy as np
import pytest

import bytelevel_ref as br
import decode_ref
import matrix_corpus as mc
import pretok_ref as pr
import spans_ref
import split_harness
import test_gpu_bytelevel as t_bytelevel
import test_gpu_decode as t_decode
import test_gpu_pretok as t_pretok
import test_gpu_spans as t_spans

pytestmark = pytest.mark.gpu

KNOB = "DPT_WAVE_GRID_BLOCKS"
WAVES = 4                      # waves to a block in all ten kernels
CAPS = (1, 3)                  # 4 waves; 12, not a power of two
TRIPS = 8                      # trips every wave makes at least under a cap
REFUSED, EMPTY, ONE_ROUND, MULTI_ROUND = range(4)

P = 4099                                   # the period of the large batches: a prime, so a string meets many wave slots
N_BIG = WAVES * (1 << 20) + 3 * P + 5      # 4,206,606 strings: 12,302 of them on a second trip


def _cap_grid(monkeypatch, cap, n):
    from dptok import _lib
    monkeypatch.setenv(KNOB, str(cap))
    assert _lib.wave_grid(n, WAVES) == cap, "the grid cap is not in force"
    assert n >= TRIPS * WAVES * cap


def _shipped_grid(monkeypatch, n):
    from dptok import _lib
    monkeypatch.delenv(KNOB, raising=False)
    assert n > WAVES * (1 << 20) and _lib.wave_grid(n, WAVES) == 1 << 20


def _shuffled(items, seed):
    return [items[i] for i in np.random.default_rng(seed).permutation(len(items))]


def _assert_alternates(classes):
    """On both capped grids some wave goes from a string of every class to one of every other class."""
    classes = np.asarray(classes)
    assert set(classes.tolist()) == {REFUSED, EMPTY, ONE_ROUND, MULTI_ROUND}
    for cap in CAPS:
        step = WAVES * cap
        seen = set(zip(classes[:-step].tolist(), classes[step:].tolist()))
        missing = {(a, b) for a in range(4) for b in range(4) if a != b} - seen
        assert not missing, (cap, sorted(missing))


def _split_classes(strings, status):
    return [REFUSED if st else EMPTY if not s else ONE_ROUND if len(s) <= 64 else MULTI_ROUND for s, st in zip(strings, status)]


def _dev(a):
    """A host array on the device (uint64 as int64: the same bytes)."""
    import torch
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _csr_offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    return off


# ================================================================== 1. capped grids: many trips per wave

# ------------------------------------------------------------------ bytelevel

@pytest.fixture(scope="module")
def bytelevel_case():
    """The shuffled strings, and per separator set the splitter and bytelevel_ref's result."""
    from dptok import ByteLevelSplit
    strings = t_bytelevel.round_edge_strings() + t_bytelevel.malformed_strings()
    strings = _shuffled(strings + [b""] * (len(strings) // 10), seed=101)
    sets = {"bloom": br.BLOOM_SEPARATORS, "other": t_bytelevel.OTHER_SEPARATORS}
    return strings, {k: (ByteLevelSplit(list(v), device=0), br.split(br.build_table(v), strings)) for k, v in sets.items()}


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("seps", ["bloom", "other"])
def test_bytelevel_capped(seps, cap, bytelevel_case, monkeypatch):
    strings, by_set = bytelevel_case
    splitter, want = by_set[seps]
    _assert_alternates(_split_classes(strings, want[0]))
    assert int((want[0] != 0).sum()) > 150
    _cap_grid(monkeypatch, cap, len(strings))
    kw = {} if cap == 1 else {"pad": 1, "off0": 0, "out0": 0}
    split_harness.check(splitter, lambda strs: want, strings, **kw)


# ------------------------------------------------------------------ pretok

@pytest.fixture(scope="module")
def pretok_case():
    """The shuffled strings, and per table (both hold the special-token literals) the Pretok and pretok_ref's result."""
    strings = t_pretok.edge_length_strings() + t_pretok.malformed_and_refused_strings() + t_pretok.SPACES
    strings = _shuffled(strings + [b""] * (len(strings) // 10), seed=102)
    pairs = {"runs_ok": t_pretok._pair(), "no_runs": t_pretok._pair(runs_ok=False)}
    assert all(len(table.literals) == 3 for _, table in pairs.values())
    return strings, {k: (pretok, pr.presplit(table, strings)) for k, (pretok, table) in pairs.items()}


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("which", ["runs_ok", "no_runs"])
def test_pretok_capped(which, cap, pretok_case, monkeypatch):
    strings, by_table = pretok_case
    pretok, want = by_table[which]
    _assert_alternates(_split_classes(strings, want[0]))
    n_refused = {k: int((w[0] != 0).sum()) for k, (_, w) in by_table.items()}
    assert 150 < n_refused["runs_ok"] < n_refused["no_runs"] < len(strings) - 100   # "  " is refused without runs_ok
    _cap_grid(monkeypatch, cap, len(strings))
    kw = {} if cap == 1 else {"pad": 1, "off0": 0, "out0": 0}
    split_harness.check(pretok, lambda strs: want, strings, **kw)


# ------------------------------------------------------------------ decode sizes / decode / roundtrip

S_OUT, S_ST, S_FD, S_LEN = t_decode.S_OUT, t_decode.S_ST, t_decode.S_FD, t_decode.S_LEN
OUT_START = t_decode.OUT_START


def _run_decode(detok, ids, id_off, status, text, offs, strip, ok=None):
    """dpt_decode_sizes, dpt_decode and dpt_roundtrip on device copies of a CSR batch, every output between guard
    zones, the decode at an odd address with out_off starting at OUT_START -> (out_len u64[n], out u8[], out_off
    i64[n+1] from 0, dec_status, rt, first_diff with S_FD where it was not written).  ``ok`` (bool[n], optional): the
    strings whose decoded length is specified; the others' ranges are sized by what the sizes pass said."""
    import torch
    n = len(id_off) - 1
    d_ids, d_io, d_text, d_offs = _dev(ids if len(ids) else np.zeros(1, np.int32)), _dev(id_off), _dev(text), _dev(offs)
    d_st = None if status is None else _dev(status)
    st_ptr = 0 if d_st is None else d_st.data_ptr()
    lens = mc.Guarded(torch, n, torch.int64, S_LEN)
    dst, rt, fd = (mc.Guarded(torch, n, torch.int32, s) for s in (S_ST, S_ST, S_FD))
    for g in (lens, dst, rt, fd):
        g.fill()
    detok.sizes_device(d_ids.data_ptr(), d_io.data_ptr(), n, lens.ptr(), status_ptr=st_ptr, strip_space=strip)
    torch.cuda.synchronize()
    h_len, fine = lens.host()
    assert fine, "guard zone of out_len overwritten"
    h_len = h_len.copy()
    out_off = np.zeros(n + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(h_len)
    total = int(out_off[-1])
    assert 0 <= int(h_len.min()) and total < 1 << 31
    d_oo = _dev(out_off + OUT_START)
    out = mc.Guarded(torch, total + 1, torch.uint8, S_OUT)
    out.fill()
    detok.decode_device(d_ids.data_ptr(), d_io.data_ptr(), n, out.ptr() + 1, d_oo.data_ptr(), dst.ptr(), status_ptr=st_ptr,
                        strip_space=strip)
    detok.roundtrip_device(d_ids.data_ptr(), d_io.data_ptr(), d_text.data_ptr(), d_offs.data_ptr(), n, rt.ptr(),
                           first_diff_ptr=fd.ptr(), status_ptr=st_ptr, strip_space=strip)
    torch.cuda.synchronize()
    res = {}
    for k, g in (("lens", lens), ("out", out), ("dst", dst), ("rt", rt), ("fd", fd)):
        res[k], fine = g.host()
        assert fine, "guard zone of %s overwritten" % k
    assert np.array_equal(res["lens"], h_len), "out_len changed after the sizes pass"
    assert res["out"][0] == S_OUT
    return h_len.view(np.uint64), res["out"][1:], out_off, res["dst"], res["rt"], res["fd"]


def _assert_first_diff(fd, wrt, wfd):
    assert np.array_equal(np.where(wrt == 5, fd.view(np.uint32).astype(np.int64), -1), wfd), np.nonzero((wrt == 5) & (fd != wfd))[0][:10]
    assert (fd[wrt != 5] == S_FD).all(), "first_diff written where the verdict is not 5"


@pytest.fixture(scope="module")
def decode_case():
    """The batch behind test_gpu_decode's edge_batch, string by string, plus strings with a failed status, strings
    with an id outside the table and more empty ones, shuffled; decode_ref's results with and without the strip."""
    e = t_decode.build_edge_batch()
    by_id, lists, texts = e["by_id"], e["lists"], e["texts"]
    assert min(by_id) == 0 and max(by_id) == 32001 and len(by_id) == 32002
    recs = [(ml, tx, 0) for ml, tx in zip(lists, texts)]
    for k in range(12):                                                      # failed: no ids, nothing but the status
        recs += [([], texts[3 * k], 1), ([], b"", 2), ([], texts[200 + k], 3)]
    recs += [([], b"", 0)] * 20
    outside = (-1, 32002, 40000, 2 ** 31 - 1, -2 ** 31)
    n_out = 0
    for src in (2, 30, 66, 100, 129, 250, 399, 400):                         # an id no table entry stands for: status 4
        ml = lists[src]
        for at in sorted({0, len(ml) // 2, 63, 64, len(ml) - 1}):
            if at < len(ml):
                recs.append((ml[:at] + [outside[n_out % len(outside)]] + ml[at + 1:], texts[src], 0))
                n_out += 1
    assert n_out >= 30
    recs = _shuffled(recs, seed=103)
    ids = np.array([i for ml, _, _ in recs for i in ml], dtype=np.int64).astype(np.int32)
    id_off = _csr_offsets([len(ml) for ml, _, _ in recs])
    text = np.frombuffer(b"".join(tx for _, tx, _ in recs) + b"\0", dtype=np.uint8)
    offs = _csr_offsets([len(tx) for _, tx, _ in recs])
    status = np.array([st for _, _, st in recs], dtype=np.int32)
    want = {strip: (decode_ref.expected_decode(by_id, ids, id_off, status, strip=strip),
                    decode_ref.expected_roundtrip(by_id, text, offs, ids, id_off, status, strip=strip)) for strip in (True, False)}
    for dec, rt in want.values():
        for arr in dec + rt:
            arr.setflags(write=False)
    ok = want[True][0][3]
    n_tok, n_bytes = np.diff(id_off.astype(np.int64)), np.diff(want[True][0][1].astype(np.int64))
    classes = np.where((status != 0) | ~ok, REFUSED, np.where(n_tok == 0, EMPTY, np.where((n_tok <= 64) & (n_bytes <= 64), ONE_ROUND, MULTI_ROUND)))
    _assert_alternates(classes)
    assert int((~ok).sum()) == n_out and {1, 2, 3} <= set(status.tolist())
    wrt, wfd = want[True][1]
    assert {0, 1, 2, 3, 4, 5} == set(wrt.tolist())
    assert {0, 62, 63, 64, 65, 302, 4000} <= set(wfd[wrt == 5].tolist())     # early, late, and by length
    # a string with an id outside the table, then a good one, on one wave of either grid
    for cap in CAPS:
        step = WAVES * cap
        assert ((~ok[:-step]) & (classes[step:] == MULTI_ROUND)).any() and ((~ok[:-step]) & (classes[step:] == ONE_ROUND)).any()
    return {"detok": e["detok"], "ids": ids, "id_off": id_off, "text": text, "offs": offs, "status": status, "want": want}


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("strip", [True, False])
def test_decode_capped(strip, cap, decode_case, monkeypatch):
    c = decode_case
    (wraw, woff, wst, ok), (wrt, wfd) = c["want"][strip]
    n = len(wst)
    _cap_grid(monkeypatch, cap, n)
    lens, out, out_off, dst, rt, fd = _run_decode(c["detok"], c["ids"], c["id_off"], c["status"], c["text"], c["offs"], strip)
    wlen = np.diff(woff)
    assert np.array_equal(lens[ok], wlen[ok]), np.nonzero(ok & (lens != wlen))[0][:10]
    assert np.array_equal(dst, wst), np.nonzero(dst != wst)[0][:10]
    wo = woff.astype(np.int64)
    for s in np.flatnonzero(ok):                                             # (the bytes of a status-4 string are unspecified)
        assert np.array_equal(out[out_off[s]:out_off[s + 1]], wraw[wo[s]:wo[s + 1]]), s
    assert np.array_equal(rt, wrt), (np.nonzero(rt != wrt)[0][:10], rt[rt != wrt][:10], wrt[rt != wrt][:10])
    _assert_first_diff(fd, wrt, wfd)


# ------------------------------------------------------------------ spans, the three forms

S_END, S_WORD, S_SS = t_spans.S_END, t_spans.S_WORD, t_spans.S_SS


def _run_spans(enc, form, text, offs, cut, ids, id_off, status):
    """dpt_token_spans on device copies of a batch, every output between guard zones -> (tok_end u32[n_tok], tok_word,
    span_status)."""
    import torch
    n, n_tok = len(offs) - 1, len(ids)
    d_text, d_offs, d_ids, d_io, d_st = _dev(text), _dev(offs), _dev(ids if n_tok else np.zeros(1, np.int32)), _dev(id_off), _dev(status)
    d_cut = None if cut is None else _dev(cut)
    end, word, ss = (mc.Guarded(torch, n_tok, torch.int32, S_END), mc.Guarded(torch, n_tok, torch.int32, S_WORD),
                     mc.Guarded(torch, n, torch.int32, S_SS))
    for g in (end, word, ss):
        g.fill()
    enc.spans_device(d_text.data_ptr(), int(offs[-1] - offs[0]), d_offs.data_ptr(), n, d_ids.data_ptr(), d_io.data_ptr(), d_st.data_ptr(),
                     end.ptr(), ss.ptr(), tok_word_ptr=word.ptr(), cut_ptr=0 if d_cut is None else d_cut.data_ptr(), mode=form)
    torch.cuda.synchronize()
    res = []
    for k, g in (("tok_end", end), ("tok_word", word), ("span_status", ss)):
        got, fine = g.host()
        assert fine, "guard zone of %s overwritten" % k
        res.append(got)
    return res[0].view(np.uint32), res[1].view(np.uint32), res[2]


def _span_records(t2i, form, text, offs, cut, ids, id_off, st):
    """A batch string by string: (text bytes, cut bytes, ids, status, spans_ref's tok_end, tok_word, False)."""
    rend, rword, rss = spans_ref.expected(t2i, form, text, offs, cut, ids, id_off, st)
    assert np.array_equal(rss, st)
    o, io = offs.astype(np.int64), id_off.astype(np.int64) - int(id_off[0])
    raw = np.asarray(text, dtype=np.uint8).tobytes()
    cutb = None if cut is None else np.asarray(cut, dtype=np.uint8).tobytes()
    return [(raw[o[s]:o[s + 1]], None if cutb is None else cutb[o[s]:o[s + 1]], ids[io[s]:io[s + 1]].tolist(), int(st[s]),
             rend[io[s]:io[s + 1]], rword[io[s]:io[s + 1]], False) for s in range(len(st))]


def _with_untiled(recs, t2i, seed):
    """``recs`` plus strings with a failed status, empty ones and copies of good strings whose ids do not tile them
    (the last flag set: status 4, entries unspecified), shuffled."""
    by_len = {}
    for t, i in t2i.items():
        by_len.setdefault(len(t.encode("utf-8")), i)
    outside = max(t2i.values()) + 1000
    good = [r for r in recs if r[3] == 0 and len(r[2]) >= 2]
    small = [r for r in good if len(r[2]) <= 10][:6]
    big = [r for r in good if len(r[2]) >= 130][:6]
    assert len(small) == 6 and len(big) == 6
    inv = spans_ref.invert(t2i)
    none = np.zeros(0, np.uint32)
    extra = []
    for k, (tx, cut, ml, _, _, _, _) in enumerate(small + big):
        n = len(inv[ml[len(ml) // 2]].encode("utf-8"))
        other = by_len[n + 1 if n + 1 in by_len else n - 1]
        for bad in (ml[:-1],                                                 # ends before the string does
                    ml + ml[-1:],                                            # ... after it
                    [outside] + ml[1:], ml[:-1] + [outside], ml[:len(ml) // 2] + [-7] + ml[len(ml) // 2 + 1:],   # no such token
                    ml[:len(ml) // 2] + [other] + ml[len(ml) // 2 + 1:]):    # a token one byte longer or shorter
            z = np.zeros(len(bad), np.uint32)
            extra.append((tx, cut, bad, 0, z, z, True))
        if len(ml) > 70:
            bad = ml[:64] + [outside] + ml[65:]                              # ... in the second round of ids
            extra.append((tx, cut, bad, 0, np.zeros(len(bad), np.uint32), np.zeros(len(bad), np.uint32), True))
        extra += [(tx, cut, [], 1, none, none, False), (b"", None if cut is None else b"", [], 2, none, none, False),
                  (tx, cut, [], 3, none, none, False)] + [(b"", None if cut is None else b"", [], 0, none, none, False)] * 4
    return _shuffled(recs + extra, seed)


def _span_case(recs):
    """Records -> the flat batch, the expected arrays and the entries that are specified."""
    has_cut = recs[0][1] is not None
    case = {"text": np.frombuffer(b"".join(r[0] for r in recs) + b"\0", dtype=np.uint8),
            "cut": np.frombuffer(b"".join(r[1] for r in recs) + b"\0", dtype=np.uint8) if has_cut else None,
            "offs": _csr_offsets([len(r[0]) for r in recs]),
            "ids": np.array([i for r in recs for i in r[2]], dtype=np.int64).astype(np.int32),
            "id_off": _csr_offsets([len(r[2]) for r in recs]),
            "status": np.array([r[3] for r in recs], dtype=np.int32),
            "end": np.concatenate([r[4] for r in recs]).astype(np.uint32), "word": np.concatenate([r[5] for r in recs]).astype(np.uint32),
            "ss": np.array([4 if r[6] else r[3] for r in recs], dtype=np.int32),
            "keep": np.concatenate([np.full(len(r[2]), not r[6]) for r in recs])}
    n_tok = np.array([len(r[2]) for r in recs])
    n_bytes = np.array([len(r[0]) for r in recs])
    classes = np.where(case["ss"] != 0, REFUSED, np.where(n_bytes == 0, EMPTY, np.where((n_tok <= 64) & (n_bytes <= 64), ONE_ROUND, MULTI_ROUND)))
    _assert_alternates(classes)
    untiled = np.array([r[6] for r in recs])
    for cap in CAPS:                                                         # the bad / break exits, then a good string on the same wave
        step = WAVES * cap
        assert (untiled[:-step] & (classes[step:] == MULTI_ROUND)).any() and (untiled[:-step] & (classes[step:] == ONE_ROUND)).any()
    assert {1, 2, 3, 4} <= set(case["ss"].tolist()) and int(untiled.sum()) >= 70
    for a in case.values():
        if a is not None:
            a.setflags(write=False)
    return case


@pytest.fixture(scope="module")
def span_cases():
    """form -> (Encoder, the shuffled batch): RAW from test_gpu_spans' edge_batch, PRESPLIT and ATOMS from the matrix
    corpus, whose ids come from the engine's encode as in the tests these batches are from."""
    from dptok import Encoder, Vocab
    e = t_spans.build_edge_batch()
    ids, id_off, st = e["got"][:3]
    out = {"raw": (e["enc"], _span_case(_with_untiled(_span_records(e["t2i"], "raw", e["text"], e["offs"], None, ids, id_off, st), e["t2i"], 104)))}
    t2i = mc.vocabularies()["base"]
    enc = Encoder(Vocab(t2i, 0))
    for k, form in enumerate(("presplit", "atoms")):
        text, offs, cut = mc.form(form)
        ids, id_off, st, _ = enc.encode_csr(text, offs, mode=form, cut_mask=cut)
        assert (st != 0).any() and (st == 0).sum() > 200
        out[form] = (enc, _span_case(_with_untiled(_span_records(t2i, form, text, offs, cut, ids, id_off, st), t2i, 105 + k)))
    return out


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("form", mc.FORMS)
def test_spans_capped(form, cap, span_cases, monkeypatch):
    enc, c = span_cases[form]
    _cap_grid(monkeypatch, cap, len(c["ss"]))
    end, word, ss = _run_spans(enc, form, c["text"], c["offs"], c["cut"], c["ids"], c["id_off"], c["status"])
    assert np.array_equal(ss, c["ss"]), (np.nonzero(ss != c["ss"])[0][:10], ss[ss != c["ss"]][:10])
    keep = c["keep"]                                                         # (a status-4 string's entries are unspecified)
    assert np.array_equal(end[keep], c["end"][keep]), np.nonzero(keep & (end != c["end"]))[0][:10]
    assert np.array_equal(word[keep], c["word"][keep]), np.nonzero(keep & (word != c["word"]))[0][:10]


# ================================================================== 2. the shipped grid: the real second trip

POOL = ("the quick (brown) fox, jumps. over | the lazy dog! " * 8).encode()
TAIL = "é中😀".encode()


def period_strings(seed, whole_tails=False):
    """P short strings: slices of 0..8 bytes of a punctuated ASCII pool; every 97th has 66..199 bytes; every 11th ends
    in a prefix of "é中😀" cut at any byte (``whole_tails``: at a character's end only)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(P):
        length = int(rng.integers(66, 200)) if i % 97 == 0 else int(rng.integers(0, 9))
        at = int(rng.integers(0, len(POOL) - 200))
        s = POOL[at:at + length]
        cut = int(rng.integers(1, len(TAIL) + 1))
        if i % 11 == 1:   # (not 0: string 4 * 2^20 + 7 of a batch, which test_decode_second_trip edits, is 94 * 11 of its period)
            s += TAIL[:max(c for c in (2, 5, 9) if c <= max(cut, 2))] if whole_tails else TAIL[:cut]
        out.append(s)
    return out


def _assert_period(lens, failed):
    """The conditions on a period: its strings' byte lengths and which of them are refused or failed."""
    lens, failed = np.asarray(lens), np.asarray(failed, dtype=bool)
    assert len(lens) == len(failed) == P
    assert failed.mean() >= 0.05 and (lens == 0).mean() >= 0.05 and (lens > 64).mean() >= 0.01 and (lens > 128).any()
    assert lens.mean() <= 8


def _tile(a, per_string=None, n=N_BIG):
    """One period's array (or bytes) repeated to n strings: one entry per string, or per_string[s] entries of string s."""
    full, rem = divmod(n, P)
    if per_string is None:
        return np.concatenate([np.tile(a, full), a[:rem]])
    cut = int(np.sum(per_string[:rem]))
    assert len(a) == int(np.sum(per_string))
    if isinstance(a, bytes):
        return a * full + a[:cut]
    return np.concatenate([np.tile(a, full), a[:cut]])


def _second_trip_split(split, strings, want):
    """A splitter's sizes + write over N_BIG strings against one period's reference, tiled."""
    st_p, ln_p, text2_p, cut_p = want
    lens_p = np.array([len(s) for s in strings], dtype=np.int64)
    _assert_period(lens_p, st_p != 0)
    pre, out_len, text2, cut = split_harness.run_packed(split, _tile(b"".join(strings), lens_p), _tile(lens_p))
    assert len(pre) == N_BIG
    assert np.array_equal(pre, _tile(st_p)), np.nonzero(pre != _tile(st_p))[0][:10]
    assert np.array_equal(out_len, _tile(ln_p)), np.nonzero(out_len != _tile(ln_p))[0][:10]   # (so the offsets are equal too)
    ln_i = ln_p.astype(np.int64)
    for what, got, w in (("text", text2, text2_p), ("cut", cut, cut_p)):
        w_all = np.frombuffer(_tile(w, ln_i), dtype=np.uint8)
        g_all = np.frombuffer(got, dtype=np.uint8)
        assert len(g_all) == len(w_all) and np.array_equal(g_all, w_all), (what, np.nonzero(g_all != w_all)[0][:10])


def test_bytelevel_second_trip(monkeypatch):
    from dptok import ByteLevelSplit
    strings = period_strings(seed=201)
    _shipped_grid(monkeypatch, N_BIG)
    _second_trip_split(ByteLevelSplit(device=0), strings, br.split(t_bytelevel.TABLE, strings))


def test_pretok_second_trip(monkeypatch):
    pretok, table = t_pretok._pair()
    strings = period_strings(seed=202)
    _shipped_grid(monkeypatch, N_BIG)
    _second_trip_split(pretok, strings, pr.presplit(table, strings))


@pytest.fixture(scope="module")
def oracle_period():
    """One period encoded by the C oracle (RAW, the llama-shaped vocabulary: a string with a character outside it or a
    leading space fails with status 1, an empty one has status 2), and the same tiled to N_BIG strings on the host."""
    from dptok import synth
    from oracle import oracle
    t2i = synth.llama_shaped_vocab()
    strings = period_strings(seed=215, whole_tails=True)   # (a seed under which the strings test_decode_second_trip edits encode)
    lens_p = np.array([len(s) for s in strings], dtype=np.int64)
    text_p = np.frombuffer(b"".join(strings) + b"\0", dtype=np.uint8)
    offs_p = _csr_offsets(lens_p)
    ids_p, io_p, st_p, _ = oracle.OracleVocab(t2i).encode_csr(text_p, offs_p)
    ids_p, st_p = ids_p.copy(), st_p.copy()
    cnt_p = np.diff(io_p.astype(np.int64))
    _assert_period(lens_p, st_p != 0)
    assert set(st_p.tolist()) == {0, 1, 2} and (st_p[lens_p == 0] == 2).all() and not cnt_p[st_p != 0].any()
    big = {"text": np.frombuffer(_tile(text_p[:-1].tobytes(), lens_p) + b"\0", dtype=np.uint8), "offs": _csr_offsets(_tile(lens_p)),
           "ids": _tile(ids_p, cnt_p), "id_off": _csr_offsets(_tile(cnt_p)), "status": _tile(st_p)}
    assert len(big["status"]) == N_BIG and len(big["ids"]) == int(big["id_off"][-1])
    return {"t2i": t2i, "text": text_p, "offs": offs_p, "ids": ids_p, "id_off": io_p, "status": st_p, "counts": cnt_p, "lens": lens_p,
            "big": big}


def test_spans_second_trip(oracle_period, monkeypatch):
    from dptok import Encoder, Vocab
    p, big = oracle_period, oracle_period["big"]
    rend, rword, rss = spans_ref.expected(p["t2i"], "raw", p["text"], p["offs"], None, p["ids"], p["id_off"], p["status"])
    _shipped_grid(monkeypatch, N_BIG)
    end, word, ss = _run_spans(Encoder(Vocab(p["t2i"], 0)), "raw", big["text"], big["offs"], None, big["ids"], big["id_off"], big["status"])
    assert np.array_equal(ss, _tile(rss)), np.nonzero(ss != _tile(rss))[0][:10]
    w = _tile(rend, p["counts"])
    assert np.array_equal(end, w), np.nonzero(end != w)[0][:10]
    w = _tile(rword, p["counts"])
    assert np.array_equal(word, w), np.nonzero(word != w)[0][:10]


def test_decode_second_trip(oracle_period, monkeypatch):
    from dptok import Detok
    p, big = oracle_period, oracle_period["big"]
    by_id = decode_ref.pieces_by_id(decode_ref.pairs_of(p["t2i"]), "sp")
    wraw, woff, wst, ok = decode_ref.expected_decode(by_id, p["ids"], p["id_off"], p["status"], strip=True)
    wrt, wfd = decode_ref.expected_roundtrip(by_id, p["text"], p["offs"], p["ids"], p["id_off"], p["status"], strip=True)
    wlen = np.diff(woff.astype(np.int64))
    assert ok.all() and np.array_equal(wrt, p["status"]) and np.array_equal(wlen[wst == 0], p["lens"][wst == 0])   # the true text: all equal
    detok = Detok(p["t2i"], "sp")
    _shipped_grid(monkeypatch, N_BIG)
    args = (detok, big["ids"], big["id_off"], big["status"])
    lens, out, out_off, dst, rt, fd = _run_decode(*args, big["text"], big["offs"], True)
    assert np.array_equal(lens, _tile(wlen).view(np.uint64)), np.nonzero(lens != _tile(wlen).view(np.uint64))[0][:10]
    assert np.array_equal(dst, _tile(wst)), np.nonzero(dst != _tile(wst))[0][:10]
    w = _tile(wraw, wlen)
    assert len(out) == len(w) and np.array_equal(out, w), np.nonzero(out != w)[0][:10]
    assert np.array_equal(rt, _tile(wrt)), np.nonzero(rt != _tile(wrt))[0][:10]
    assert (fd == S_FD).all()
    # one byte changed in a string of the first trip, of the second trip and in the last string
    victims = [5, WAVES * (1 << 20) + 7, N_BIG - 1]
    text2 = big["text"].copy()
    o = big["offs"].astype(np.int64)
    want_rt, want_fd = _tile(wrt).copy(), np.full(N_BIG, -1, dtype=np.int64)
    for k, s in enumerate(victims):
        n = int(o[s + 1] - o[s])
        assert big["status"][s] == 0 and n >= 2, (s, n)
        at = (0, n - 1, n // 2)[k]
        text2[o[s] + at] ^= 1
        want_rt[s], want_fd[s] = 5, at
    _, _, _, _, rt, fd = _run_decode(*args, text2, big["offs"], True)
    assert np.flatnonzero(rt == 5).tolist() == victims
    assert np.array_equal(rt, want_rt)
    _assert_first_diff(fd, want_rt, want_fd)


# ================================================================== 3. hist_kernel's stride

@pytest.mark.parametrize("n", [256 * 1024 + 1, 3 * 256 * 1024 + 77])
def test_histogram_stride(n):
    """dpt_token_histogram runs at most 256 blocks of 1024 threads (HIST_THREADS, csrc/dpt_kernels.hip), a string to a
    thread: from 256 * 1024 + 1 strings on a thread takes a second one."""
    import torch
    from dptok import _lib
    rng = np.random.default_rng(n)
    nb = 16
    counts = rng.integers(0, 40, size=n)
    status = rng.choice(np.array([0, 0, 0, 0, 1, 2, 3, 4], dtype=np.int32), size=n)
    counts[status != 0] = 0
    d_io, d_st = _dev(_csr_offsets(counts)), _dev(status)
    hist = mc.Guarded(torch, nb + 8, torch.int64, S_LEN)
    hist.fill()
    hist.view.zero_()
    _lib.check(_lib.lib().dpt_token_histogram(d_io.data_ptr(), d_st.data_ptr(), n, hist.ptr(), nb, 0), "dpt_token_histogram")
    torch.cuda.synchronize()
    h, fine = hist.host()
    assert fine, "a store outside the histogram"
    assert np.array_equal(h[:nb], np.bincount(np.minimum(counts, nb - 1), minlength=nb))
    assert h[nb] == counts.sum() and h[nb + 1] == n
    assert np.array_equal(h[nb + 2:nb + 7], np.bincount(status, minlength=5)) and h[nb + 7] == 0
