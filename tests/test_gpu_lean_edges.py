"""Both first-pass routes of plain raw calls, each on a route the test chose (tests/lean_routes.py): the lean kernel plus
the list-fed general kernel on a fresh context (asserted: words (0, 0, 0, 0) before, no probe and no skipped call after),
and the general RAW kernel alone on another.  Outputs identical and equal to the C oracle's, and the lean launch's
deferred count against the CPU model of the window tiling and the lean classifier (tests/lean_ref.py) -- a clean string
deferred because of what lies past its window changes no id, only that count.

* the edge matrix (tests/lean_edge_matrix.py): window lengths of every ``wlen % 4`` and 252..256, windows ended by a
  last space at 1..4, 127, 128, 252..255 or by a space at byte 256, long words, a poison at the first and last bytes
  of the first, second and third window, neighbours in the blob that start with a byte >= 0x80 or with 0x7F, all four
  alignments of a string's start -- on int16 and int32 staging (``tokenize_lean_kernel<1, .>`` and ``<2, .>``), the
  whole matrix through the device CSR entry, a subset through the padded and the host entries; every call holds at
  most five deferred strings, so the hint must stay on and the count is exact;
* the adversarial raw corpora of tests/test_gpu_parity.py (tests/raw_corpora.py) on both routes."""
import numpy as np
import pytest

import lean_edge_matrix as mx
import lean_ref
import raw_corpora
from lean_routes import model_sets, pinned_routes, want_deferred

pytestmark = pytest.mark.gpu

VOCABS = ("llama32k", "llama32k+40000")
ID_SHIFT = 40000   # (test_gpu_parity.py::test_staging_width_by_id_range: ids past 32767 are staged as int32)


@pytest.fixture(scope="module")
def setups(vocabs):
    """name -> (t2i, Vocab, OracleVocab, the two-byte token's bytes), with what the matrix assumes of the vocabulary"""
    from dptok import Vocab
    from oracle import oracle
    base = vocabs["llama32k"]
    out = {}
    for name, t2i in (("llama32k", base), ("llama32k+40000", {t: i + ID_SHIFT for t, i in base.items()})):
        nt, fnt = model_sets(t2i)
        # 0x7F: ASCII (the last byte the high-bit test lets through) and no token, alone or as a string's first atom
        assert "\x7f" not in t2i and "▁\x7f" not in t2i and 0x7F in nt and 0x7F in fnt
        used = set(range(0x61, 0x7B))
        assert (used | {0x20}).isdisjoint(nt) and used.isdisjoint(fnt)   # letters and inner spaces never defer a string
        assert 0x20 in fnt   # ... a string that starts with a space is deferred: '▁' + ' ' is no token
        assert (nt & mx.GENERIC_NO_TOKEN, fnt & mx.GENERIC_FIRST_NO_TOKEN) == (mx.GENERIC_NO_TOKEN, mx.GENERIC_FIRST_NO_TOKEN)
        tok2 = sorted(k for k in t2i if len(k) == 1 and len(k.encode()) == 2)[0]
        assert "é" not in t2i
        out[name] = (t2i, Vocab(t2i, 0), oracle.OracleVocab(t2i), tok2.encode())
    assert max(out["llama32k"][0].values()) <= 32767 < min(out["llama32k+40000"][0].values())
    return out


@pytest.fixture(scope="module")
def base_strings():
    bs = mx.bases()
    mx.check_bases(bs)   # the window lengths named beside each base string are the model's
    first = {w[0] for _, _, w, _ in bs if w}
    assert {w % 4 for w in first} == {0, 1, 2, 3} and {252, 253, 254, 255, 256, 1, 2, 3, 4, 127, 128} <= first
    assert sum(1 for _, _, w, _ in bs if len(w) >= 3 and w[1] == 256) >= 3
    return bs


def _run_calls(setup, calls, entry, counts_seen=None):
    t2i, vocab, orc, _ = setup
    nt, fnt = model_sets(t2i)
    first_words = None
    for name, strings in calls:
        want = len(lean_ref.predicted_deferred(strings, nt, fnt))
        # the packing's generic prediction holds for this vocabulary, and no wave can turn the hint off
        assert want == mx.n_deferred(strings) <= mx.MAX_DEFERRED, name
        assert len(strings) % mx.SLOTS == 0
        text, offs = mx.pack(strings)
        try:
            ref, words = pinned_routes(vocab, orc, text, offs, entry=entry, want=want, exact=True)
        except AssertionError as e:
            raise AssertionError("call %r (%s entry): %s" % (name, entry, e)) from e
        if counts_seen is not None:
            counts_seen.add(words[1])
        first_words = first_words or (name, words)
    return first_words


GROUPS = ("poison-e", "poison-t", "poison-d", "neighbours", "alignment")


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("vname", VOCABS)
def test_edge_matrix_device_entry(vname, group, setups, base_strings):
    """the whole matrix through dpt_encode, exact deferred counts, the hint still on after every call"""
    setup = setups[vname]
    tok2 = setup[3]
    seen = set()
    if group.startswith("poison-"):
        p = group[-1]   # (with 0x7F go the extras: the long word before the poison, 0x7F at a string's first byte)
        calls = mx.variant_calls(base_strings, tok2, select=lambda name, poison, place: poison == p, with_extras=p == "d")
        assert p != "d" or calls[-1][0] == "not-deferred"
    elif group == "neighbours":
        calls = mx.neighbour_calls(base_strings, tok2)
    else:
        calls = mx.alignment_calls(base_strings)
    first = _run_calls(setup, calls, "device", seen)
    if group.startswith("poison-"):
        assert {1, 2, 3, 4, 5} <= seen, seen      # list claims of one to five deferred strings
        assert any(c[0].endswith("-last") for c in calls)
    else:   # (the two bases that start with a space are deferred wherever they stand)
        assert {0, 5} <= seen if group == "neighbours" else seen == {2}, seen
    print("%s %s: %d calls, first %r -> debug_lean_words %r" % (vname, group, len(calls), first[0], first[1]))


@pytest.mark.parametrize("entry", ["padded", "host"])
@pytest.mark.parametrize("vname", VOCABS)
def test_edge_subset_other_entries(vname, entry, setups, base_strings):
    """dpt_encode_padded and dpt_encode_host through the lean pair: the strings deferred after one or two windows
    staged ids, the 256-byte windows, every ``wlen % 4``, the neighbours and the alignments of the first bases"""
    setup = setups[vname]
    calls = mx.variant_calls(base_strings, setup[3], select=mx.subset_select)
    assert any("w3" in c[0] for c in calls) and any("len256" in c[0] or "c256" in c[0] for c in calls)
    calls += mx.neighbour_calls(base_strings, setup[3])[::9] + mx.alignment_calls(base_strings)[1:3]
    seen = set()
    first = _run_calls(setup, calls, entry, seen)
    assert {0, 1, 2, 3, 4, 5} <= seen, seen
    print("%s %s: %d calls, first %r -> debug_lean_words %r" % (vname, entry, len(calls), first[0], first[1]))


def test_shifted_vocabulary_is_staged_as_int32(setups, base_strings):
    """(the cell check of the ``<2, .>`` kernels: the shifted vocabulary's ids do not fit int16 staging, its call takes
    the lean pair all the same, and the same call on the unshifted one gives the ids less the shift)"""
    strings = [b for _, b, w, lw in base_strings if w and not lw and not mx.is_deferred(b)][:16]
    text, offs = mx.pack(strings)
    res = {}
    for vname in VOCABS:
        t2i, vocab, orc, _ = setups[vname]
        ref, words = pinned_routes(vocab, orc, text, offs, want=0, exact=True)
        assert (ref[2] == 0).all()
        res[vname] = ref[0]
        print("%s: max id %d, debug_lean_words %r, vocab.stats %r" % (vname, int(ref[0].max()), words, vocab.stats))
    assert int(res["llama32k"].max()) <= 32767 < int(res["llama32k+40000"].min())
    assert np.array_equal(res["llama32k"] + ID_SHIFT, res["llama32k+40000"])


def test_window_ends_on_a_tie_heavy_vocabulary():
    """The matrix's clean strings over {a,b,c} on a tie-heavy capless vocabulary of tests/raw_corpora.py (the one with
    the most tokens of the first five): nearly every word has several shortest tokenizations, and the one selected
    depends on where the window's records say a word ends -- the end record prep_window_lean writes for each
    ``wlen % 4``, with the next string's first byte (no space) right behind the window.  Neighbours and alignments;
    the letters are all tokens, so the only strings deferred are the neighbours and the bases that start with a space."""
    from dptok import Vocab
    from oracle import oracle
    t2i = max((c[0] for c in raw_corpora.tie_heavy_cases(5, 1)), key=len)
    nt, fnt = model_sets(t2i)
    assert set(b"abc ").isdisjoint(nt) and set(b"abc").isdisjoint(fnt) and {0x20, 0x7F} <= fnt and 0x7F in nt
    bs = mx.bases(alphabet=b"abc")
    mx.check_bases(bs)
    setup = (t2i, Vocab(t2i, 0), oracle.OracleVocab(t2i), None)
    calls = mx.neighbour_calls(bs, None) + mx.alignment_calls(bs)
    seen = set()
    first = _run_calls(setup, calls, "device", seen)
    assert {0, 2, 5} <= seen, seen
    print("tie-heavy vocabulary of %d tokens: %d calls, first %r -> debug_lean_words %r" % (len(t2i), len(calls), first[0], first[1]))


# ---------------------------------------------------------------- the adversarial raw corpora, route pinned
def _partition_corpus(n):
    """test_work_partitions_vs_oracle's short ragged strings, 1 % of them with a non-ASCII character at a seeded place
    (as test_gpu_lean_pass.py::test_two_partitions_one_percent_non_ascii does): min(16, n / 4096) partitions"""
    parts = raw_corpora.work_partition_parts(n)
    rng = np.random.default_rng(14)
    for s in rng.choice(n, size=n // 100, replace=False):
        t = parts[int(s)]
        k = int(rng.integers(0, len(t) + 1))
        parts[int(s)] = t[:k] + mx.E + t[k:]
    return raw_corpora.pack_parts(parts)


CORPORA = ["a0-llama32k", "a0-toy1k", "walker-31", "walker-31-capless", "walker-32", "tie-heavy", "long-words",
           "mid-pass-raw", "partitions-8192", "partitions-65536"]


def _walker_runs(case):
    """The walker corpus.  Seed 31 ('▁' a token) is capless but for one thing: a string that starts with a space or
    with '\n' has the first atom '▁ ' / '▁\n' (pretokenize_raw marks the first character as it is), which
    is no token of that vocabulary -- its first window is not capless, the lean kernel has no capped recurrence, and
    the string must be deferred.  So the whole corpus goes under the bound with the model's count (asserted to be
    exactly those strings), and "-capless" is the corpus without them: there nothing at all may be deferred."""
    t2i, text, offs = raw_corpora.walker_case(int(case.split("-")[1]))
    if case.startswith("walker-31"):
        strings = lean_ref.split_blob(text, offs)
        nt, fnt = model_sets(t2i)
        marked = {i for i, b in enumerate(strings) if b[:1] in (b" ", b"\n")}
        want = lean_ref.predicted_deferred(strings, nt, fnt)
        # (but ' ' + a 300-byte word: no window at all, status 3 before anything is classified)
        assert want <= marked and len(want) > 100 and all(not lean_ref.raw_windows(strings[i])[0] for i in marked - want)
        if case.endswith("-capless"):
            text, offs = raw_corpora.pack_parts([b for i, b in enumerate(strings) if i not in marked])
    return [(t2i, text, offs)]


@pytest.mark.parametrize("case", CORPORA)
def test_raw_corpora_both_routes(case, vocabs):
    """Each corpus on both routes through dpt_encode.  Deferred counts: exactly the model's while the hint stays on, at
    least one and at most the model's once a wave turned it off mid-call (the A0 corpus's control bytes defer many
    strings).  The printable capless corpora -- tie-heavy on its own {a,b,c} vocabularies, the printable long words,
    the walker corpus with '▁' a token less its strings that start with a space or '\n' (_walker_runs) -- must
    defer nothing at all.  The walker corpus of seed 32 has no '▁' token: the model's rule (a space that is no
    string start is the atom '▁') covers it, every window with an inner space is deferred there, and the same
    bound applies."""
    from dptok import Vocab
    from oracle import oracle
    zero = False
    if case.startswith("a0-"):
        runs = [(vocabs[case[3:]],) + tuple(raw_corpora.a0_corpus())]
    elif case.startswith("walker-"):
        runs = _walker_runs(case)
        zero = case.endswith("-capless")
    elif case == "tie-heavy":
        runs = list(raw_corpora.tie_heavy_cases(5, 400))
        zero = True
    elif case == "long-words":
        runs = [(vocabs["llama32k"],) + tuple(raw_corpora.long_words_corpus())]
        zero = True
    elif case == "mid-pass-raw":
        runs = [(vocabs["llama32k"],) + tuple(raw_corpora.mid_pass_raw(raw_corpora.mid_pass_strings()))]
    else:
        runs = [(vocabs["llama32k"],) + tuple(_partition_corpus(int(case[11:])))]
    for t2i, text, offs in runs:
        want = want_deferred(t2i, text, offs)
        if zero:
            assert want == 0, want
        else:
            assert want > 0
        ref, words = pinned_routes(Vocab(t2i, 0), oracle.OracleVocab(t2i), text, offs, want=want)
        if zero:
            assert words[:2] == (0, 0), words
        print("%s: %d strings, model %d deferred -> debug_lean_words %r" % (case, len(offs) - 1, want, words))
