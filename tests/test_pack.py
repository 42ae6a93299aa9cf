"""dptok/pack.py on the CPU: every packer against a per-string plain-Python model (bytes concatenation,
no numpy), the empty-word rule against the loop ``Encoder.encode_presplit`` used to run, and the shape of
the one table the binding is made from (dptok/_lib.py CALLS against include/dpt.h)."""
import itertools
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT

from dptok import _lib, engine, pack  # noqa: E402

SURROGATE = "a\ud800b"        # a lone surrogate: "surrogatepass" keeps its three bytes
WS = "▁"                     # 3 bytes of UTF-8


def _model(strings, first):
    """Strings as words of pieces -> (text + NUL, offsets, cut mask + NUL): a piece's first byte is marked
    ``first`` when it opens a word, else 2."""
    text, cut, offs = b"", b"", [0]
    for words in strings:
        for pieces in words:
            for k, p in enumerate(pieces):
                e = p.encode("utf-8", "surrogatepass")
                text += e
                cut += bytes([first if k == 0 else 2] * min(len(e), 1)) + bytes(max(len(e) - 1, 0))
        offs.append(len(text))
    return text + b"\0", offs, cut + b"\0"


def _presplit_model(strings):
    kept = [ws[:ws.index("")] if "" in ws else ws for ws in strings]
    return _model([[[w] for w in ws] for ws in kept], 1) + ([len(ws) for ws in kept],
                                                           [ws.index("") if "" in ws else -1 for ws in strings])


def _same(got, want):
    for g, w, dtype in zip(got, want, (np.uint8, np.uint64, np.uint8)):
        assert isinstance(g, np.ndarray) and g.dtype == dtype and g.ndim == 1
        assert g.tolist() == list(w)


STRING_BATCHES = [[], [""], ["", ""], [SURROGATE], [WS], ["ab", "", WS + "é中😀", SURROGATE, "\0x"]]


@pytest.mark.parametrize("texts", STRING_BATCHES)
def test_pack_strings_and_vocab(texts):
    want = _model([[[t]] for t in texts], 3)[:2]
    _same(pack.pack_strings(texts), want)
    t2i = {t: 7 - 3 * i for i, t in enumerate(dict.fromkeys(texts))}
    blob, off, ids, n = pack.pack_vocab(t2i)
    _same((blob, off), _model([[[t]] for t in t2i], 3)[:2])
    assert ids.dtype == np.int32 and ids.tolist() == list(t2i.values()) and n == len(t2i)


ATOM_BATCHES = [[], [[]], [[], []], [[[WS]]], [[[SURROGATE, "x"]]],
                [[["a", "b"], [WS, "c"]], [], [["é"]], [[WS + "a"], ["中", SURROGATE, "😀"], ["z"]]]]


@pytest.mark.parametrize("strings", ATOM_BATCHES)
def test_pack_word_atoms(strings):
    _same(pack.pack_word_atoms(strings), _model(strings, 3))


NONEMPTY_LISTS = [[], [[WS]], [[WS, "a"], [SURROGATE], ["é", "中", "b"]], [["a"], ["b", WS + "é"], ["😀", "c", "d", "e"]]]


@pytest.mark.parametrize("lists", NONEMPTY_LISTS + [[[]], [[], [WS]], [[WS, "a"], [], [SURROGATE], ["é", "中", "b"]]])
def test_atoms_to_csr(lists):
    _same(pack.atoms_to_csr(lists), _model([[atoms] for atoms in lists], 3))


@pytest.mark.parametrize("lists", NONEMPTY_LISTS)
def test_atoms_to_csr_is_pack_word_atoms_of_one_word_strings(lists):
    assert all(lists)
    got, want = pack.atoms_to_csr(lists), pack.pack_word_atoms([[atoms] for atoms in lists])
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    if lists:
        assert len(got[0]) > 1 and got[1][-1] == len(got[0]) - 1     # real data went through


def test_empty_words_and_atoms():
    with pytest.raises(ValueError, match="empty word"):
        pack.pack_word_atoms([[[]]])
    with pytest.raises(ValueError, match="empty word"):
        pack.pack_word_atoms([[["a"]], [["b"], []]])
    text, offs, cut = pack.atoms_to_csr([[]])            # a zero-length string, no error
    assert text.tolist() == [0] and offs.tolist() == [0, 0] and cut.tolist() == [0]
    for f, arg in ((pack.pack_word_atoms, [[["a", ""]]]), (pack.atoms_to_csr, [["", "a"]])):
        with pytest.raises(ValueError, match="empty atom"):
            f(arg)


PRESPLIT_BATCHES = [[], [[]], [[], []], [[WS]], [[SURROGATE, "x"]],
                    [["", "a", "b"]], [["a", "", "b"]], [["a", "b", ""]], [[""]],
                    [[WS + "ab", "c"], [], ["", WS], ["é", "", "中"], ["x", WS + "😀", ""], ["z"]]]


@pytest.mark.parametrize("strings", PRESPLIT_BATCHES)
def test_pack_presplit_words(strings):
    got, want = pack.pack_presplit_words(strings), _presplit_model(strings)
    _same(got[:3], want[:3])
    assert (got[3], got[4]) == (want[3], want[4])


def _presplit_loop(ids, id_off, st, n_words, cut_at):
    """The loop of Encoder.encode_presplit before presplit_outcome, as it stood."""
    n_str = len(st)
    flat = ids.tolist()
    o = id_off.tolist()
    out = []
    for i in range(n_str):
        s = int(st[i])
        if cut_at[i] < 0 and n_words[i] == 0:
            out.append(([], _lib.STATUS_OK))           # no words: the reference's loop emits nothing
        elif cut_at[i] >= 0 and s in (_lib.STATUS_OK, _lib.STATUS_EMPTY_WORD):
            out.append(([], _lib.STATUS_EMPTY_WORD))   # the prefix tokenized (or was empty): IndexError
        else:
            out.append((flat[o[i]:o[i + 1]] if s == _lib.STATUS_OK else [], s))
    return out


@pytest.mark.parametrize("c_path", [True, False])
def test_presplit_outcome_is_the_old_loop(c_path, monkeypatch):
    cases = list(itertools.product(range(4), (-1, 0, 2), (0, 2)))
    st = np.array([c[0] for c in cases], dtype=np.int32)
    cut_at, n_words = [c[1] for c in cases], [c[2] for c in cases]
    counts = np.where(st == 0, 3, 0)                   # failed strings carry no ids (the kernels' rule)
    id_off = np.zeros(len(cases) + 1, dtype=np.uint64)
    id_off[1:] = np.cumsum(counts)
    ids = np.arange(100, 100 + int(id_off[-1]), dtype=np.int32)
    want = _presplit_loop(ids, id_off, st, n_words, cut_at)
    assert {w[1] for w in want} == {0, 1, 2, 3} and any(w[0] for w in want)
    if not c_path:
        monkeypatch.setattr(engine, "_pylists", None)
    fixed, none = pack.presplit_outcome(st, n_words, cut_at)
    assert fixed.dtype == np.int32 and none.dtype == bool and st.tolist() == [c[0] for c in cases]
    assert engine.csr_lists(ids, id_off, fixed, none=none, keep_failed=False) == want
    assert pack.csr_lists(ids, id_off, fixed, none=none, keep_failed=False,
                          pylists=pack._pylists if c_path else None) == want
    empty = pack.presplit_outcome(np.zeros(0, np.int32), [], [])
    assert len(empty[0]) == 0 and len(empty[1]) == 0


def test_calls_table_is_the_header():
    src = open(os.path.join(ROOT, "include", "dpt.h")).read()
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(dpt_\w+)\s*\(", src, re.M)))
    assert sorted(_lib.CALLS) == declared == _lib.EXPORTED
    binding = open(os.path.join(PKG, "dptok", "_lib.py")).read()
    for name in declared:                              # (a dict literal drops a repeated key silently)
        assert binding.count('"%s": (' % name) == 1, name
    assert _lib.OPTIONAL < set(_lib.CALLS)
    assert set(_lib.DECODE_CALLS) == _lib.OPTIONAL - {"dpt_debug_host_layout"}
    L = _lib.lib()
    for name, (restype, argtypes) in _lib.CALLS.items():
        assert isinstance(argtypes, list)
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes is argtypes, name
    assert _lib.has_decode()
