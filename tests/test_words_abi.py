"""CPU checks of the word-compare calls' boundary: the symbols, dpt_word_side's layout, every argument error (before
any device work) and the empty call (no GPU needed)."""
import ctypes

from conftest import PKG  # noqa: F401  (puts the package on sys.path)

SEL = ("sel_str", "sel_word", "sel_begin", "sel_end", "sel_a_first", "sel_a_count", "sel_b_first", "sel_b_count")


def _side(_lib, null=None, tok_end=80):
    """A side of non-null placeholders, never dereferenced when an argument is rejected; ``null``: the member to leave
    null."""
    v = {"off": 16, "counts": None, "status": None, "tok_word": 48, "tok_end": tok_end}
    if null:
        v[null] = None
    return _lib.WordSide(v["off"], v["counts"], v["status"], v["tok_word"], v["tok_end"])


def _sizes(L, _lib, a="ok", b="ok", n_str=1, flags=1, n_words=96, n_sel=112, wc_status=128):
    sa = None if a is None else ctypes.byref(_side(_lib, None if a == "ok" else a))
    sb = None if b is None else ctypes.byref(_side(_lib, None if b == "ok" else b))
    return L.dpt_word_compare_sizes(sa, sb, n_str, flags, n_words or None, n_sel or None, None, None, wc_status or None, None)


def _write(L, _lib, a="ok", b="ok", n_str=1, flags=1, wc_status=128, a_tok_end=80, word=(144, 160, 176), sel_off=192, **sel):
    sa = None if a is None else ctypes.byref(_side(_lib, None if a == "ok" else a, tok_end=a_tok_end))
    sb = None if b is None else ctypes.byref(_side(_lib, None if b == "ok" else b))
    ptrs = [sel.get(k, 208 + 16 * i) or None for i, k in enumerate(SEL)]
    return L.dpt_word_compare_write(sa, sb, n_str, flags, *(w or None for w in word), sel_off or None, *ptrs, wc_status or None, None)


def test_library_exports_the_calls():
    from dptok import _lib
    L = _lib.lib()
    assert _lib.has_words()
    for name in ("dpt_word_compare_sizes", "dpt_word_compare_write"):
        assert hasattr(L, name) and name in _lib.CALLS and name in _lib.EXPORTED and name in _lib.OPTIONAL_WORDS
    assert set(_lib.WORDS_CALLS) == _lib.OPTIONAL_WORDS
    assert not (_lib.OPTIONAL_WORDS & (_lib.OPTIONAL | _lib.OPTIONAL_LATER | _lib.OPTIONAL_PRETOK | _lib.OPTIONAL_BYTELEVEL | _lib.OPTIONAL_BPE))
    assert len(_lib.CALLS["dpt_word_compare_sizes"][1]) == 10 and len(_lib.CALLS["dpt_word_compare_write"][1]) == 18
    assert L.dpt_abi_version() == 6
    assert (_lib.WORDS_LESS, _lib.WORDS_GREATER) == (1, 2)


def test_structure_layout():
    from dptok import _lib
    S = _lib.WordSide
    fields = ("off", "counts", "status", "tok_word", "tok_end")
    assert ctypes.sizeof(S) == 40 and [f for f, _ in S._fields_] == list(fields)
    assert [getattr(S, f).offset for f in fields] == [0, 8, 16, 24, 32]


def test_argument_errors_name_the_argument():
    from dptok import _lib
    L = _lib.lib()
    for call in (_sizes, _write):
        for n_str in (1, 0):   # every error is found with n_str == 0 too
            for kw, word in (({"a": None}, b"null a"), ({"b": None}, b"null b"), ({"a": "off"}, b"a->off"), ({"b": "off"}, b"b->off"),
                             ({"a": "tok_word"}, b"a->tok_word"), ({"b": "tok_word"}, b"b->tok_word"), ({"wc_status": 0}, b"wc_status"),
                             ({"flags": 0}, b"flags"), ({"flags": 4}, b"flags"), ({"flags": 7}, b"flags"), ({"flags": -1}, b"flags")):
                assert call(L, _lib, n_str=n_str, **kw) == -1 and word in L.dpt_last_error(), (call.__name__, kw)
        for n_str in (1 << 31, 1 << 40):
            assert call(L, _lib, n_str=n_str) == -1 and b"n_str" in L.dpt_last_error()
    for n_str in (1, 0):
        assert _sizes(L, _lib, n_str=n_str, n_words=0) == -1 and b"n_words" in L.dpt_last_error()
        assert _sizes(L, _lib, n_str=n_str, n_sel=0) == -1 and b"n_sel" in L.dpt_last_error()
        for word in ((0, 160, 176), (144, 0, 176), (144, 160, 0), (144, 0, 0), (0, 0, 176)):
            assert _write(L, _lib, n_str=n_str, word=word) == -1 and b"word_off" in L.dpt_last_error(), word
        for k in SEL:                                                        # one sel_* array and no sel_off
            assert _write(L, _lib, n_str=n_str, sel_off=0, **{x: 0 for x in SEL if x != k}) == -1 and b"sel_off" in L.dpt_last_error(), k
        for k in ("sel_begin", "sel_end"):                                   # the byte spans without side a's tok_end
            others = {x: 0 for x in ("sel_begin", "sel_end") if x != k}
            assert _write(L, _lib, n_str=n_str, a_tok_end=None, **others) == -1 and b"tok_end" in L.dpt_last_error(), k


def test_empty_call_is_ok():
    from dptok import _lib
    L = _lib.lib()
    for flags in (1, 2, 3):
        assert _sizes(L, _lib, n_str=0, flags=flags) == 0
        assert _write(L, _lib, n_str=0, flags=flags) == 0
    assert _write(L, _lib, n_str=0, word=(0, 0, 0)) == 0
    assert _write(L, _lib, n_str=0, sel_off=0, **{x: 0 for x in SEL}) == 0
    assert _write(L, _lib, n_str=0, a_tok_end=None, sel_begin=0, sel_end=0) == 0
    assert _write(L, _lib, n_str=0, word=(0, 0, 0), sel_off=192, **{x: 0 for x in SEL}) == 0   # statuses only
