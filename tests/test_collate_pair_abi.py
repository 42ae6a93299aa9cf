"""CPU checks of dpt_collate_pair's boundary: the symbol, the two structures' layout, its argument errors (before
any device work) and the empty call (no GPU needed)."""
import ctypes

from conftest import PKG  # noqa: F401  (puts the package on sys.path)


def _opts(_lib, row_len=8, row_stride=0, flags=0):
    return _lib.CollatePairOpts(row_len, row_stride, 0, 1, 3, 2, -100, 0, 0, flags)


def _call(L, _lib, opts, a="ok", b="ok", input_ids=1, n_str=1):
    """dpt_collate_pair with non-null placeholders: 16 / 32 / 48 are never dereferenced when an argument is rejected.
    ``a`` / ``b``: "ok", None (a null side) or the name of the member to leave null."""
    def side(how):
        if how is None:
            return None
        return ctypes.byref(_lib.CollateSide(None if how == "ids" else 16, None if how == "off" else 32, None, None))
    return L.dpt_collate_pair(side(a), side(b), n_str, ctypes.byref(opts) if opts is not None else None,
                              48 if input_ids else None, None, None, None, None, None, None)


def test_library_exports_collate_pair():
    from dptok import _lib
    L = _lib.lib()
    assert hasattr(L, "dpt_collate_pair") and _lib.has_collate_pair()
    assert "dpt_collate_pair" in _lib.CALLS and "dpt_collate_pair" in _lib.EXPORTED and "dpt_collate_pair" in _lib.OPTIONAL_LATER
    assert L.dpt_abi_version() == 6


def test_structure_layouts():
    from dptok import _lib
    S, O = _lib.CollateSide, _lib.CollatePairOpts
    assert ctypes.sizeof(S) == 32
    assert [getattr(S, f).offset for f in ("ids", "off", "counts", "status")] == [0, 8, 16, 24]
    assert ctypes.sizeof(O) == 48
    fields = ("row_len", "row_stride", "pad_id", "bos_id", "sep_id", "eos_id", "ignore_id", "max_a", "max_b", "flags")
    assert [f for f, _ in O._fields_] == list(fields)
    assert [getattr(O, f).offset for f in fields] == [0, 8, 16, 20, 24, 28, 32, 36, 40, 44]


def test_argument_errors_name_the_argument():
    from dptok import _lib
    L = _lib.lib()
    for n_str in (1, 0):   # every error is found with n_str == 0 too
        ok = _opts(_lib)
        for kw, word in (({"a": None}, b"null a"), ({"b": None}, b"null b"), ({"a": "ids"}, b"a->ids"), ({"a": "off"}, b"a->off"),
                         ({"b": "ids"}, b"b->ids"), ({"b": "off"}, b"b->off"), ({"input_ids": 0}, b"input_ids")):
            assert _call(L, _lib, ok, n_str=n_str, **kw) == -1 and word in L.dpt_last_error(), kw
        assert _call(L, _lib, None, n_str=n_str) == -1 and b"opts" in L.dpt_last_error()
        assert _call(L, _lib, _opts(_lib, row_len=0), n_str=n_str) == -1 and b"row_len" in L.dpt_last_error()
        three = _lib.COLLATE_BOS | _lib.COLLATE_SEP | _lib.COLLATE_EOS
        assert _call(L, _lib, _opts(_lib, row_len=2, flags=three), n_str=n_str) == -1 and b"row_len" in L.dpt_last_error()
        assert _call(L, _lib, _opts(_lib, row_len=0, flags=_lib.COLLATE_SEP), n_str=n_str) == -1 and b"row_len" in L.dpt_last_error()
        assert _call(L, _lib, _opts(_lib, row_len=(1 << 31) + 1), n_str=n_str) == -1 and b"row_len" in L.dpt_last_error()
        assert _call(L, _lib, _opts(_lib, row_stride=7), n_str=n_str) == -1 and b"row_stride" in L.dpt_last_error()
        assert _call(L, _lib, _opts(_lib, flags=256), n_str=n_str) == -1 and b"flags" in L.dpt_last_error()
        assert _call(L, _lib, _opts(_lib, flags=1 << 31), n_str=n_str) == -1 and b"flags" in L.dpt_last_error()


def test_empty_call_is_ok():
    from dptok import _lib
    L = _lib.lib()
    assert _call(L, _lib, _opts(_lib, row_stride=12), n_str=0) == 0
    assert _call(L, _lib, _opts(_lib, row_len=3, flags=255), n_str=0) == 0
    assert _call(L, _lib, _opts(_lib, row_len=1 << 31), n_str=0) == 0


def test_python_call_builds_the_options():
    from dptok import _lib, collate
    assert (_lib.COLLATE_SEP, _lib.COLLATE_MASK_A, _lib.COLLATE_TRIM_A_FIRST) == (32, 64, 128)
    assert collate.collate_pair_flags() == 16
    assert collate.collate_pair_flags(sep_id=0) == 48
    assert collate.collate_pair_flags(mask_a=True, int64=False) == 64 and collate.collate_pair_flags(trim_a_first=True, int64=False) == 128
    assert collate.collate_pair_flags(bos_id=0, sep_id=4, eos_id=5, pad_left=True, trunc_left=True, int64=True, mask_a=True,
                                      trim_a_first=True) == 255
