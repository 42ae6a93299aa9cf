"""CPU checks of dpt_collate's boundary: the symbol, its argument errors (before any device work) and the
empty call (no GPU needed)."""
import ctypes

from conftest import PKG  # noqa: F401  (puts the package on sys.path)


def _call(L, opts, ids=1, off=1, input_ids=1, n_str=1):
    """dpt_collate with non-null placeholders: 16 / 32 / 48 are never dereferenced when an argument is rejected."""
    return L.dpt_collate(16 if ids else None, 32 if off else None, None, None, n_str,
                         ctypes.byref(opts) if opts is not None else None, 48 if input_ids else None, None, None, None, None)


def test_library_exports_collate():
    from dptok import _lib
    L = _lib.lib()
    assert hasattr(L, "dpt_collate") and _lib.has_collate()
    assert "dpt_collate" in _lib.CALLS and "dpt_collate" in _lib.EXPORTED
    assert L.dpt_abi_version() == 6
    assert ctypes.sizeof(_lib.CollateOpts) == 40 and _lib.CollateOpts.row_stride.offset == 8 and _lib.CollateOpts.flags.offset == 32


def test_argument_errors_name_the_argument():
    from dptok import _lib
    L = _lib.lib()
    ok = _lib.CollateOpts(8, 0, 0, 1, 2, -100, 0)
    for kw, word in (({"ids": 0}, b"ids"), ({"off": 0}, b"off"), ({"input_ids": 0}, b"input_ids")):
        assert _call(L, ok, **kw) == -1 and word in L.dpt_last_error()
    assert _call(L, None) == -1 and b"opts" in L.dpt_last_error()
    assert _call(L, _lib.CollateOpts(0, 0, 0, 1, 2, -100, 0)) == -1 and b"row_len" in L.dpt_last_error()
    both = _lib.COLLATE_BOS | _lib.COLLATE_EOS
    assert _call(L, _lib.CollateOpts(1, 0, 0, 1, 2, -100, both)) == -1 and b"row_len" in L.dpt_last_error()
    assert _call(L, _lib.CollateOpts(0, 0, 0, 1, 2, -100, _lib.COLLATE_EOS)) == -1 and b"row_len" in L.dpt_last_error()
    assert _call(L, _lib.CollateOpts(8, 7, 0, 1, 2, -100, 0)) == -1 and b"row_stride" in L.dpt_last_error()
    assert _call(L, _lib.CollateOpts(8, 0, 0, 1, 2, -100, 32)) == -1 and b"flags" in L.dpt_last_error()
    assert _call(L, _lib.CollateOpts(8, 0, 0, 1, 2, -100, 1 << 31)) == -1 and b"flags" in L.dpt_last_error()
    # every error is found with n_str == 0 too
    assert _call(L, _lib.CollateOpts(8, 7, 0, 1, 2, -100, 0), n_str=0) == -1


def test_empty_call_is_ok():
    from dptok import _lib
    L = _lib.lib()
    for flags in (0, _lib.COLLATE_BOS | _lib.COLLATE_EOS | _lib.COLLATE_PAD_LEFT | _lib.COLLATE_TRUNC_LEFT | _lib.COLLATE_I64):
        assert _call(L, _lib.CollateOpts(8, 12, 0, 1, 2, -100, flags), n_str=0) == 0


def test_python_call_builds_the_options():
    from dptok import collate
    assert collate.collate_flags() == 16
    assert collate.collate_flags(bos_id=0, eos_id=5, pad_left=True, trunc_left=True, int64=False) == 15
