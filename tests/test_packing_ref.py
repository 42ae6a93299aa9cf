"""CPU checks of the packing calls: the reference's loop against its searchsorted chain, the bounds on n_rows, the
symbols, and every argument error of dpt_pack_sizes / dpt_pack_plan / dpt_pack_write (before any device work; no GPU
needed)."""
import ctypes

import numpy as np

from conftest import PKG  # noqa: F401  (puts the package on sys.path)

import packing_ref as pr


def test_loop_equals_chain_and_bounds():
    rng = np.random.default_rng(11)
    for case in range(4000):
        L = int(rng.integers(1, 40))
        n = int(rng.integers(0, 60))
        ln = pr.random_lengths(rng, n, L)
        str_row, str_col, row_first, row_fill, n_rows = pr.plan_loop(ln.tolist(), L)
        c_row, c_col, c_first, c_fill, c_rows = pr.plan_chain(ln, L)
        assert n_rows == c_rows, case
        assert str_row == c_row.tolist() and str_col == c_col.tolist(), case
        assert row_first[:n_rows] == c_first.tolist() and row_first[n_rows] == n and row_fill == c_fill.tolist(), case
        T = int(ln.sum())
        assert n_rows <= (2 * T) // L + 1 and n_rows <= int((ln > 0).sum()), case
        assert all(0 < f <= L for f in row_fill) and sum(row_fill) == T


def test_loop_row_cap_views():
    ln = [3, 0, 4, 4, 0, 0, 8, 1]
    str_row, str_col, row_first, row_fill, n_rows = pr.plan_loop(ln, 8, row_cap=5)
    assert n_rows == 4 and str_row == [0, pr.NONE, 0, 1, pr.NONE, pr.NONE, 2, 3] and str_col == [0, 0, 3, 0, 0, 0, 0, 0]
    assert row_first == [0, 3, 6, 7, 8, 8] and row_fill == [7, 4, 8, 1, 0]
    assert pr.plan_loop(ln, 8, row_cap=2)[2:4] == ([0, 3, 6], [7, 4])
    assert pr.plan_loop([0, 0], 8, row_cap=1) == ([pr.NONE] * 2, [0, 0], [2, 2], [0], 0)


def test_rows_ref_small():
    ids, off = [5, 6, 7, 8, 9, 10, 11], [10, 13, 13, 17]
    rows = pr.rows_ref(ids, off, row_len=6, pad_id=-1, bos_id=1, ignore_id=-100, flags=pr.BOS | pr.MASK_FIRST)
    assert rows[0] == [[1, 5, 6, 7, 1, -1], [1, 8, 9, 10, 11, -1]]
    assert rows[1] == [[0, 1, 2, 3, 0, 0], [0, 1, 2, 3, 4, 0]]
    assert rows[2] == [[1, 1, 1, 1, 2, 0], [1, 1, 1, 1, 1, 0]]
    assert rows[3] == [[-100, 5, 6, 7, -100, -100], [-100, 8, 9, 10, 11, -100]]
    left = pr.rows_ref(ids, off, row_len=3, flags=pr.TRUNC_LEFT | pr.EOS, eos_id=2)
    assert left[0] == [[6, 7, 2], [2, 0, 0], [10, 11, 2]]


def test_library_exports_packing():
    from dptok import _lib, packing
    L = _lib.lib()
    assert _lib.has_packing()
    want = {"dpt_pack_sizes", "dpt_pack_plan_workspace", "dpt_pack_plan", "dpt_pack_write", "dpt_debug_pack_geometry"}
    assert want == set(_lib.PACKING_CALLS) == _lib.OPTIONAL_PACKING and want <= set(_lib.EXPORTED)
    assert not (want & (_lib.OPTIONAL | _lib.OPTIONAL_LATER | _lib.OPTIONAL_PRETOK | _lib.OPTIONAL_BYTELEVEL | _lib.OPTIONAL_BPE
                        | _lib.OPTIONAL_WORDS))
    assert all(hasattr(L, name) for name in want) and L.dpt_abi_version() == 6
    B, cap = packing.pack_geometry()
    assert B >= 64 and B & (B - 1) == 0 and cap >= 1
    assert L.dpt_debug_pack_geometry(None, None) == -1
    # the workspace: at most 16 bytes per string plus a constant
    for n in (0, 1, B - 1, B, B + 1, 10 * B + 3, (1 << 31) - 1):
        assert packing.plan_workspace_bytes(n) <= 16 * n + 64
    n = ctypes.c_uint64()
    assert L.dpt_pack_plan_workspace(1 << 31, ctypes.byref(n)) == -1 and L.dpt_pack_plan_workspace(4, None) == -1
    assert packing.pack_flags() == 16 and packing.pack_flags(0, 5, True, False, True) == 1 | 2 | 8 | 256


def _opts(row_len=8, row_stride=0, flags=0):
    from dptok import _lib
    return _lib.CollateOpts(row_len, row_stride, 0, 1, 2, -100, flags)


# (the placeholder addresses 16, 32, ... are never dereferenced when an argument is rejected)
def _sizes(L, opts, off=1, lengths=1, n_str=1):
    return L.dpt_pack_sizes(16 if off else None, None, None, n_str, ctypes.byref(opts) if opts is not None else None,
                            32 if lengths else None, None)


def _plan(L, tok_off=1, n_str=1, row_len=8, row_cap=4, n_rows=1, ws=1, ws_bytes=1 << 20):
    return L.dpt_pack_plan(16 if tok_off else None, n_str, row_len, row_cap, None, None, None, None, 32 if n_rows else None,
                           48 if ws else None, ws_bytes, None)


def _write(L, opts, side=1, ids=1, off=1, tok_off=1, row_first=1, n_rows=1, input_ids=1, n_str=1, row_cap=4):
    from dptok import _lib
    s = _lib.CollateSide(16 if ids else None, 32 if off else None, None, None)
    return L.dpt_pack_write(ctypes.byref(s) if side else None, n_str, 48 if tok_off else None, 64 if row_first else None,
                            80 if n_rows else None, row_cap, ctypes.byref(opts) if opts is not None else None,
                            96 if input_ids else None, None, None, None, None)


def _bad_opts():
    """(options, the word its error names) for every option error the three calls share"""
    from dptok import _lib
    both = _lib.COLLATE_BOS | _lib.COLLATE_EOS
    return [(_opts(0), b"row_len"), (_opts(1, flags=both), b"row_len"), (_opts(0, flags=_lib.COLLATE_EOS), b"row_len"),
            (_opts((1 << 31) + 1), b"row_len"), (_opts(8, 7), b"row_stride"), (_opts(flags=_lib.COLLATE_PAD_LEFT), b"flags"),
            (_opts(flags=_lib.COLLATE_SEP), b"flags"), (_opts(flags=_lib.COLLATE_MASK_A), b"flags"), (_opts(flags=512), b"flags"),
            (_opts(flags=1 << 31), b"flags")]


def test_sizes_argument_errors():
    from dptok import _lib
    L = _lib.lib()
    for kw, word in (({"off": 0}, b"off"), ({"lengths": 0}, b"lengths")):
        assert _sizes(L, _opts(), **kw) == -1 and word in L.dpt_last_error()
    assert _sizes(L, None) == -1 and b"opts" in L.dpt_last_error()
    for opts, word in _bad_opts():
        for n_str in (1, 0):
            assert _sizes(L, opts, n_str=n_str) == -1 and word in L.dpt_last_error(), word
    assert _sizes(L, _opts(), n_str=1 << 31) == -1 and b"n_str" in L.dpt_last_error()
    for flags in (0, 1 | 2 | 8 | 16 | 256):
        assert _sizes(L, _opts(8, 12, flags), n_str=0) == 0


def test_plan_argument_errors():
    from dptok import _lib, packing
    L = _lib.lib()
    for kw, word in (({"tok_off": 0}, b"tok_off"), ({"n_rows": 0}, b"n_rows"), ({"ws": 0}, b"ws"), ({"row_len": 0}, b"row_len"),
                     ({"row_len": (1 << 31) + 1}, b"row_len"), ({"n_str": 1 << 31}, b"n_str"), ({"row_cap": 1 << 31}, b"row_cap")):
        assert _plan(L, **kw) == -1 and word in L.dpt_last_error(), word
    for kw in ({"tok_off": 0}, {"n_rows": 0}, {"row_len": 0}, {"row_cap": 1 << 31}):   # found with n_str == 0 too
        assert _plan(L, n_str=0, **kw) == -1
    need = packing.plan_workspace_bytes(5000)
    assert _plan(L, n_str=5000, ws_bytes=need - 1) == _lib.DPT_E_CAP and b"ws_bytes" in L.dpt_last_error()
    assert _plan(L, n_str=5000, ws_bytes=0) == _lib.DPT_E_CAP


def test_write_argument_errors():
    from dptok import _lib
    L = _lib.lib()
    for kw, word in (({"side": 0}, b"side"), ({"ids": 0}, b"ids"), ({"off": 0}, b"off"), ({"tok_off": 0}, b"tok_off"),
                     ({"row_first": 0}, b"row_first"), ({"n_rows": 0}, b"n_rows"), ({"input_ids": 0}, b"input_ids")):
        assert _write(L, _opts(), **kw) == -1 and word in L.dpt_last_error(), word
    assert _write(L, None) == -1 and b"opts" in L.dpt_last_error()
    for opts, word in _bad_opts():
        for n_str in (1, 0):
            assert _write(L, opts, n_str=n_str) == -1 and word in L.dpt_last_error(), word
    assert _write(L, _opts(), n_str=1 << 31) == -1 and b"n_str" in L.dpt_last_error()
    assert _write(L, _opts(), row_cap=1 << 31) == -1 and b"row_cap" in L.dpt_last_error()
    assert _write(L, _opts(), n_str=0, row_cap=1 << 31) == -1
    # the empty calls launch nothing
    for flags in (0, 1 | 2 | 8 | 16 | 256):
        assert _write(L, _opts(8, 12, flags), n_str=0) == 0
    assert _write(L, _opts(), row_cap=0) == 0
