"""The byte-level split's separator table (build_bytelevel_tables in csrc/dpt_bytelevel.cpp, through the test-only
dpt_debug_bytelevel_table) against the model of tests/bytelevel_ref.py, byte for byte: the bitmap below U+0080, the
sorted list above and the scalars; the DPT_E_ARG cases; the binding against the header.  No GPU: the table is a pure
function of its arguments."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

import bytelevel_ref as br


def _build(seps):
    """The three tables as the library builds them (numpy arrays), or its error code."""
    from dptok import _lib
    L = _lib.lib()
    arr = np.array(list(seps) + [0], dtype=np.uint32)
    out = []
    for which in range(3):
        size = ctypes.c_uint64(1 << 60)
        rc = L.dpt_debug_bytelevel_table(arr.ctypes.data, len(seps), which, None, 0, ctypes.byref(size))
        if rc != 0:
            return rc
        buf = np.zeros(size.value + 8, dtype=np.uint8)
        buf[size.value:] = 0xA5
        assert L.dpt_debug_bytelevel_table(arr.ctypes.data, len(seps), which, buf.ctypes.data, size.value, ctypes.byref(size)) == 0
        assert (buf[size.value:] == 0xA5).all()
        if size.value:   # a table that does not fit is reported, not truncated
            assert L.dpt_debug_bytelevel_table(arr.ctypes.data, len(seps), which, buf.ctypes.data, size.value - 1,
                                               ctypes.byref(size)) == _lib.DPT_E_CAP
        out.append(buf[:size.value].copy())
    return out[0].view(np.uint64), out[1].view(np.uint32), out[2].view(np.int64)


def _same(seps):
    got, want = _build(seps), br.build_table(seps)
    if isinstance(want, int):
        assert got == want
        return want
    assert not isinstance(got, int), got
    wb = br.table_bytes(want)
    assert all(np.array_equal(g, w) for g, w in zip(got, wb)), (got, wb)
    return want


def test_bloom_table():
    t = _same(br.BLOOM_SEPARATORS)
    assert len(t) == 39
    bits, high, scalars = _build(br.BLOOM_SEPARATORS)
    assert scalars.tolist() == [39, 26] and high[0] == 0x85 and high[-1] == 0xFF0C and len(high) == 26
    assert int(bits[0]) == sum(1 << c for c in (9, 10, 11, 12, 13, 0x20, 0x21, 0x28, 0x29, 0x2C, 0x2E, 0x3F)) and int(bits[1]) == 1 << (0x7C - 64)


def test_other_sets():
    assert _same([0x20]) == {0x20}
    assert _same([0x3002, 0x20, 0x3002, 0x20, 0x7F, 0x80, 0x10FFFF, 0x1F600, 0]) == {0, 0x20, 0x7F, 0x80, 0x3002, 0x1F600, 0x10FFFF}
    assert _build([0x10FFFF, 0x20, 0xE000, 0xD7FF])[1].tolist() == [0xD7FF, 0xE000, 0x10FFFF]      # sorted, around the surrogates
    assert len(_same([0x20] + list(range(0x100, 0x1FF)))) == 256                                    # the most a table holds
    assert _build([0x20] * 256)[2].tolist() == [1, 0]                                               # duplicates collapse


def test_argument_errors():
    from dptok import _lib
    L = _lib.lib()
    assert _same([]) == br.E_ARG
    assert _same([0x20] + list(range(0x100, 0x200))) == br.E_ARG                                    # 257
    assert _same([0x2E, 0x2C]) == br.E_ARG and b"U+0020" in L.dpt_last_error()                      # no space
    assert _same([0x20, 0xD800]) == br.E_ARG and _same([0x20, 0xDFFF]) == br.E_ARG                  # surrogates
    assert _same([0x20, 0x110000]) == br.E_ARG and _same([0x20, 0xFFFFFFFF]) == br.E_ARG
    size = ctypes.c_uint64()
    sp = (ctypes.c_uint32 * 1)(0x20)
    assert L.dpt_debug_bytelevel_table(None, 1, 0, None, 0, ctypes.byref(size)) == _lib.DPT_E_ARG
    assert L.dpt_debug_bytelevel_table(sp, 1, 0, None, 0, None) == _lib.DPT_E_ARG
    assert L.dpt_debug_bytelevel_table(sp, 1, 3, None, 0, ctypes.byref(size)) == _lib.DPT_E_ARG
    assert L.dpt_debug_bytelevel_table(sp, 1, -1, None, 0, ctypes.byref(size)) == _lib.DPT_E_ARG
    assert L.dpt_debug_bytelevel_table(sp, 1, 0, None, 0, ctypes.byref(size)) == 0 and size.value == 16
    # the device calls check their arguments before any device work
    h = ctypes.c_void_p()
    assert L.dpt_bytelevel_create(None, 1, 0, ctypes.byref(h)) == _lib.DPT_E_ARG
    assert L.dpt_bytelevel_create(sp, 1, 0, None) == _lib.DPT_E_ARG
    assert L.dpt_bytelevel_create(sp, 0, 0, ctypes.byref(h)) == _lib.DPT_E_ARG
    nosp = (ctypes.c_uint32 * 1)(0x2E)
    assert L.dpt_bytelevel_create(nosp, 1, 0, ctypes.byref(h)) == _lib.DPT_E_ARG and not h.value
    assert L.dpt_bytelevel_sizes(None, None, None, 0, None, None, None) == _lib.DPT_E_ARG and b"bytelevel" in L.dpt_last_error()
    assert L.dpt_bytelevel_write(None, None, None, 0, None, None, None, None, None) == _lib.DPT_E_ARG
    assert L.dpt_bytelevel_destroy(None) == 0


def test_binding_agrees_with_the_header():
    from dptok import _lib
    L = _lib.lib()
    want = {"dpt_bytelevel_create", "dpt_bytelevel_destroy", "dpt_bytelevel_sizes", "dpt_bytelevel_write", "dpt_debug_bytelevel_table"}
    assert want == set(_lib.BYTELEVEL_CALLS) == _lib.OPTIONAL_BYTELEVEL and want <= set(_lib.EXPORTED)
    assert not (want & (_lib.OPTIONAL | _lib.OPTIONAL_LATER | _lib.OPTIONAL_PRETOK)) and _lib.has_bytelevel()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpt.h")).read(), flags=re.S)
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int}
    for name in want:
        params = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src).group(1).split(",")
        types = []
        for p in params:
            p = p.strip()
            if "*" in p:
                types.append(ctypes.POINTER(ctypes.c_uint64) if name.startswith("dpt_debug") and p.endswith("*size")
                             else ctypes.POINTER(ctypes.c_void_p) if "**" in p else ctypes.c_void_p)
            else:
                types.append(ctype[p.replace("const ", "").split()[0]])
        fn = getattr(L, name)
        assert fn.argtypes == types == _lib.BYTELEVEL_CALLS[name], name
        assert fn.restype is ctypes.c_int
    hdr = open(os.path.join(ROOT, "include", "dpt.h")).read()
    assert "#define DPT_ABI_VERSION 6\n" in hdr and "#define DPT_BYTELEVEL_MAX_SEPARATORS %d\n" % br.MAX_SEPARATORS in hdr
    import dptok
    assert dptok.ByteLevelSplit.sizes_device and dptok.ByteLevelSplit.write_device and dptok.ByteLevelSplit.split
    assert list(dptok.BLOOM_SEPARATORS) == sorted(br.BLOOM_SEPARATORS)
