"""The pre-tokenization table (build_pretok_tables in csrc/dpt_pretok.cpp, through the test-only
dpt_debug_pretok_table) against the model of tests/pretok_ref.py, byte for byte: the known-set bitmap, the list
above U+FFFF, the literal block, the prefix and the scalars.  No GPU: the table is a pure function of its arguments."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import pretok_ref as pr

BYTES = [("<0x%02X>" % b).encode() for b in range(256)]
WS = pr.WS


def _build(pieces, bos=b"", literals=()):
    """The five tables as the library builds them (numpy arrays / bytes), or its error code."""
    from dptok import _lib
    L = _lib.lib()
    off = np.zeros(len(pieces) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in pieces], dtype=np.uint64)
    blob = np.frombuffer(b"".join(pieces) + b"\0", dtype=np.uint8)
    lit_off = np.zeros(len(literals) + 1, dtype=np.uint64)
    lit_off[1:] = np.cumsum([len(x) for x in literals], dtype=np.uint64)
    lit = np.frombuffer(b"".join(literals) + b"\0", dtype=np.uint8)
    bosb = np.frombuffer(bos + b"\0", dtype=np.uint8)
    args = (blob.ctypes.data, off.ctypes.data, len(pieces), bosb.ctypes.data, len(bos), lit.ctypes.data, lit_off.ctypes.data,
            len(literals))
    out = []
    for which in range(5):
        size = ctypes.c_uint64(1 << 60)
        rc = L.dpt_debug_pretok_table(*args, which, None, 0, ctypes.byref(size))
        if rc != 0:
            return rc
        buf = np.zeros(size.value + 8, dtype=np.uint8)
        buf[size.value:] = 0xA5
        assert L.dpt_debug_pretok_table(*args, which, buf.ctypes.data, size.value, ctypes.byref(size)) == 0
        assert (buf[size.value:] == 0xA5).all()
        if size.value:   # a table that does not fit is reported, not truncated
            assert L.dpt_debug_pretok_table(*args, which, buf.ctypes.data, size.value - 1, ctypes.byref(size)) == _lib.DPT_E_CAP
        out.append(buf[:size.value].copy())
    return out[0].view(np.uint32), out[1].view(np.uint32), out[2].tobytes(), out[3].tobytes(), out[4].view(np.int64)


def _same(pieces, bos=b"", literals=()):
    got, want = _build(pieces, bos, literals), pr.build_table(pieces, bos, literals)
    if isinstance(want, int):
        assert got == want
        return want
    assert not isinstance(got, int), got
    wb = pr.table_bytes(want)
    assert np.array_equal(got[0], wb[0]) and np.array_equal(got[1], wb[1])
    assert got[2] == wb[2] and got[3] == wb[3] and got[4].tolist() == wb[4].tolist()
    return want


def test_llama_shaped_vocab(vocabs):
    pieces = pr.vocab_pieces(vocabs["llama32k"])
    t = _same(pieces, b"<s>" if b"<s>" in pieces else b"", [b"<s>", b"</s>", b"<unk>"])
    assert isinstance(t, pr.Table) and len(t.known) > 90 and ord("a") in t.known


def test_sentencepiece_vocab():
    pytest.importorskip("sentencepiece")
    from sp_llama import SPLlama
    t = _same(pr.vocab_pieces(SPLlama().get_vocab()), b"<s>", [b"<unk>", b"<s>", b"</s>"])
    assert isinstance(t, pr.Table) and t.runs_ok and ord("\n") not in t.known and ord("e") in t.known


def test_toy_vocabularies():
    base = BYTES + [b"<s>", b"a", b"b", WS, WS + b"ab", "é".encode(), "中".encode()]
    t = _same(base, b"<s>", [b"<s>"])
    assert t.runs_ok and t.known == {ord("a"), ord("b"), 0x2581, 0xE9, 0x4E2D}
    assert not _same(base + [WS + WS], b"<s>").runs_ok                      # a "▁▁" piece
    assert not _same(base + [WS * 4]).runs_ok
    assert _same(base + [b"a" + WS + b"b"]) == pr.E_VOCAB                   # '▁' inside a piece
    assert _same(base + [WS + WS + b"x"]) == pr.E_VOCAB
    assert _same(base + [WS + b"x" + WS]) == pr.E_VOCAB
    assert _same([p for p in base if p != b"<0x7F>"]) == pr.E_VOCAB        # a byte piece missing
    assert _same(base, b"<bos>") == pr.E_VOCAB                             # the BOS piece is no piece
    from dptok import _lib
    assert b"BOS" in _lib.lib().dpt_last_error()
    astral = _same(base + ["😀".encode(), "𝄞".encode(), b"\xf0\x9f\x98", b"\xed\xa0\x80", b"\xc0\xaf", b""], b"", [])
    assert astral.known == t.known | {0x1F600, 0x1D11E}                     # malformed pieces are no characters
    assert _build(base + ["😀".encode(), "𝄞".encode()])[1].tolist() == [0x1D11E, 0x1F600]
    dup = _same(base + [b"a", b"a"], b"<s>", [b"<s>", b"</s>", b"<s>"])     # the literal list is taken as it is
    assert len(dup.known) == len(t.known) and len(dup.literals) == 3


def test_argument_limits():
    base = BYTES + [b"<s>", b"a", b"x" * 70]
    assert _same(base, b"<s>", [b"l%02d" % k for k in range(32)]).literals[31] == b"l31"
    assert _same(base, b"<s>", [b"l%02d" % k for k in range(33)]) == pr.E_ARG
    assert _same(base, b"<s>", [b"y" * 64]).literals == (b"y" * 64,)
    assert _same(base, b"<s>", [b"y" * 65]) == pr.E_ARG
    assert _same(base, b"<s>", [b"ok", b""]) == pr.E_ARG
    assert _same(base, b"x" * 70) == pr.E_ARG                               # a BOS piece over DPT_PRETOK_MAX_BOS bytes
    from dptok import _lib
    L = _lib.lib()
    size = ctypes.c_uint64()
    off = (ctypes.c_uint64 * 2)(0, 1)
    blob = ctypes.create_string_buffer(b"a")
    assert L.dpt_debug_pretok_table(blob, off, 1, None, 0, None, None, 0, 5, None, 0, ctypes.byref(size)) == _lib.DPT_E_ARG
    assert L.dpt_debug_pretok_table(blob, off, 1, None, 2, None, None, 0, 0, None, 0, ctypes.byref(size)) == _lib.DPT_E_ARG
    assert L.dpt_debug_pretok_table(blob, off, 1, None, 0, None, None, 1, 0, None, 0, ctypes.byref(size)) == _lib.DPT_E_ARG
    assert L.dpt_debug_pretok_table(blob, off, 1, None, 0, None, None, 0, 0, None, 0, None) == _lib.DPT_E_ARG
    assert L.dpt_debug_pretok_table(blob, off, 1, None, 0, None, None, 0, 0, None, 0, ctypes.byref(size)) == _lib.DPT_E_VOCAB
    # the device calls check their arguments before any device work
    h = ctypes.c_void_p()
    assert L.dpt_pretok_create(None, None, 0, None, 0, None, None, 0, 0, ctypes.byref(h)) == _lib.DPT_E_ARG
    assert L.dpt_pretok_sizes(None, None, None, 0, None, None, None) == _lib.DPT_E_ARG and b"pretok" in L.dpt_last_error()
    assert L.dpt_pretok_write(None, None, None, 0, None, None, None, None, None) == _lib.DPT_E_ARG
    assert L.dpt_pretok_destroy(None) == 0


def test_binding_agrees_with_the_header():
    from dptok import _lib
    L = _lib.lib()
    want = {"dpt_pretok_create", "dpt_pretok_destroy", "dpt_pretok_sizes", "dpt_pretok_write", "dpt_debug_pretok_table"}
    assert want == set(_lib.PRETOK_CALLS) == _lib.OPTIONAL_PRETOK and want <= set(_lib.EXPORTED)
    assert not (want & _lib.OPTIONAL) and not (want & _lib.OPTIONAL_LATER) and _lib.has_pretok()
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
        assert fn.argtypes == types == _lib.PRETOK_CALLS[name], name
        assert fn.restype is ctypes.c_int
    assert _lib.PRETOK_NEEDS_HOST == 6 == pr.NEEDS_HOST
    hdr = open(os.path.join(ROOT, "include", "dpt.h")).read()
    assert "#define DPT_ABI_VERSION 6\n" in hdr and "#define DPT_PRETOK_NEEDS_HOST 6 " in hdr
    for macro, value in (("MAX_LITERALS", pr.MAX_LITERALS), ("MAX_LITERAL_BYTES", pr.MAX_LITERAL_BYTES), ("MAX_BOS", pr.MAX_BOS_BYTES)):
        assert "#define DPT_PRETOK_%s %d\n" % (macro, value) in hdr
    import dptok
    assert dptok.Pretok.sizes_device and dptok.Pretok.write_device and dptok.Pretok.presplit
