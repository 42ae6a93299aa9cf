"""The decode table (build_detok_tables in csrc/dpt_detok.cpp, through the test-only dpt_debug_detok_table)
against the model of tests/decode_ref.py, byte for byte: the entries, the blob and the scalars, under all
three rules and with a skip list.  No GPU: the table is a pure function of its arguments."""
import ctypes

import numpy as np
import pytest

import decode_ref
import matrix_corpus as mc

# a hole (ids 3 and 41..49 have no token), two tokens on id 7 (the later wins), an empty token, a byte string
# given twice with two ids ("dup": the last entry counts, id 10; id 8 is then a hole), byte pieces, word marks,
# byte-level code points (U+0120 = ' ', U+010A = '\n', U+00C3 U+00A9 = the bytes of 'é'), a 3-byte character
INLINE = [("a", 0), ("b", 1), ("ab", 2), ("", 3), ("abcd", 4), ("<0x0A>", 5), ("▁", 6), ("▁x", 7), ("dup", 8), ("c", 9),
          ("dup", 10), ("later", 7), ("<0x41>", 12), ("<0x4g>", 13), ("<0xab>", 14), ("x<0x0A>", 15), ("▁▁a▁", 16),
          ("Ġhello", 17), ("Ċ", 18), ("Ã©", 19), ("中", 20), ("aĠ中", 21), ("é", 22), ("ŃĀ", 23), ("Ņ", 24), ("<0xFF>", 25),
          ("q" * 300, 40), ("tail", 50)]
VOCABS = ["toy1k", "llama32k", "long+40000", "sp", "bloom_big", "inline"]


@pytest.fixture(scope="module")
def pairs(vocabs):
    def get(name):
        if name == "inline":
            return [(t.encode("utf-8"), i) for t, i in INLINE]
        if name == "sp":
            from sp_llama import SPLlama
            return decode_ref.pairs_of(SPLlama().get_vocab())
        if name == "bloom_big":
            import bloom_fixture
            return decode_ref.pairs_of(bloom_fixture.big_vocab())
        return decode_ref.pairs_of(vocabs[name] if name in vocabs else mc.vocabularies()[name])
    return get


def _build(entries, rule, skip=()):
    """(entries uint32[n_tab, 2], blob bytes, id_min, n_tab, longest) as the library builds them, or its
    error code."""
    from dptok import _lib
    L = _lib.lib()
    off = np.zeros(len(entries) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(b) for b, _ in entries], dtype=np.uint64)
    blob = np.frombuffer(b"".join(b for b, _ in entries) + b"\0", dtype=np.uint8)
    ids = np.array([i for _, i in entries], dtype=np.int32)
    sk = np.array(list(skip), dtype=np.int32)
    args = (blob.ctypes.data, off.ctypes.data, ids.ctypes.data, len(entries), decode_ref.RULES[rule],
            sk.ctypes.data if len(sk) else None, len(sk))
    out = []
    for which in range(3):
        size = ctypes.c_uint64(1 << 60)
        rc = L.dpt_debug_detok_table(*args, which, None, 0, ctypes.byref(size))
        if rc != 0:
            return rc
        buf = np.zeros(size.value + 8, dtype=np.uint8)
        buf[size.value:] = 0xA5
        assert L.dpt_debug_detok_table(*args, which, buf.ctypes.data, size.value, ctypes.byref(size)) == 0
        assert (buf[size.value:] == 0xA5).all()
        if size.value:   # a table that does not fit is reported, not truncated
            assert L.dpt_debug_detok_table(*args, which, buf.ctypes.data, size.value - 1, ctypes.byref(size)) == _lib.DPT_E_CAP
        out.append(buf[:size.value].copy())
    scalars = out[2].view(np.int64)
    assert len(scalars) == 4 and int(scalars[2]) == len(out[1])
    return out[0].view(np.uint32).reshape(-1, 2), out[1].tobytes(), int(scalars[0]), int(scalars[1]), int(scalars[3])


@pytest.mark.parametrize("name", VOCABS)
def test_table_matches_model(name, pairs):
    entries = pairs(name)
    ids = sorted({i for _, i in entries})
    skips = {"none": (), "some": (ids[1], ids[len(ids) // 2], ids[1])}
    for rule in decode_ref.RULES:
        for sk, skip in skips.items():
            if sk == "some" and rule != "sp" and name != "inline":
                continue   # (the skip list does not depend on the rule: once per vocabulary, and in full on the small one)
            got = _build(entries, rule, skip)
            want = decode_ref.table(entries, rule, skip)
            assert not isinstance(got, int), (name, rule, got)
            tab, blob, id_min, n_tab, longest = got
            assert (id_min, n_tab, longest) == want[2:], (name, rule, sk)
            assert np.array_equal(tab, want[0]), (name, rule, sk, np.nonzero((tab != want[0]).any(axis=1))[0][:10])
            assert blob == want[1], (name, rule, sk)


def test_table_properties(pairs):
    assert _build(pairs("long+40000"), "sp")[2] == mc.ID_SHIFT                    # id_min != 0
    tab, blob, id_min, n_tab, longest = _build(pairs("inline"), "sp", skip=[6, 60])
    assert (id_min, n_tab, longest) == (0, 61, 300)                              # the skip id 60 widens the table
    piece = lambda i: blob[int(tab[i, 0]):int(tab[i, 0]) + int(tab[i, 1])]
    none = [i for i in range(n_tab) if tab[i, 1] == decode_ref.NONE]
    assert none == [3, 8, 11] + list(range(26, 40)) + list(range(41, 50)) + list(range(51, 60))
    assert tab[6].tolist()[1] == 0 and tab[60].tolist()[1] == 0                   # skipped: empty, not "no token"
    assert piece(7) == b"later" and piece(10) == b"dup" and piece(5) == b"\n" and piece(12) == b"A" and piece(25) == b"\xff"
    assert piece(13) == b"<0x4g>" and piece(14) == b"<0xab>" and piece(15) == b"x<0x0A>" and piece(16) == b"  a "
    tab, blob, *_ = _build(pairs("inline"), "bytelevel")
    assert piece(17) == b" hello" and piece(18) == b"\n" and piece(19) == "é".encode() and piece(20) == "中".encode()
    assert piece(21) == "aĠ中".encode() and piece(22) == b"\xe9" and piece(23) == b"\xad\x00" and piece(24) == "Ņ".encode()
    tab, blob, *_ = _build(pairs("inline"), "pieces")
    assert piece(16) == "▁▁a▁".encode() and piece(5) == b"<0x0A>"


def test_sparse_ids_and_bad_arguments(vocabs):
    from dptok import _lib
    entries = decode_ref.pairs_of(vocabs["toy1k"])
    n = len(decode_ref.entries(entries))
    lo = min(i for _, i in entries)
    fits = entries + [(b"far", lo + 8 * (n + 1) + 65536 - 1)]
    assert not isinstance(_build(fits, "sp"), int) and decode_ref.table(fits, "sp") is not None
    sparse = entries + [(b"far", lo + 8 * (n + 1) + 65536)]
    assert _build(sparse, "sp") == _lib.DPT_E_VOCAB and decode_ref.table(sparse, "sp") is None
    assert b"sparse" in _lib.lib().dpt_last_error()
    assert _build(entries, "sp", skip=[10_000_000]) == _lib.DPT_E_VOCAB           # a far skip id likewise
    L = _lib.lib()
    size = ctypes.c_uint64()
    off = (ctypes.c_uint64 * 2)(0, 1)
    blob = ctypes.create_string_buffer(b"a")
    assert L.dpt_debug_detok_table(blob, off, None, 1, 3, None, 0, 0, None, 0, ctypes.byref(size)) == -1   # no such rule
    assert L.dpt_debug_detok_table(blob, off, None, 1, 1, None, 0, 3, None, 0, ctypes.byref(size)) == -1   # no such table
    assert L.dpt_debug_detok_table(blob, off, None, 1, 1, None, 2, 0, None, 0, ctypes.byref(size)) == -1   # null skip list
    assert L.dpt_debug_detok_table(blob, off, None, 1, 1, None, 0, 0, None, 0, ctypes.byref(size)) == 0 and size.value == 8
    h = ctypes.c_void_p()
    assert L.dpt_detok_create(None, None, None, 0, 1, None, 0, 0, ctypes.byref(h)) == -1
    # the calls check their arguments before any device work
    assert L.dpt_decode_sizes(None, None, None, None, 0, 0, None, None) == -1 and b"detok" in L.dpt_last_error()
    assert L.dpt_roundtrip_host(None, None, None, None, None, None, None, 0, 0, None, None) == -1


def test_binding_exposes_every_decode_symbol():
    from dptok import _lib
    L = _lib.lib()
    want = {"dpt_detok_create", "dpt_detok_destroy", "dpt_decode_sizes", "dpt_decode", "dpt_roundtrip", "dpt_decode_host",
            "dpt_roundtrip_host", "dpt_debug_detok_table"}
    assert want == set(_lib.DECODE_CALLS) and want <= set(_lib.EXPORTED)
    for name in want:
        fn = getattr(L, name)
        assert fn.argtypes == _lib.DECODE_CALLS[name] and fn.restype is ctypes.c_int
    import dptok
    assert (dptok.RT_EQUAL, dptok.RT_DIFFERS) == (0, 5) and dptok.Detok.decode_csr and dptok.Detok.roundtrip_device
