"""CPU checks of the BPE calls' C-ABI boundary (include/dpt.h dpt_bpe_create, dpt_bpe_encode, dpt_debug_bpe_lookup):
every DPT_E_ARG before a device is touched, and the pair table's bytes answering through the kernel's own probe --
every inserted pair found, every absent one missed -- on the llama table, the BLOOM-scale table and toy tables."""
import ctypes
import json

import numpy as np
import pytest

E_ARG = -1


def _lib():
    from dptok import _lib
    return _lib.lib()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _toy():
    l = np.array([0, 1, 2, 5], dtype=np.int32)
    r = np.array([1, 2, 3, 5], dtype=np.int32)
    m = np.array([4, 5, 6, 7], dtype=np.int32)
    k = np.array([0, 0, 3, 3], dtype=np.uint32)   # equal ranks on different pairs
    return l, r, m, k


def test_create_argument_errors():
    L = _lib()
    l, r, m, k = _toy()
    h = ctypes.c_void_p()
    ok = [_p(l), _p(r), _p(m), _p(k)]
    assert L.dpt_bpe_create(*ok, 4, 0, None) == E_ARG
    for i in range(4):
        args = list(ok)
        args[i] = None
        assert L.dpt_bpe_create(*args, 4, 0, ctypes.byref(h)) == E_ARG and b"null" in L.dpt_last_error()
    assert L.dpt_bpe_create(*ok, 0, 0, ctypes.byref(h)) == E_ARG
    assert L.dpt_bpe_create(*ok, 1 << 31, 0, ctypes.byref(h)) == E_ARG and b"2^31" in L.dpt_last_error()
    for which in range(3):
        arrs = [a.copy() for a in (l, r, m)]
        arrs[which][2] = -1
        assert L.dpt_bpe_create(_p(arrs[0]), _p(arrs[1]), _p(arrs[2]), _p(k), 4, 0, ctypes.byref(h)) == E_ARG
        assert b"negative" in L.dpt_last_error()
    l2 = l.copy()
    r2 = r.copy()
    l2[3], r2[3] = l[0], r[0]                                               # a key given twice
    assert L.dpt_bpe_create(_p(l2), _p(r2), _p(m), _p(k), 4, 0, ctypes.byref(h)) == E_ARG and b"twice" in L.dpt_last_error()
    k2 = k.copy()
    k2[1] = 0xFFFFFFFF
    assert L.dpt_bpe_create(_p(l), _p(r), _p(m), _p(k2), 4, 0, ctypes.byref(h)) == E_ARG
    assert not h.value and L.dpt_bpe_destroy(None) == 0


def test_encode_argument_errors():
    L = _lib()
    fake = ctypes.c_void_p(64)                                               # never dereferenced: the checks come first
    buf = np.zeros(16, dtype=np.uint64)
    p = _p(buf)
    ok = [fake, fake, p, 8, p, p, 1, p, 8, p, p, None, None]
    for i in (0, 1, 2, 4, 5, 7, 9, 10):
        args = list(ok)
        args[i] = None
        assert L.dpt_bpe_encode(*args) == E_ARG and b"null" in L.dpt_last_error(), i
    args = list(ok)
    args[8] = 7                                                              # ids_cap < n_bytes
    assert L.dpt_bpe_encode(*args) == E_ARG and b"ids_cap" in L.dpt_last_error()


def test_lookup_argument_errors():
    L = _lib()
    l, r, m, k = _toy()
    q = np.zeros(2, dtype=np.int32)
    om, ok = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.uint32)
    assert L.dpt_debug_bpe_lookup(_p(l), _p(r), _p(m), _p(k), 4, _p(q), _p(q), 2, _p(om), _p(ok)) == 0
    assert L.dpt_debug_bpe_lookup(None, _p(r), _p(m), _p(k), 4, _p(q), _p(q), 2, _p(om), _p(ok)) == E_ARG
    assert L.dpt_debug_bpe_lookup(_p(l), _p(r), _p(m), _p(k), 0, _p(q), _p(q), 2, _p(om), _p(ok)) == E_ARG
    for i in (5, 6, 8, 9):
        args = [_p(l), _p(r), _p(m), _p(k), 4, _p(q), _p(q), 2, _p(om), _p(ok)]
        args[i] = None
        assert L.dpt_debug_bpe_lookup(*args) == E_ARG
    l2, r2 = l.copy(), r.copy()
    l2[1], r2[1] = l[2], r[2]
    assert L.dpt_debug_bpe_lookup(_p(l2), _p(r2), _p(m), _p(k), 4, _p(q), _p(q), 2, _p(om), _p(ok)) == E_ARG
    assert b"twice" in L.dpt_last_error()


def _hits_and_misses(pairs, seed):
    from dptok.bpe import debug_lookup
    l, r, m, k = pairs
    om, ok = debug_lookup(l, r, m, k, l, r)
    assert np.array_equal(om, m) and np.array_equal(ok, k)                   # every inserted pair
    rng = np.random.default_rng(seed)
    hi = int(max(l.max(), r.max())) + 1
    have = set(zip(l.tolist(), r.tolist()))
    ql = np.concatenate([rng.integers(0, hi, 50000), r[:20000], l[:20000]]).astype(np.int32)   # random, swapped, left + 1
    qr = np.concatenate([rng.integers(0, hi, 50000), l[:20000], r[:20000] + 1]).astype(np.int32)
    om, ok = debug_lookup(l, r, m, k, ql, qr)
    want = dict(zip(zip(l.tolist(), r.tolist()), zip(m.tolist(), k.tolist())))
    n_miss = 0
    for a, b, gm, gk in zip(ql.tolist(), qr.tolist(), om.tolist(), ok.tolist()):
        if (a, b) in have:
            assert (gm, gk) == want[(a, b)]
        else:
            assert (gm, gk) == (-1, 0xFFFFFFFF), (a, b)
            n_miss += 1
    assert n_miss > 40000


def test_lookup_llama_table():
    pytest.importorskip("sentencepiece")
    from dptok.bpe import pairs_from_scores
    from sp_llama import SPLlama
    sp = SPLlama().sp
    n = sp.get_piece_size()
    exclude = [i for i in range(n) if sp.is_control(i) or sp.is_unknown(i) or sp.is_unused(i) or sp.is_byte(i)]
    pairs = pairs_from_scores({sp.id_to_piece(i): i for i in range(n)}, {sp.id_to_piece(i): sp.get_score(i) for i in range(n)}, exclude)
    assert len(pairs[0]) == 68229
    _hits_and_misses(pairs, 1)


def test_lookup_bloom_scale_table():
    from bloom_fixture import big_tokenizer_bytes
    from dptok.bpe import pairs_from_merges
    model = json.loads(big_tokenizer_bytes())["model"]
    pairs = pairs_from_merges(model["vocab"], model["merges"], model)
    assert len(pairs[0]) == 250420
    _hits_and_misses(pairs, 2)


def test_lookup_toy_tables():
    from dptok.bpe import debug_lookup
    l, r, m, k = _toy()
    ql, qr = np.array([0, 1, 2, 5, 1, 0, 3, 7, 5], dtype=np.int32), np.array([1, 2, 3, 5, 0, 0, 2, 7, 4], dtype=np.int32)
    om, ok = debug_lookup(l, r, m, k, ql, qr)
    assert om.tolist() == [4, 5, 6, 7, -1, -1, -1, -1, -1] and ok.tolist() == [0, 0, 3, 3] + [0xFFFFFFFF] * 5
    om, ok = debug_lookup([7], [7], [9], [12], [7, 7, 9, -1], [7, 9, 7, 7])  # one pair; a negative query misses
    assert om.tolist() == [9, -1, -1, -1] and ok.tolist() == [12] + [0xFFFFFFFF] * 3
    # ids near the top of int32, ranks near the top of uint32
    big = 0x7FFFFFFF
    om, ok = debug_lookup([big, big - 1], [big, big], [big, 3], [0xFFFFFFFE, 0], [big, big - 1, big], [big, big, big - 1])
    assert om.tolist() == [big, 3, -1] and ok.tolist() == [0xFFFFFFFE, 0, 0xFFFFFFFF]
