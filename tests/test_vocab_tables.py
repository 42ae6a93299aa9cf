"""The vocabulary's device tables (build_vocab_tables in csrc/dpt_vocab.cpp, through the test-only
dpt_debug_vocab_table) against a small Python model of the documented formats: the double-array trie
(slots, slot ids, slots4 with the child filters), the two-byte root table, pair16, phase A0's byte-pair
table, the cuckoo token hash, the per-id token lengths and the scalars.  No GPU: the tables are a pure
function of the vocabulary."""
import ctypes

import numpy as np
import pytest

TERM, LEAF, BASE_MASK = 0x80000000, 0x40000000, 0x3FFFFFFF
# dpt_internal.h
PAIR16_N = 65536 + 256
TOKHASH_OFFSET = PAIR16_N * 2 + 65536 * 8
TOKHASH_MAX_BYTES_LONG = 64
TOKHASH_K = [0xFB13EED5, 0xE031651B, 0xD57B9AE9, 0xF49344BF, 0xB7A058D5, 0xB4BC663D, 0xE3606AA1, 0x829E9285, 0x9D183F11,
             0xF3C85069, 0xAEAD8A81, 0xC9C1030B, 0xC71547B7, 0xF78B48A3, 0xB5FE207F, 0xEA0A7265, 0xC71BEEC7]
M32 = 0xFFFFFFFF
SCALARS = ("root_base", "ws_node", "ws_base", "ws_id", "ids16", "id_min", "n_tab", "hash_buckets", "hash_probe", "n_tokens",
           "n_nodes", "n_slots", "max_bytes", "max_cp", "device_bytes_lo", "device_bytes_hi")


def child_bit(b):
    return (b ^ (b >> 5)) & 31


def tokhash(key, seed):
    """(h, fp) of a token's bytes: tokhash_start / step / end."""
    nd = 4 if len(key) <= 16 else (len(key) + 3) // 4
    padded = key + b"\0" * (4 * nd - len(key))
    lo, hi = (seed ^ len(key)) & M32, (seed * 0x9E3779B9) & M32
    for k in range(nd):
        t = ((int.from_bytes(padded[4 * k:4 * k + 4], "little") ^ lo) * TOKHASH_K[k] + hi) & 0xFFFFFFFFFFFFFFFF
        lo, hi = t & M32, t >> 32
    t = ((lo ^ 0x5BD1E995) * TOKHASH_K[16] + hi) & 0xFFFFFFFFFFFFFFFF
    return (t & M32) ^ (t >> 32), (t >> 32) | 1


def tokhash_alt(b, fp, mask):
    return (b ^ (fp >> 8)) & mask


# ~40 tokens: a duplicated byte string with two ids ("dup": the last wins), "<0x0A>", the word mark alone and
# with a letter, one-byte tokens that are prefixes ("a", "<") and leaves ("q", "abcd"), tokens of 17 and 65
# bytes (the 16-byte key / the hash table's 64-byte limit), two-, three- and four-byte characters.
INLINE = [("a", 0), ("b", 1), ("ab", 2), ("abc", 3), ("abcd", 4), ("<0x0A>", 5), ("▁", 6), ("▁x", 7), ("dup", 8), ("c", 9),
          ("dup", 10), ("q", 11), ("zz", 12), ("<", 13), ("<0", 14), ("é", 15), ("中", 16), ("k" * 17, 17), ("m" * 65, 18),
          ("the", 19), ("th", 20), ("he", 21), ("😀", 22), (" ", 23), ("\n", 24), ("▁the", 25), ("▁a", 26), ("e", 27),
          ("t", 28), ("h", 29), ("x", 30), ("é中", 31), ("0", 32), ("A", 33), ("0A", 34), (">", 35), ("m" * 64, 36),
          ("k" * 16, 37), ("ba", 38), ("zzz", 39)]
INLINE_BIG_ID = [(t, 40000 if t == "zz" else i) for t, i in INLINE]   # an id above 32767: no int16 staging
VOCABS = ["toy1k", "llama32k", "inline", "inline_big_id"]


def _entries(name, vocabs):
    pairs = {"inline": INLINE, "inline_big_id": INLINE_BIG_ID}.get(name) or list(vocabs[name].items())
    from dptok.engine import encode_utf8
    return [(encode_utf8(t), i) for t, i in pairs]


def _build(entries):
    """Every table of the vocabulary `entries` ([(bytes, id)]) as numpy arrays, or the error code."""
    from dptok import _lib
    L = _lib.lib()
    off = np.zeros(len(entries) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(b) for b, _ in entries], dtype=np.uint64)
    blob = np.frombuffer(b"".join(b for b, _ in entries) + b"\0", dtype=np.uint8)
    ids = np.array([i for _, i in entries], dtype=np.int32)
    out = []
    for which, dtype in enumerate((np.int32, np.int32, np.int32, np.uint8, np.uint16, np.int32)):
        size = ctypes.c_uint64(1 << 60)
        args = (blob.ctypes.data, off.ctypes.data, ids.ctypes.data, len(entries), which)
        assert L.dpt_debug_vocab_table(*args, None, 0, ctypes.byref(size)) == 0, L.dpt_last_error()
        buf = np.zeros(size.value + 8, dtype=np.uint8)
        buf[size.value:] = 0xA5
        assert L.dpt_debug_vocab_table(*args, buf.ctypes.data, size.value, ctypes.byref(size)) == 0
        assert (buf[size.value:] == 0xA5).all()
        if size.value:   # a table that does not fit is reported, not truncated
            assert L.dpt_debug_vocab_table(*args, buf.ctypes.data, size.value - 1, ctypes.byref(size)) == _lib.DPT_E_CAP
        out.append(buf[:size.value].view(dtype).copy())
    slots, slot_ids, slots4, pair, tok_len, scalars = out
    assert len(scalars) == len(SCALARS)
    n_hash = (len(pair) - TOKHASH_OFFSET) // 4
    return {"slots": slots.reshape(-1, 2), "slot_ids": slot_ids, "slots4": slots4.reshape(-1, 4),
            "pair16": pair[:PAIR16_N * 2].view(np.int16), "a0": pair[PAIR16_N * 2:TOKHASH_OFFSET].view(np.uint32).reshape(65536, 2),
            "hash": pair[TOKHASH_OFFSET:].view(np.uint32), "n_hash": n_hash, "tok_len": tok_len,
            **dict(zip(SCALARS, (int(x) for x in scalars)))}


class Model:
    """The vocabulary as the formats' documentation sees it: tokens (the last entry of equal bytes wins),
    their prefixes and each prefix's child bytes; and the walk over the tables under test."""

    def __init__(self, entries, tab):
        self.tab = tab
        self.tokens = {b: i for b, i in entries if b}
        self.children = {b"": set()}
        for tok in self.tokens:
            for k in range(len(tok)):
                self.children.setdefault(tok[:k], set()).add(tok[k])
                self.children.setdefault(tok[:k + 1], set())
        self.n_slots = tab["n_slots"]
        self.base = tab["slots"][:, 0].view(np.uint32)
        self.check = tab["slots"][:, 1]

    def step(self, node, b):
        """the child of `node` by byte b, or -1: slot t = base[node] + b with check[t] == node"""
        t = (int(self.base[node]) & BASE_MASK) + b
        return t if t < self.n_slots and int(self.check[t]) == node else -1

    def walk(self, key, node=0):
        for b in key:
            node = self.step(node, b)
            if node < 0:
                return -1
        return node


@pytest.fixture(scope="module", params=VOCABS)
def vt(request, vocabs):
    entries = _entries(request.param, vocabs)
    tab = _build(entries)
    return request.param, entries, tab, Model(entries, tab)


def test_inline_vocabulary_has_the_cases():
    toks = [t for t, _ in INLINE]
    assert toks.count("dup") == 2 and {"<0x0A>", "▁", "▁x"} <= set(toks) and 38 <= len(INLINE) <= 42
    assert {len(t.encode()) for t in toks} >= {1, 2, 3, 4, 16, 17, 64, 65}
    assert max(i for _, i in INLINE) <= 32767 < max(i for _, i in INLINE_BIG_ID)


def test_shapes_and_scalars(vt):
    name, entries, tab, m = vt
    ns = tab["n_slots"]
    assert tab["slots"].shape == (ns + 65536, 2) and tab["slots4"].shape == (ns + 65536, 4) and tab["slot_ids"].shape == (ns,)
    assert tab["root_base"] == int(m.base[0]) & BASE_MASK and int(m.check[0]) == -2
    ids = list(m.tokens.values())
    assert tab["ids16"] == int(all(0 <= i <= 32767 for i in ids))
    assert tab["ids16"] == (0 if name == "inline_big_id" else 1)
    assert tab["n_tokens"] == len(m.tokens) and tab["n_nodes"] == len(m.children)
    assert tab["max_bytes"] == max(len(t) for t in m.tokens)
    assert tab["max_cp"] == max(sum((b & 0xC0) != 0x80 for b in t) for t in m.tokens)
    ws = m.walk(b"\xE2\x96\x81")
    assert (b"\xE2\x96\x81" in m.children) == (ws >= 0) and ws != 0
    assert tab["ws_node"] == ws
    assert tab["ws_base"] == (int(m.base[ws]) & BASE_MASK if ws >= 0 else 0)
    assert tab["ws_id"] == (m.tokens.get(b"\xE2\x96\x81", -1) if ws >= 0 else -1)
    # the figure dpt_vocab_stats reports: every table's bytes but the token hash's
    dev = tab["slots"].nbytes + tab["slot_ids"].nbytes + tab["slots4"].nbytes + TOKHASH_OFFSET + tab["tok_len"].nbytes
    assert tab["device_bytes_lo"] + (tab["device_bytes_hi"] << 32) == dev


def test_every_token_walks_to_its_id_and_nothing_else_walks(vt):
    _, _, tab, m = vt
    ns = tab["n_slots"]
    assert np.array_equal(tab["slots4"][:ns, :2], tab["slots"][:ns]) and np.array_equal(tab["slots4"][:ns, 2], tab["slot_ids"])
    node_of = {}
    for prefix in m.children:
        node = m.walk(prefix)
        assert node >= 0, prefix
        node_of[prefix] = node
        word = int(m.base[node])
        is_tok = prefix in m.tokens
        assert bool(word & TERM) == is_tok, prefix
        assert int(tab["slot_ids"][node]) == (m.tokens[prefix] if is_tok else -1), prefix
        assert bool(word & LEAF) == (not m.children[prefix] and prefix != b""), prefix
        # the child filter: a bit per child byte that exists, no other
        want = 0
        for b in m.children[prefix]:
            want |= 1 << child_bit(b)
        assert int(tab["slots4"][node, 3]) & M32 == want, prefix
    assert len(set(node_of.values())) == len(node_of)
    # every other slot is free: no parent, no id, no filter
    free = np.ones(ns, dtype=bool)
    free[list(node_of.values())] = False
    assert (m.check[:ns][free] == -1).all() and (tab["slot_ids"][free] == -1).all() and not tab["slots4"][:ns][free][:, 3].any()
    # a byte string that is no token's prefix fails the check at its last byte, whatever slot it lands on
    rng = np.random.default_rng(3)
    tried = 0
    prefixes = list(m.children)
    for k in rng.permutation(len(prefixes))[:3000]:
        p = prefixes[k]
        for b in {0, 0x0A, 0x20, 0x3C, 0x61, 0x80, 0xE2, 0xFF, int(rng.integers(256))} - m.children[p]:
            assert m.step(node_of[p], b) < 0, (p, b)
            tried += 1
    assert tried > 200


def test_root_and_pair_tables_agree_with_the_two_step_walk(vt):
    _, _, tab, m = vt
    ns = tab["n_slots"]
    root2 = tab["slots"][ns:].view(np.uint32)
    root4 = tab["slots4"][ns:].view(np.uint32)
    a0 = tab["a0"]
    want2, want4 = np.zeros((65536, 2), np.uint32), np.zeros((65536, 4), np.uint32)
    want16, want_a0 = np.full(PAIR16_N, -1, np.int16), np.zeros((65536, 2), np.uint32)
    filt = tab["slots4"][:ns, 3].view(np.uint32)
    for b0 in range(256):
        s1 = m.step(0, b0)
        e1 = s1 >= 0
        term1 = e1 and bool(int(m.base[s1]) & TERM)
        assert e1 == (b0 in m.children[b""]) and term1 == (bytes([b0]) in m.tokens)
        want16[65536 + b0] = np.int32(m.tokens.get(bytes([b0]), -1)).astype(np.int16)
        for b1 in range(256):
            s2 = m.step(s1, b1) if e1 else -1
            key = bytes([b0, b1])
            assert (s2 >= 0) == (key in m.children)
            i = b0 << 8 | b1
            y = (s2 if s2 >= 0 else 0) | (LEAF if e1 else 0) | (TERM if term1 else 0)   # (bits 30 / 31 of .y)
            if s2 >= 0:
                word, tid = int(m.base[s2]), m.tokens.get(key, -1)
                want2[i] = (word, y)
                want4[i] = (word, y, tid & M32, filt[s2])
                want16[i] = np.int32(tid).astype(np.int16)   # (a 16-bit table: the kernels read it for int16 vocabularies only)
                want_a0[i] = (1 | term1 << 1 | 4 | (8 if key in m.tokens else 0) | (0 if m.children[key] else 16), filt[s2])
            else:
                want2[i] = (0, y)
                want4[i] = (0, y, M32, 0)
                want_a0[i] = (e1 | term1 << 1, 0)
        # a raw '\n' after b0 stands for "<0x0A>": its entry is (b0, '<')'s
        want_a0[b0 << 8 | 0x0A] = want_a0[b0 << 8 | 0x3C]
    assert np.array_equal(root2, want2)
    assert np.array_equal(root4, want4)
    assert np.array_equal(tab["pair16"], want16)
    assert np.array_equal(a0, want_a0)
    assert np.array_equal(a0[np.arange(256) << 8 | 0x0A], a0[np.arange(256) << 8 | 0x3C])


def test_token_hash_finds_every_token_by_the_kernels_lookup(vt):
    _, _, tab, m = vt
    h = tab["hash"]
    mask, probe, seed, nl = (int(x) for x in h[:4])
    keys = {t: i for t, i in m.tokens.items() if len(t) <= TOKHASH_MAX_BYTES_LONG}
    assert probe == 2 and mask & (mask + 1) == 0 and mask + 1 >= len(keys) > (mask + 1) // 2   # buckets of two: load <= 1/2
    assert nl == 1 + m.tokens[b"<0x0A>"] if b"<0x0A>" in m.tokens else nl == 0
    assert tab["hash_buckets"] == mask + 1 and tab["hash_probe"] == 2 and tab["n_hash"] == 4 + 4 * (mask + 1)
    buckets = h[4:].reshape(mask + 1, 2, 2)   # [bucket][entry] = {fp, id}

    def lookup(key):
        hh, fp = tokhash(key, seed)
        home = hh & mask
        for b in (home, tokhash_alt(home, fp, mask)):   # the home bucket first, then its partner
            for e in range(2):
                if int(buckets[b, e, 0]) == fp:
                    return int(buckets[b, e, 1])
        return None
    for key, tid in keys.items():
        assert lookup(key) == tid & M32, key
    # nothing else is in the table: no token of more than 64 bytes, no stale duplicate
    assert int((buckets[:, :, 0] != 0).sum()) == len(keys)


def test_tok_len_is_the_byte_length_per_id(vt):
    _, _, tab, m = vt
    ids = list(m.tokens.values())
    lo, hi = min(ids), max(ids)
    assert tab["id_min"] == lo and tab["n_tab"] == hi - lo + 1 == len(tab["tok_len"])
    want = np.zeros(hi - lo + 1, dtype=np.uint16)
    for t, i in m.tokens.items():
        assert want[i - lo] in (0, len(t))
        want[i - lo] = len(t)
    assert np.array_equal(tab["tok_len"], want)


@pytest.mark.parametrize("entries", [[("e", 5), ("▁e", 5), ("x", 6)], [("a", 0), ("b", 10**7)]],
                         ids=["one id on two lengths", "ids {0, 10^7}"])
def test_no_tok_len_table(entries):
    tab = _build([(t.encode(), i) for t, i in entries])
    assert len(tab["tok_len"]) == 0 and tab["n_tab"] == 0
    assert tab["n_tokens"] == len(entries)   # the other tables are built as ever
    m = Model([(t.encode(), i) for t, i in entries], tab)
    for t, i in entries:
        assert int(tab["slot_ids"][m.walk(t.encode())]) == i


def test_argument_errors():
    from dptok import _lib
    L = _lib.lib()
    size = ctypes.c_uint64()
    off = (ctypes.c_uint64 * 3)(0, 2, 1)
    blob = ctypes.create_string_buffer(b"ab")
    assert L.dpt_debug_vocab_table(blob, off, None, 2, 0, None, 0, ctypes.byref(size)) == -1 and b"monotone" in L.dpt_last_error()
    off = (ctypes.c_uint64 * 2)(0, 2)
    assert L.dpt_debug_vocab_table(blob, off, None, 1, 6, None, 0, ctypes.byref(size)) == -1
    assert L.dpt_debug_vocab_table(blob, off, None, 1, 0, None, 0, None) == -1
    assert L.dpt_debug_vocab_table(blob, off, None, 1, 1, None, 0, ctypes.byref(size)) == 0 and size.value >= 4 * 258 and size.value % 4 == 0
