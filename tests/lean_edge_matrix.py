"""TEST INFRASTRUCTURE: the edge matrix of the lean first pass (tests/test_gpu_lean_edges.py runs it; tests/test_lean_ref.py
checks on the CPU that it is what this says).

Base strings are lowercase letters with spaces at chosen positions, so that the model (tests/lean_ref.py) gives the
window lengths listed beside each -- every ``wlen % 4``, 252..256, windows ended by a last space at 1, 2, 3, 4, 127,
128, 252..255, by a space at byte 256, a second and a third window of exactly 256 bytes, long words.  Variants put
one *poison* into a base string, keeping its length and its spaces: 'é' (two bytes >= 0x80, no token), a two-byte
character that is a token (the string keeps status 0, so its ids are compared), or 0x7F (ASCII, no token by itself:
the window is not capless and the string is deferred after phase A).  Calls hold at most five strings the model
defers, so no lean wave can turn the hint off and the deferred count is exact."""
import numpy as np

import lean_ref

E = "é".encode()
DEL = b"\x7f"
SLOTS = 4          # strings per wave of the 16-lane first pass
MAX_DEFERRED = 5   # (a wave needs six deferrals of its own to turn the hint off)
# What the packing assumes of a vocabulary (the user asserts it): of the matrix's bytes only 0x7F is no token by itself,
# and as a string's first atom neither '▁' + 0x7F nor '▁' + ' ' is one -- so a base string that starts with a
# space is deferred by itself (its first window is not capless), and counts as such in every call that holds it.
GENERIC_NO_TOKEN = frozenset({0x7F})
GENERIC_FIRST_NO_TOKEN = frozenset({0x7F, 0x20})


def is_deferred(b):
    return lean_ref.deferred(b, GENERIC_NO_TOKEN, GENERIC_FIRST_NO_TOKEN)


def n_deferred(strings):
    return sum(1 for b in strings if is_deferred(b))


LOWERCASE = bytes(range(0x61, 0x7B))


def letters(n, spaces=(), seed=0, alphabet=LOWERCASE):
    """n letters of the alphabet (seeded), spaces at the given positions"""
    rng = np.random.default_rng(1000 + seed)
    b = np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), size=n)].copy()
    for k in spaces:
        b[k] = 0x20
    return b.tobytes()


def bases(alphabet=LOWERCASE):
    """[(name, bytes, [window lengths], a long word ends the walk)]; ``alphabet``: the letters (a tie-heavy
    vocabulary over three of them has many equal-cost tokenizations of every word, where the choice among them
    leans on the word-end marks of the window's records)"""
    out = []

    def add(name, n, spaces, wlens, long_word=False):
        out.append((name, letters(n, spaces, seed=len(out), alphabet=alphabet), list(wlens), long_word))
    for n in (1, 2, 3, 4, 5, 7, 8):                      # one short window
        add("len%d" % n, n, [n // 2] if n >= 5 else [], [n])
    for n in range(252, 257):                            # one window of 252..256 bytes
        add("len%d" % n, n, range(5, n - 3, 9), [n])
    for n in range(257, 261):                            # a first window of 252..255 bytes, then 5
        add("len%d" % n, n, list(range(5, n - 20, 9)) + [n - 5], [n - 5, 5])
    for p in (1, 2, 3, 4, 127, 128, 252, 253, 254, 255):   # the first window ends at a last space at p
        add("L300p%d" % p, 300, [p, 257], [p, 257 - p, 43] if p < 44 else [p, 300 - p])
        add("L513p%d" % p, 513, [p, 257], [p, 257 - p, 256])
        add("L769p%d" % p, 769, [p, 257, 513], [p, 257 - p, 256, 256])
    add("c256", 300, [256], [256, 44])                   # no space in 1..255, byte 256 a space
    add("c256x2", 513, [256, 512], [256, 256, 1])
    add("long257", 257, [], [], True)                    # no space in 1..256: a long word at once
    add("long300", 300, [257], [], True)
    add("sp0long", 300, [0], [], True)                   # byte 0 the only early space
    add("sp0", 300, [0, 200], [200, 100])
    add("sp0len256", 256, [0], [256])
    add("w3x256", 700, [100, 356, 612], [100, 256, 256, 88])   # second and third window exactly 256 bytes
    add("lean_then_long", 400, [3, 7, 330], [7], True)         # a lean window, then a word of 322 bytes
    return out


def check_bases(bs):
    """the model gives every base string the windows listed for it"""
    for name, b, wlens, long_word in bs:
        wins, lw = lean_ref.raw_windows(b)
        assert ([w for _, w in wins], lw) == (wlens, long_word), (name, wins, lw)


def _put(b, at, poison):
    """b with ``poison`` over bytes [at, at + len): None when that would cover a space or leave the window"""
    wins, _ = lean_ref.raw_windows(b)
    n = len(poison)
    if at < 0 or at + n > len(b) or 0x20 in b[at:at + n]:
        return None
    if not any(p <= at and at + n <= p + w for p, w in wins):
        return None
    return b[:at] + poison + b[at + n:]


def variants(bs, tok2):
    """{variant bytes: (base name, poison name, place)}: one poison per string.  ``tok2``: the two-byte token.
    Places: bytes 0..3 of the first window, its last bytes, the first bytes after the space that starts the second
    and the third window, the third window's last bytes, the string's last bytes.  0x7F stays off string position 0."""
    assert len(tok2) == 2 and min(tok2) >= 0x80
    out = {}
    for name, b, wlens, long_word in bs:
        wins, _ = lean_ref.raw_windows(b)
        if not wins:
            continue
        for pname, poison in (("e", E), ("t", tok2), ("d", DEL)):
            n = len(poison)
            places = [("w1+%d" % k, k) for k in range(4)] + [("w1end", wins[0][1] - n)]
            if len(wins) > 1:
                places.append(("w2+1", wins[1][0] + 1))
            if len(wins) > 2:
                places += [("w3+1", wins[2][0] + 1), ("w3end", wins[2][0] + wins[2][1] - n)]
            places.append(("end", len(b) - n))
            for place, at in places:
                if pname == "d" and at == 0:
                    continue
                if pname == "t" and place in ("w1+0", "w1+2", "w1+3"):
                    continue
                v = _put(b, at, poison)
                if v is not None:
                    out.setdefault(v, (name, pname, place))
    return out


def extras(tok2):
    """strings outside the variant scheme -> [(name, bytes)]"""
    long_word = letters(300, seed=77)
    return [("lean_long_then_hi", b"abc def " + long_word + b" " + E + b" x"),    # the retry list, not deferred
            ("lean_long_then_tok", b"abc def " + long_word + b" " + tok2 + b" x"),
            ("del_at_0", DEL + b"abc def"),                                        # judged as '▁' + 0x7F
            ("hi_then_long", E + b" " + long_word)]                                # a poisoned window first: deferred


def _clean_pool(bs):
    return [b for _, b, wlens, long_word in bs if wlens and not long_word and not is_deferred(b)]


def _fill(strings, pool, k0, front):
    """clean strings from the pool until the call is a whole number of waves (and at least two)"""
    k = k0
    while len(strings) % SLOTS or len(strings) < 2 * SLOTS:
        s = pool[k % len(pool)]
        strings.insert(0, s) if front else strings.append(s)
        k += 1
    return strings


def pack_deferred(items, bs):
    """[(name, bytes)] the model defers -> calls [(call name, [bytes])] of 1, 2, 3, 4, 5, 1, ... of them, filled up
    with clean strings to whole waves; in every other call the deferred strings come last (the last one ends the call)"""
    pool = _clean_pool(bs)
    calls, i, c = [], 0, 0
    while i < len(items):
        k = c % MAX_DEFERRED + 1
        chunk = [b for _, b in items[i:i + k]]
        last = (c // MAX_DEFERRED) % 2 == 1
        if last:
            strings = _fill(list(chunk), pool, 3 * c, front=True)
        else:   # spread: a clean string between the deferred ones
            strings = []
            for j, b in enumerate(chunk):
                strings += [b, pool[(3 * c + j) % len(pool)]]
            strings = _fill(strings, pool, 3 * c + len(chunk), front=False)
        calls.append(("%s..%d%s" % (items[i][0], len(chunk), "-last" if last else ""), strings))
        i += k
        c += 1
    return calls


def variant_calls(bs, tok2, select=None, with_extras=None):
    """the variants (``select(base name, poison, place)``: a subset) and the extras (default: with the whole set only) as
    calls of at most five deferred"""
    with_extras = select is None if with_extras is None else with_extras
    vs = variants(bs, tok2)
    # (a base string that is deferred by itself -- it starts with a space -- has no variants worth a call)
    dirty = {name for name, b, _, _ in bs if is_deferred(b)}
    items = [("%s/%s/%s" % tag, v) for v, tag in vs.items() if tag[0] not in dirty and (select is None or select(*tag))]
    deferred_items = [it for it in items if is_deferred(it[1])]
    kept = [it for it in items if it not in deferred_items]   # (a poison after a long word)
    calls = pack_deferred(deferred_items, bs)
    if with_extras:
        ex = extras(tok2)
        d = [it for it in ex if is_deferred(it[1])]
        kept += [it for it in ex if it not in d]
        calls += pack_deferred(d, bs)
    if kept:
        calls.append(("not-deferred", _fill([b for _, b in kept], _clean_pool(bs), 0, front=False)))
    return calls


def neighbour_calls(bs, tok2):
    """every base string clean and followed directly by a string that starts with 'é', with the two-byte token, with
    0x7F, by an empty string; and as the last string of the blob behind a 0..3-byte string (all four alignments of
    its start occur over the bases)"""
    calls = []
    pool = _clean_pool(bs)
    for pname, head in (("e", E), ("t", tok2), ("d", DEL)):
        if head is None:   # (a vocabulary without a two-byte token)
            continue
        strings, first = [], None
        for i, (name, b, _, _) in enumerate(bs):
            if n_deferred(strings + [b, head + b"a"]) > MAX_DEFERRED:
                # (the filler goes in front: the last deferred string ends the call)
                calls.append(("next-%s-%s" % (pname, first), _fill(strings, pool, i, front=True)))
                strings, first = [], None
            first = first or name
            strings += [b, head + b"a"]
        calls.append(("next-%s-%s" % (pname, first), _fill(strings, pool, 0, front=True)))
    for i in range(0, len(bs), 12):
        strings = []
        for name, b, _, _ in bs[i:i + 12]:
            strings += [b, b""]
        calls.append(("next-empty-%s" % bs[i][0], _fill(strings, pool, i, front=False)))
    for i, (name, b, _, _) in enumerate(bs):
        strings = [pool[i % len(pool)], pool[(i + 5) % len(pool)]]
        pad = (i - sum(len(s) for s in strings)) % 4
        strings += [b"a" * pad, b]
        assert sum(len(s) for s in strings[:-1]) % 4 == i % 4 and len(strings) == SLOTS
        calls.append(("last-%s" % name, strings))
    return calls


def alignment_calls(bs):
    """every base string with its start at each of the four byte alignments, set by a 0..3-byte string in front"""
    calls = []
    for a in range(4):
        strings, pos = [], 0
        for name, b, _, _ in bs:
            pad = (a - pos) % 4
            strings += [b"a" * pad, b]
            pos += pad + len(b)
            assert (pos - len(b)) % 4 == a
        calls.append(("align%d" % a, _fill(strings, _clean_pool(bs), a, front=False)))
    return calls


def pack(strings):
    """bytes strings back to back and a padding NUL -> (text u8[], offs u64[n+1])"""
    offs = np.zeros(len(strings) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in strings])
    return np.frombuffer(b"".join(strings) + b"\0", np.uint8).copy(), offs


def subset_select(name, poison, place):
    """the padded and the host entry's share: the strings deferred after a window (or two) staged ids, the 256-byte
    windows, each ``wlen % 4`` of a first window"""
    if place in ("w2+1", "w3+1", "w3end") and name in ("L769p1", "L513p2", "L300p3", "c256x2", "w3x256", "len259", "L513p255"):
        return True
    return place in ("w1end", "w1+1") and name in ("len256", "c256", "len5", "len7", "len253", "len254", "len255")
