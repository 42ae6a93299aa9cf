"""TEST INFRASTRUCTURE: the expected output of the decode calls (include/dpt.h dpt_detok_create,
dpt_decode, dpt_roundtrip) by a pure-Python restatement of their rules.

A decode table maps an id to the bytes it decodes to:

* ``pieces``: the token's UTF-8 bytes as they are;
* ``sp``: SentencePiece's own decode -- every U+2581 becomes ' ', a token that is exactly ``<0xNN>`` (two
  upper-case hex digits) becomes the byte NN; no UTF-8 repair;
* ``bytelevel``: every code point goes back through the GPT-2 / ByteLevel bytes-to-unicode alphabet (the 188
  printable Latin-1 bytes stand for themselves, the other 68 are U+0100.. in byte order); a token with a code
  point outside the alphabet keeps its UTF-8 bytes.

Ids of the skip list decode to nothing.  Of entries with equal bytes the last one counts, empty tokens do
not, and of two tokens on one id the later one wins.  A string's decode is the concatenation, without its
first byte when that is ' ' and ``strip`` is set.
"""
import re

import numpy as np

RULES = {"pieces": 0, "sp": 1, "bytelevel": 2}
RT_EQUAL, RT_DIFFERS, INTERNAL = 0, 5, 4
NONE = 0x80000000   # the entry of an id no token has

_PRINTABLE = list(range(0x21, 0x7F)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
_BYTE_HEX = re.compile(rb"<0x[0-9A-F]{2}>")


def bytelevel_alphabet():
    """code point -> byte for the 256 code points of the alphabet."""
    out, n = {}, 0
    for b in range(256):
        if b in _PRINTABLE:
            out[b] = b
        else:
            out[0x100 + n] = b
            n += 1
    assert len(out) == 256 and n == 68
    return out


_ALPHABET = bytelevel_alphabet()


def piece(tok: bytes, rule: str) -> bytes:
    """What one token's bytes decode to."""
    if rule == "pieces":
        return tok
    if rule == "sp":
        if _BYTE_HEX.fullmatch(tok):
            return bytes([int(tok[3:5], 16)])
        return tok.replace(b"\xe2\x96\x81", b" ")
    assert rule == "bytelevel"
    try:
        cps = [ord(c) for c in tok.decode("utf-8")]
    except UnicodeDecodeError:
        return tok
    if any(c not in _ALPHABET for c in cps):
        return tok
    return bytes(_ALPHABET[c] for c in cps)


def entries(pairs):
    """(token bytes, id) in order -> the entries that count: non-empty, the last of equal bytes."""
    last = {}
    for k, (t, _) in enumerate(pairs):
        if t:
            last[t] = k
    return [(t, i) for k, (t, i) in enumerate(pairs) if t and last[t] == k]


def pairs_of(t2i):
    return [(t.encode("utf-8", "surrogatepass"), i) for t, i in t2i.items()]


def pieces_by_id(pairs, rule, skip_ids=()):
    """id -> decoded bytes (b"" for a skipped id; an id no token has is absent)."""
    out = {}
    for t, i in entries(pairs):
        out[i] = piece(t, rule)
    for i in skip_ids:
        out[i] = b""
    return out


def table(pairs, rule, skip_ids=()):
    """The device table: (entries uint32[n_tab, 2] = {blob offset, length or NONE}, blob bytes, id_min,
    n_tab, longest piece), or None when the ids are spread over more than 8 * n_tokens + 65536 values.
    The blob holds the pieces in id order."""
    live = entries(pairs)
    by_id = pieces_by_id(pairs, rule, skip_ids)
    if not by_id:
        return None
    lo, hi = min(by_id), max(by_id)
    if hi - lo + 1 > 8 * len(live) + 65536:
        return None
    tab = np.zeros((hi - lo + 1, 2), dtype=np.uint32)
    tab[:, 1] = NONE
    blob = bytearray()
    for i in range(lo, hi + 1):
        if i in by_id:
            tab[i - lo] = (len(blob), len(by_id[i]))
            blob += by_id[i]
    return tab, bytes(blob), lo, hi - lo + 1, max(len(p) for p in by_id.values())


def decode_ids(by_id, ids, strip=False):
    """One string's ids -> (bytes, ok); ok False when an id has no piece (the bytes are then those of the
    ids before it)."""
    out = bytearray()
    ok = True
    for i in ids:
        p = by_id.get(int(i))
        if p is None:
            ok = False
            break
        out += p
    if strip and out[:1] == b" ":
        del out[0]
    return bytes(out), ok


def roundtrip_one(by_id, ids, text: bytes, strip=False):
    """(verdict, first difference or None).  A difference found in the bytes before the first id without a
    piece counts (5); else such an id gives 4."""
    dec, ok = decode_ids(by_id, ids, strip)
    n = min(len(dec), len(text))
    if dec[:n] != text[:n]:
        return RT_DIFFERS, next(k for k in range(n) if dec[k] != text[k])
    if not ok:
        return (RT_DIFFERS, len(text)) if len(dec) > len(text) else (INTERNAL, None)
    if len(dec) != len(text):
        return RT_DIFFERS, n
    return RT_EQUAL, None


def expected_decode(by_id, ids, id_off, status=None, strip=False):
    """(bytes u8[], out_off u64[n+1], dec_status i32[n], ok bool[n]) of a CSR batch; a string with a
    non-zero status decodes to nothing and keeps it, one with an id that has no piece gets 4 (ok False:
    its bytes and its length are unspecified)."""
    io = np.asarray(id_off).astype(np.int64) - int(id_off[0])
    flat = np.asarray(ids).tolist()
    n = len(io) - 1
    parts, st, good = [], np.zeros(n, np.int32), np.ones(n, bool)
    for s in range(n):
        if status is not None and status[s] != 0:
            st[s] = status[s]
            parts.append(b"")
            continue
        b, ok = decode_ids(by_id, flat[io[s]:io[s + 1]], strip)
        if not ok:
            st[s], good[s] = INTERNAL, False
        parts.append(b)
    off = np.zeros(n + 1, np.uint64)
    if n:
        off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), off, st, good


def expected_roundtrip(by_id, text, offs, ids, id_off, status=None, strip=False):
    """(rt i32[n], first_diff int64[n], -1 where rt != 5) of a CSR batch against its text."""
    o = np.asarray(offs).astype(np.int64)
    raw = bytes(np.asarray(text, dtype=np.uint8)[int(o[0]):int(o[-1])])
    o = o - o[0]
    io = np.asarray(id_off).astype(np.int64) - int(id_off[0])
    flat = np.asarray(ids).tolist()
    n = len(io) - 1
    rt, fd = np.zeros(n, np.int32), np.full(n, -1, np.int64)
    for s in range(n):
        if status is not None and status[s] != 0:
            rt[s] = status[s]
            continue
        v, d = roundtrip_one(by_id, flat[io[s]:io[s + 1]], raw[o[s]:o[s + 1]], strip)
        rt[s] = v
        if d is not None:
            fd[s] = d
    return rt, fd
