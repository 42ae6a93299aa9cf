"""TEST INFRASTRUCTURE: a plain-Python model of the device-side byte-level (BLOOM) pre-tokenization rule
(include/dpt.h dpt_bytelevel_create / dpt_bytelevel_sizes / dpt_bytelevel_write; csrc/dpt_bytelevel.cpp and
csrc/dpt_bytelevel.hip): the separator table and, per string, whether it is well-formed UTF-8 and the ATOMS text
+ cut mask the rule then writes.  Bytes in, bytes out; no numpy in the rule itself."""
from __future__ import annotations

from typing import Iterable, List, Sequence, Tuple

import numpy as np

NEEDS_HOST = 6                      # DPT_PRETOK_NEEDS_HOST
MAX_SEPARATORS = 256                # DPT_BYTELEVEL_MAX_SEPARATORS
E_ARG = -1

# the 39 code points BLOOM's split regex keeps out of a word, as the issue lists them
BLOOM_SEPARATORS = (list(range(0x09, 0x0E)) + [0x20] + [ord(c) for c in "!(),.?|"] + [0x85, 0xA0, 0x060C, 0x06D4, 0x0964, 0x1680]
                    + list(range(0x2000, 0x200B)) + [0x2026, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000, 0x3001, 0x3002, 0xFF0C])


def alphabet() -> List[str]:
    """byte -> its GPT-2 bytes-to-unicode character."""
    keep = set(range(0x21, 0x7F)) | set(range(0xA1, 0xAD)) | set(range(0xAE, 0x100))
    out, n = [], 0
    for b in range(256):
        if b in keep:
            out.append(chr(b))
        else:
            out.append(chr(256 + n))
            n += 1
    return out


ALPHABET = alphabet()
ATOM = [c.encode("utf-8") for c in ALPHABET]


def build_table(seps: Sequence[int]):
    """The separator set as the library keeps it (a frozenset), or the error code it answers."""
    seps = list(seps)
    if not 1 <= len(seps) <= MAX_SEPARATORS:
        return E_ARG
    if any(c < 0 or c > 0x10FFFF or 0xD800 <= c <= 0xDFFF for c in seps) or 0x20 not in seps:
        return E_ARG
    return frozenset(seps)


def table_bytes(table: frozenset):
    """The table as dpt_debug_bytelevel_table returns it: (bitmap uint64[2] of the separators below U+0080, the
    others uint32[] ascending, scalars int64[2])."""
    bits = [0, 0]
    for cp in table:
        if cp < 0x80:
            bits[cp >> 6] |= 1 << (cp & 63)
    high = np.array(sorted(cp for cp in table if cp >= 0x80), dtype=np.uint32)
    return np.array(bits, dtype=np.uint64), high, np.array([len(table), len(high)], dtype=np.int64)


def word_starts(table: frozenset, chars: str) -> List[int]:
    """The indices of ``chars`` at which a word starts: the three-character-window rule."""
    n = len(chars)
    sep = [ord(c) in table for c in chars]
    absorbed = [chars[i] == " " and i + 1 < n and not sep[i + 1] for i in range(n)]
    out = []
    for i in range(n):
        if (i == 0 or absorbed[i] or (not sep[i] and sep[i - 1] and not absorbed[i - 1])
                or (sep[i] and not absorbed[i] and not sep[i - 1])):
            out.append(i)
    return out


def words_of_text(table: frozenset, chars: str) -> List[str]:
    """The words of ``chars`` in the byte alphabet: what ``pre_tokenize_str`` answers."""
    st = word_starts(table, chars) + [len(chars)]
    return ["".join(ALPHABET[b] for b in chars[a:b].encode("utf-8")) for a, b in zip(st, st[1:])]


def split_one(table: frozenset, s: bytes) -> Tuple[int, bytes, bytes]:
    """One string -> (pre_status, ATOMS text, cut mask): (6, b"", b"") when it is not well-formed UTF-8."""
    try:
        chars = s.decode("utf-8")          # strict: truncated, overlong, surrogate, > U+10FFFF, stray continuation
    except UnicodeDecodeError:
        return NEEDS_HOST, b"", b""
    starts = set(word_starts(table, chars))
    out, cut = bytearray(), bytearray()
    for i, ch in enumerate(chars):
        for k, b in enumerate(ch.encode("utf-8")):
            out.extend(ATOM[b])
            cut.extend(bytes([3 if k == 0 and i in starts else 2]) + bytes(len(ATOM[b]) - 1))
    if len(out) >= 1 << 32:
        return NEEDS_HOST, b"", b""
    return 0, bytes(out), bytes(cut)


def split(table: frozenset, strings: Iterable[bytes]):
    """A batch -> (pre_status int32[n], out_len uint64[n], text bytes, cut bytes): the outputs back to back."""
    st, ln, txt, cut = [], [], [], []
    for s in strings:
        a, b, c = split_one(table, s)
        st.append(a)
        ln.append(len(b))
        txt.append(b)
        cut.append(c)
    return np.array(st, dtype=np.int32), np.array(ln, dtype=np.uint64), b"".join(txt), b"".join(cut)


def words_of(text2: bytes, cut: bytes) -> List[List[str]]:
    """The words of atoms an ATOMS call sees: text2 cut where bit 1 of the mask is set, grouped where bit 0 is."""
    words: List[List[str]] = []
    starts = [i for i, c in enumerate(cut) if c & 2] + [len(text2)]
    for a, b in zip(starts, starts[1:]):
        if cut[a] & 1:
            words.append([])
        words[-1].append(text2[a:b].decode("utf-8"))
    return words
