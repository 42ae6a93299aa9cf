"""TEST INFRASTRUCTURE: a plain-Python model of the device-side llama-mode pre-tokenization rule
(include/dpt.h dpt_pretok_create / dpt_pretok_sizes / dpt_pretok_write; csrc/dpt_pretok.cpp and
csrc/dpt_pretok.hip): the table of a vocabulary and, per string, whether the rule certifies it and the
pre-split text + cut mask it then writes.  Bytes in, bytes out; no numpy in the rule itself."""
from __future__ import annotations

from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

WS = "▁".encode("utf-8")            # U+2581
NEEDS_HOST = 6                      # DPT_PRETOK_NEEDS_HOST
MAX_LITERALS, MAX_LITERAL_BYTES, MAX_BOS_BYTES = 32, 64, 61
E_ARG, E_VOCAB = -1, -3


def one_char(b: bytes) -> Optional[int]:
    """The code point of ``b`` when it is exactly one well-formed UTF-8 character, else None."""
    try:
        s = b.decode("utf-8")
    except UnicodeDecodeError:
        return None
    return ord(s) if len(s) == 1 else None


class Table(NamedTuple):
    known: frozenset          # code points that are a one-character piece
    runs_ok: bool             # no piece of two or more characters is '▁' only
    bos: bytes                # the BOS piece (b"": no BOS word)
    literals: Tuple[bytes, ...]


def table_from(known: Iterable[int], runs_ok: bool, bos: bytes = b"", literals: Sequence[bytes] = ()) -> Table:
    return Table(frozenset(known), bool(runs_ok), bytes(bos), tuple(bytes(x) for x in literals))


def build_table(pieces: Iterable[bytes], bos: bytes = b"", literals: Sequence[bytes] = ()):
    """The table of a vocabulary given as its pieces' bytes, or the error code the library answers."""
    literals = [bytes(x) for x in literals]
    if len(literals) > MAX_LITERALS or any(not 1 <= len(x) <= MAX_LITERAL_BYTES for x in literals) or len(bos) > MAX_BOS_BYTES:
        return E_ARG
    pieces = [bytes(p) for p in pieces if len(p)]
    have = set(pieces)
    if any(("<0x%02X>" % b).encode() not in have for b in range(256)):
        return E_VOCAB
    known, runs_ok = set(), True
    for p in pieces:
        all_ws = len(p) % 3 == 0 and p == WS * (len(p) // 3)
        if all_ws and len(p) >= 6:
            runs_ok = False
        if not all_ws and p.find(WS, 1) >= 0:
            return E_VOCAB
        cp = one_char(p)
        if cp is not None:
            known.add(cp)
    if bos and bytes(bos) not in have:
        return E_VOCAB
    return Table(frozenset(known), runs_ok, bytes(bos), tuple(literals))


def table_bytes(t: Table):
    """The table as dpt_debug_pretok_table returns it: (BMP bitmap uint32[2048], astral code points uint32[]
    ascending, literal block bytes, prefix bytes, scalars int64[4])."""
    bmp = np.zeros(2048, dtype=np.uint32)
    for cp in t.known:
        if cp < 0x10000:
            bmp[cp >> 5] |= np.uint32(1 << (cp & 31))
    astral = np.array(sorted(cp for cp in t.known if cp >= 0x10000), dtype=np.uint32)
    first = np.zeros(8, dtype=np.uint32)
    for x in t.literals:
        first[x[0] >> 5] |= np.uint32(1 << (x[0] & 31))
    off = np.zeros(len(t.literals) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(x) for x in t.literals], dtype=np.int64)
    lit = first.tobytes() + off.tobytes() + b"".join(t.literals)
    scalars = np.array([int(t.runs_ok), len(t.known), len(t.literals), len(t.bos)], dtype=np.int64)
    return bmp, astral, lit, t.bos + WS, scalars


def presplit_one(t: Table, s: bytes) -> Tuple[int, bytes, bytes]:
    """One string -> (pre_status, text2, cut mask): (6, b"", b"") when the rule does not certify it."""
    refused = (NEEDS_HOST, b"", b"")
    if s[:1] == b" " or WS in s or any(x in s for x in t.literals) or (not t.runs_ok and b"  " in s):
        return refused
    try:
        chars = s.decode("utf-8")          # strict: truncated, overlong, surrogate, > U+10FFFF, stray continuation
    except UnicodeDecodeError:
        return refused
    out, cut = bytearray(t.bos), bytearray(len(t.bos))

    def put(b: bytes, opens: bool):
        out.extend(b)
        cut.extend(bytes([1 if opens else 0]) + bytes(len(b) - 1))

    if chars:
        put(WS, True)
    for ch in chars:
        if ch == " ":
            put(WS, True)
        elif ord(ch) in t.known:
            put(ch.encode("utf-8"), False)
        else:
            put(b"".join(b"<0x%02X>" % b for b in ch.encode("utf-8")), False)
    if len(out) >= 1 << 32:
        return refused
    if out:
        cut[0] = 1
    return 0, bytes(out), bytes(cut)


def presplit(t: Table, strings: Sequence[bytes]):
    """A batch -> (pre_status int32[n], out_len uint64[n], text2 bytes, cut bytes): the certified strings'
    outputs back to back."""
    st, ln, txt, cut = [], [], [], []
    for s in strings:
        a, b, c = presplit_one(t, s)
        st.append(a)
        ln.append(len(b))
        txt.append(b)
        cut.append(c)
    return np.array(st, dtype=np.int32), np.array(ln, dtype=np.uint64), b"".join(txt), b"".join(cut)


def words_of(text2: bytes, cut: bytes) -> List[str]:
    """The words a PRESPLIT call sees: text2 split where the cut mask is set."""
    starts = [i for i, c in enumerate(cut) if c] + [len(text2)]
    if not text2:
        return []
    assert starts[0] == 0
    return [text2[a:b].decode("utf-8") for a, b in zip(starts, starts[1:])]


def vocab_pieces(t2i: Dict[str, int]) -> List[bytes]:
    return [k.encode("utf-8", "surrogatepass") for k in t2i]
