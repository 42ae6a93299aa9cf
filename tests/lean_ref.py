"""TEST INFRASTRUCTURE: a CPU model of the raw first pass's window tiling and of the lean kernel's classifier
("the lean pass and the hint"; csrc/dpt_kernels.hip: window_bounds, prep_window_lean, the LEAN == 1
refill and the deferral after phase A).  Plain Python, written from what those places document, so that a test can
say for every string of a call whether the lean kernel keeps it or defers it -- a wrong deferral changes no id, only
the count dpt_ctx_debug_lean_words reports.

The model:

* a raw string is walked in windows of at most 256 bytes (``raw_windows``);
* the lean kernel keeps a window when it is pure ASCII *and* capless: every atom of it is a token by itself
  (``lean_window``);
* a string is deferred at its first window that is not lean, unless a word too long for any window ended the walk
  before that (``predicted_deferred``): such a string goes to the 2048-byte pass's list with status 3, not to the
  lean kernel's.  Empty strings (status 2) are never deferred.
"""
from typing import Dict, FrozenSet, Iterable, List, Optional, Sequence, Set, Tuple

WINDOW = 256
SPACE, NEWLINE = 0x20, 0x0A
SPACE_MARK, NEWLINE_ATOM = "▁", "<0x0A>"


def raw_windows(b: bytes) -> Tuple[List[Tuple[int, int]], bool]:
    """The raw-mode windows [(pos, wlen), ...] of ``b`` and whether a long word ended the walk.

    At ``pos`` with ``rem`` bytes left: the whole rest when ``rem <= 256``; otherwise the window ends at the last
    space among its bytes 1..255 (byte 0 starts the window anyway), or at byte 256 -- the first byte past a full
    window -- when that is a space and so lies later; the next window starts at that space.  With neither, one word
    does not fit a window: the walk ends there (True) and what is left is the 2048-byte pass's."""
    wins: List[Tuple[int, int]] = []
    pos, n = 0, len(b)
    while pos < n:
        rem = n - pos
        if rem <= WINDOW:
            wins.append((pos, rem))
            break
        best = WINDOW if b[pos + WINDOW] == SPACE else b.rfind(b" ", pos + 1, pos + WINDOW) - pos
        if best < 1:
            return wins, True
        wins.append((pos, best))
        pos += best
    return wins, False


def _single(c: int) -> str:
    return SPACE_MARK if c == SPACE else NEWLINE_ATOM if c == NEWLINE else chr(c)


def no_token_bytes(t2i: Dict[str, int]) -> FrozenSet[int]:
    """The ASCII bytes that are no token by themselves under ``t2i``, anywhere but at a string's first byte.

    Derived from phase A's ``capb`` (a slot's flag "some atom of the window is not a token by itself", which is what
    the lean kernel defers on after phase A).  In a pure-ASCII raw window an atom is one byte, and the single-atom
    span is looked up as the reference's pretokenize_raw spells it: a space is the word-start atom '▁', '\\n'
    is the atom "<0x0A>", every other byte is itself.  So byte c is in the set iff that spelling is not a key."""
    return frozenset(c for c in range(128) if _single(c) not in t2i)


def first_no_token_bytes(t2i: Dict[str, int]) -> FrozenSet[int]:
    """The same for a string's first byte c, whose atom carries the word-start mark: '▁' + chr(c), with the
    byte as it is -- a leading space or '\\n' is not respelled (phase A's ASCII walker starts that atom at the
    '▁' node and steps over the raw byte)."""
    return frozenset(c for c in range(128) if SPACE_MARK + chr(c) not in t2i)


def lean_window(window_bytes: bytes, no_token: Iterable[int], first_no_token: Optional[Iterable[int]] = None) -> bool:
    """True when the lean kernel keeps the window: no byte >= 0x80 and no byte in ``no_token``.  For the window that
    starts its string pass ``first_no_token`` (``first_no_token_bytes``): byte 0 is judged by that set instead."""
    if any(c >= 0x80 for c in window_bytes):
        return False
    body = window_bytes
    if first_no_token is not None and len(window_bytes):
        if window_bytes[0] in first_no_token:
            return False
        body = window_bytes[1:]
    return not any(c in no_token for c in body)


def deferred(b: bytes, no_token: Iterable[int], first_no_token: Optional[Iterable[int]] = None) -> bool:
    """One string: a window that is not lean comes before any long word.  (A long word after lean windows: the
    string leaves the lean kernel with status 3, whatever follows the word.)"""
    wins, _ = raw_windows(b)
    for pos, wlen in wins:
        first = first_no_token if pos == 0 else None
        if not lean_window(b[pos:pos + wlen], no_token, first):
            return True
    return False


def predicted_deferred(strings: Sequence[bytes], no_token: Iterable[int],
                       first_no_token: Optional[Iterable[int]] = None) -> Set[int]:
    """Indices of the strings the lean kernel defers when it claims every string of the call."""
    no_token = frozenset(no_token)
    first = None if first_no_token is None else frozenset(first_no_token)
    return {i for i, b in enumerate(strings) if deferred(b, no_token, first)}


def split_blob(text, offs) -> List[bytes]:
    """The strings of a packed (text u8[], offs u64[n+1]) corpus as bytes."""
    raw = bytes(memoryview(text)) if not isinstance(text, (bytes, bytearray)) else bytes(text)
    o = [int(x) for x in offs]
    return [raw[o[i]:o[i + 1]] for i in range(len(o) - 1)]
