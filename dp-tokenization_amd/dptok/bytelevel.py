"""BLOOM's pre-tokenization on the device: text in, DPT_MODE_ATOMS input (text + cut mask) out."""
from __future__ import annotations

from typing import Iterable

import numpy as np

from . import _lib
from ._lib import DptError, check, destroy_handle, new_handle
from .pack import _ptr
from .pretok import two_pass_split

NEEDS_HOST = _lib.PRETOK_NEEDS_HOST

# What BLOOM's split regex " ?[^(\s|[.,!?…。，、।۔،])]+" keeps out of a word: 39 code points, found by a sweep over
# every Unicode scalar value (tests/golden/make_bloom_pretok.py).  The regex engine reads the inner '[' as a nested
# class, so '[' and ']' are not among them; '(', ')' and '|' are.
BLOOM_SEPARATORS = tuple(sorted(
    set(range(0x09, 0x0E)) | {0x20} | {ord(c) for c in "!(),.?|"} | {0x85, 0xA0, 0x060C, 0x06D4, 0x0964, 0x1680}
    | set(range(0x2000, 0x200B)) | {0x2026, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000, 0x3001, 0x3002, 0xFF0C}))


def bytes_to_unicode():
    """The GPT-2 / ByteLevel alphabet: byte -> character (0x21..0x7E, 0xA1..0xAC and 0xAE..0xFF are themselves, the
    other 68 bytes U+0100..U+0143 in order)."""
    keep = list(range(0x21, 0x7F)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    out, n = {}, 0
    for b in range(256):
        if b in keep:
            out[b] = chr(b)
        else:
            out[b] = chr(256 + n)
            n += 1
    return out


class ByteLevelSplit:
    """Device-resident separator table of a split of the family "optional U+0020, then one or more non-separators,
    isolated", followed by ByteLevel without prefix space or regex (include/dpt.h dpt_bytelevel_create): the words
    and atoms the BLOOM adapter builds from ``pre_tokenize_str`` and a dictionary lookup per character, written by
    two kernels.  The rule is exact; only strings that are not well-formed UTF-8 get ``pre_status`` NEEDS_HOST (6)
    and no output."""

    def __init__(self, separators: Iterable[int] = BLOOM_SEPARATORS, device: int = 0):
        if not _lib.has_bytelevel():   # (loads the library)
            raise DptError(f"{_lib.LIB_PATH} was built before the byte-level split calls (no dpt_bytelevel_create): rebuild it")
        seps = [int(c) for c in separators]
        if any(c < 0 or c > 0xFFFFFFFF for c in seps):
            raise DptError("ByteLevelSplit: a separator outside uint32")
        sep = np.array(seps + [0], dtype=np.uint32)
        self.handle = new_handle("dpt_bytelevel_create", _ptr(sep), len(seps), device)
        self.device = device
        self.separators = tuple(sorted(set(seps)))

    def __del__(self):
        destroy_handle(self, "handle", "dpt_bytelevel_destroy")

    # (the argument types are void*: a plain int passes as that address, 0 as NULL)
    def sizes_device(self, text_ptr: int, off_ptr: int, n_str: int, out_len_ptr: int, pre_status_ptr: int, stream: int = 0) -> None:
        """dpt_bytelevel_sizes: out_len (uint64 per string) = the bytes of each string's ATOMS form, pre_status
        (int32 per string) = 0 or NEEDS_HOST.  Device addresses, stream-ordered, no sync, no workspace."""
        check(_lib.lib().dpt_bytelevel_sizes(self.handle, text_ptr, off_ptr, n_str, out_len_ptr, pre_status_ptr, stream),
              "dpt_bytelevel_sizes")

    def write_device(self, text_ptr: int, off_ptr: int, n_str: int, pre_status_ptr: int, out_text_ptr: int, out_off_ptr: int,
                     cut_ptr: int, stream: int = 0) -> None:
        """dpt_bytelevel_write: string s's ATOMS form at out_text + out_off[s] - out_off[0] and its cut mask at the
        same index of cut (out_off: uint64[n_str + 1], the prefix sum of ``sizes_device``'s lengths from any start;
        pre_status: what it wrote)."""
        check(_lib.lib().dpt_bytelevel_write(self.handle, text_ptr, off_ptr, n_str, pre_status_ptr, out_text_ptr, out_off_ptr,
                                             cut_ptr, stream), "dpt_bytelevel_write")

    def split(self, text_t, offs_t):
        """torch device tensors in (text uint8, offsets int64[n + 1]) -> (text2 uint8, offs2 int64[n + 1] from 0,
        cut uint8, pre_status int32[n]) on the same device: sizes, a cumsum, write.  One host read (the total)."""
        return two_pass_split(self.sizes_device, self.write_device, text_t, offs_t)
