"""Probe strings for the device byte-level pre-tokenizer's self-check (packages/tokenizer_utils.py dp_tokenize_bloom
with ``device_pretokenize=True``): each goes once through the tokenizer object's ``pre_tokenize_str`` and once
through the device rule, and the first probe whose words differ stops the construction.  They cover every
separator between letters, after a space and in a run; a space, a separator and 2- / 3- / 4-byte characters on both
edges of the kernel's 64-byte rounds; runs of spaces; leading and trailing spaces; and characters a wider or narrower
``\\s`` would class differently."""
from .bytelevel import BLOOM_SEPARATORS

_SEPS = [chr(c) for c in BLOOM_SEPARATORS]

PROBES = (
    # plain text and spacing
    ["", "x", " ", "  ", "   ", "a b", "hello world", "a  b", "a   b", "a    b", "x ", "x  ", " x", "  x", " a b ", "  a  b  ",
     "ab " * 30, "a" * 70, "hi...", "wait, what?!", "(x|y)", "[x]", "{x}", "a[b]c", "x=(1,2)", "3.14", "e.g. this", "a . b",
     "a .b", "a. b", "a ,, b", "line\nbreak", "a \n b", "a\t b", "a \tb", "\n\n", " \n", "\n ", "x\r\ny"]
    # every separator: between letters, after a space, before a space, doubled, alone, at either end
    + [t.replace("S", c) for c in _SEPS for t in ("aSb", "a Sb", "aS b", "aSSb", "S", "Sa", "aS", "a S b")]
    # the edges of the 64-byte rounds: a space in byte 63 before a letter / a separator / the end; separators and
    # longer characters straddling the edge in each of their positions
    + ["a" * k + t for k in (61, 62, 63, 64, 125, 126, 127)
       for t in (" b", " .", " ", "  b", ". b", "。b", " 。", "。 b", "😀 b", "é b", "\u00a0b", " \u2003b", " \u00a0", " [")]
    # characters near the separators that are none (written as escapes: several are invisible): other spaces,
    # zero-width characters, dashes, quotes, brackets, full-width forms, other scripts' stops, controls, marks
    + ["a\u200bb", "a\u200cb", "a\u2060b", "a\ufeffb", "a\u180eb", "a\u00adb", "a\u2010b", "a\u2014b", "a\u2018b\u2019",
       "a\u00abb\u00bb", "a\u3008b\u3009", "a\uff08b\uff09", "a\uff0eb", "a\uff01b", "a\uff1fb", "a\u061fb", "a\u061bb", "a\u0965b",
       "a\u3003b", "a\u001cb", "a\u001fb", "a\u0000b", "a\u007fb", "e\u0301 x", "\u0301", "a:b;c", "a-b_c", "it's", '"q"']
    # other scripts and 4-byte characters
    + ["café au lait", "naïve façade", "Привет, мир!", "السلام عليكم، يا", "नमस्ते। जी", "中文字。日本語、テキスト", "한국어 텍스트", "😀", "a😀b 👍🏽",
       "👨‍👩‍👧 family", "𝄞 clef", "x² ½", "α β γ"]
)
