"""Probe strings for the device pre-tokenizer's self-check (packages/tokenizer_utils.py dp_tokenize_llama with
``device_pretokenize=True``): each goes once through the tokenizer object + ``merge_tokens`` and once through the
device rule, and a certified probe whose words differ stops the construction.  They cover the rule's edge classes
-- spaces in every position, newlines and tabs, digits, punctuation, byte fallback, 2- / 3- / 4-byte characters,
literal special tokens and byte-piece names -- and the characters a normalising model would rewrite: compatibility
ligatures, full-width forms, combining marks, non-breaking and ideographic spaces, zero-width characters."""

PROBES = [
    # plain text and spacing
    "", "x", "a b", "hello world", "the weather is nice today", "a  b", "a   b", "a    b", "x ", "x  ", " x", "  x",
    " ", "  ", "a b ", " a b", "OptimalLengthTokenization", "midafternoon", "ab " * 20, "a" * 70,
    # control characters
    "\n", "\n\n", "ab\ncd", "ab\n\ncd", "\nab", "ab\n", "a \n b", "\t", "ab\tc", "x\r\ny", "a\x00b", "a\x7fb", "a\x1bb",
    # digits and punctuation
    "12345 6.78", "3.14159", "2024-01-31", "100%", "a,b;c:d", "(x)", "[y]", "{z}", "a/b\\c", "it's", '"q"', "a--b", "...",
    "e=mc^2", "x_1 + y_2", "user@example.com", "http://a.b/c?d=e&f", "#tag", "$5", "a*b", "~x", "`c`", "a|b", "<", ">", "<>",
    "a<b>c", "</", "<s", "s>",
    # special tokens and byte-piece names as text
    "<s>", "</s>", "<unk>", "<s> hello", "a<s>b", "a </s>", "<pad>", "<0x0A>", "<0x41>", "a<0x41>b", "<0xC3><0x9F>", "<0xzz>",
    # U+2581 itself
    "▁", "▁literal", "a▁b", "▁▁x",
    # accented Latin, other scripts, 4-byte characters
    "é", "café au lait", "ü ß", "naïve façade", "Ångström", "€uro", "£5 ¥6", "x²", "½ cup", "α β γ", "Привет мир",
    "السلام عليكم", "שלום", "नमस्ते", "中文字", "日本語 テキスト", "한국어", "😀", "😀 smile", "a😀b", "👍🏽", "👨‍👩‍👧", "𝄞 clef", "🇫🇷",
    # what a normaliser would rewrite (written as escapes: several are invisible)
    "\ufb01 ligature", "\ufb02ow", "\uff46\uff55\uff4c\uff4c \uff57\uff49\uff44\uff54\uff48", "\uff11\uff12\uff13",
    "e\u0301", "a\u0308 o\u0302", "\u00a0nbsp", "a\u00a0b", "a\u3000b", "a\u200bb", "\ufeffbom", "a\u00adb", "\u212b", "\u210c",
    "\u2460", "\u338f", "\u01c6", "\u1e9b\u0323", "\u2028sep", "a\u2009b", "\u2126", "\u00b5m", "\u2122", "x\u0303\u0301",
]
