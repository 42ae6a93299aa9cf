"""CPU checks for the token-spans feature: the pure-Python walk that the GPU tests take their expected
values from (tests/spans_ref.py) against hand-written cases, and the argument errors of the two
entry points (include/dpt.h dpt_token_spans, dpt_token_spans_host), which come before any device."""
import ctypes

import numpy as np
import pytest

import spans_ref


def test_walk_raw_hand_cases():
    # "ab cd": the space opens the second word and belongs to its first token
    assert spans_ref.walk_raw("ab cd", ["▁ab", "▁cd"]) == ([2, 5], [0, 1])
    assert spans_ref.walk_raw("ab cd", ["▁a", "b", "▁", "c", "d"]) == ([1, 2, 3, 4, 5], [0, 0, 1, 1, 1])
    # a newline is the six-byte atom '<0x0A>' over one input byte, and opens no word
    assert spans_ref.walk_raw("a\nb", ["▁a", "<0x0A>", "b"]) == ([1, 2, 3], [0, 0, 0])
    # multi-byte code points: ends are byte offsets
    assert spans_ref.walk_raw("é 中😀", ["▁é", "▁中", "😀"]) == ([2, 6, 10], [0, 1, 1])
    assert spans_ref.walk_raw("", []) == ([], [])
    for bad in (["▁ab", "▁cx"], ["▁ab"], ["▁ab", "▁cd", "e"], ["▁ab", "", "▁cd"]):
        with pytest.raises(AssertionError):
            spans_ref.walk_raw("ab cd", bad)


def test_walk_raw_literal_and_real_newline(vocabs):
    """A literal '<0x0A>' in the input beside a real newline: both become the token '<0x0A>', over six
    input bytes and over one."""
    from oracle import oracle
    t2i = vocabs["llama32k"]
    s = "ab<0x0A>cd\nef"
    ids, st = oracle.OracleVocab(t2i).encode_strs([s])[0]
    inv = spans_ref.invert(t2i)
    toks = [inv[i] for i in ids]
    assert st == 0 and toks == ["▁ab", "<0x0A>", "cd", "<0x0A>", "ef"]
    assert spans_ref.walk_raw(s, toks) == ([2, 8, 10, 11, 13], [0, 0, 0, 0, 0])


def test_walk_bytes_hand_cases():
    text = "▁ab▁cé".encode("utf-8")                      # bytes: ▁ 0-2, a 3, b 4, ▁ 5-7, c 8, é 9-10
    ws = np.zeros(len(text), dtype=bool)
    ws[[0, 5]] = True
    assert spans_ref.walk_bytes(text, ws, ["▁ab", "▁c", "é"]) == ([5, 9, 11], [0, 1, 1])
    assert spans_ref.walk_bytes(text, ws, ["▁", "ab", "▁cé"]) == ([3, 5, 11], [0, 0, 1])
    with pytest.raises(AssertionError):
        spans_ref.walk_bytes(text, ws, ["▁ab", "▁c"])
    with pytest.raises(AssertionError):
        spans_ref.walk_bytes(text, ws, ["▁ab", "▁cx"])


def test_expected_on_a_csr_batch(vocabs):
    """``expected`` over a batch with offsets that do not start at 0, an empty string (status 2) and a failing one."""
    from dptok import pack_strings
    from oracle import oracle
    t2i = vocabs["llama32k"]
    strs = ["zz", "ab cd", "", " x", "a\nb"]
    text, offs = pack_strings(strs)
    ids, id_off, st, _ = oracle.OracleVocab(t2i).encode_csr(text[2:], offs[1:] - offs[1])
    assert st.tolist() == [0, 2, 1, 0]
    end, word, ss = spans_ref.expected(t2i, "raw", text, offs[1:], None, ids, id_off, st)
    assert ss.tolist() == [0, 2, 1, 0]
    o = id_off.astype(np.int64)
    assert end[o[0]:o[1]][-1] == 5 and word[o[0]:o[1]].tolist()[0] == 0 and word[o[0]:o[1]].tolist()[-1] == 1
    assert o[1] == o[2] == o[3]
    assert end[o[3]:o[4]].tolist()[-1] == 3 and not word[o[3]:o[4]].any()
    assert (np.diff(end[o[0]:o[1]].astype(np.int64)) > 0).all()


def _spans_args(**over):
    """ctypes arguments of dpt_token_spans after ``v`` and before the stream: every pointer valid host
    memory unless overridden with None.  (The checks under test return before anything is read.)"""
    a = dict(mode=0, text=ctypes.create_string_buffer(b"ab"), n_bytes=2, str_off=(ctypes.c_uint64 * 2)(0, 2),
             cut_mask=None, n_str=1, ids=(ctypes.c_int32 * 2)(), id_off=(ctypes.c_uint64 * 2)(0, 1),
             status=(ctypes.c_int32 * 1)(), tok_end=(ctypes.c_uint32 * 2)(), tok_word=(ctypes.c_uint32 * 2)(),
             span_status=(ctypes.c_int32 * 1)())
    a.update(over)
    return [a[k] for k in ("mode", "text", "n_bytes", "str_off", "cut_mask", "n_str", "ids", "id_off", "status", "tok_end",
                           "tok_word", "span_status")]


@pytest.mark.parametrize("entry", ["device", "host"])
def test_spans_argument_errors_before_any_device(entry):
    from dptok import _lib
    L = _lib.lib()
    fake_v = ctypes.create_string_buffer(256)   # never read: a pointer check fails first in every call below

    def call(v, **over):
        if entry == "device":
            return L.dpt_token_spans(v, *_spans_args(**over), None)
        return L.dpt_token_spans_host(None, v, *_spans_args(**over))

    assert call(None) == -1 and b"vocab" in L.dpt_last_error()
    for name in ("str_off", "ids", "id_off", "status", "tok_end", "span_status"):
        assert call(fake_v, **{name: None}) == -1, name
        assert name.encode() in L.dpt_last_error(), (name, L.dpt_last_error())
    for mode in (1, 2):   # PRESPLIT and ATOMS need the cut mask
        assert call(fake_v, mode=mode, cut_mask=None) == -1 and b"cut_mask" in L.dpt_last_error()
    assert call(fake_v, mode=7) == -1 and b"mode" in L.dpt_last_error()
    assert call(fake_v, text=None) == -1 and b"text" in L.dpt_last_error()


def test_spans_entry_points_are_bound():
    from dptok import Encoder, TokenSpans, _lib
    assert {"dpt_token_spans", "dpt_token_spans_host"} <= set(_lib.EXPORTED)
    assert callable(Encoder.spans_device) and callable(Encoder.encode_csr_spans)
    assert TokenSpans._fields == ("ids", "offsets", "word_ids", "text")
    assert _lib.lib().dpt_abi_version() == 6
