"""Where the host-buffer calls keep their arrays in the ctx's staging buffers (csrc/dpt_host_layout.h, through
the test-only dpt_debug_host_layout).  No GPU: a layout is a pure function of the call's sizes.  Every segment
is 8-byte aligned, none overlaps the next, each keeps the room the kernels read past its payload -- the NUL
after a text or cut mask, one dword after every int32 array -- and at least the room the hand-written layout
structs gave it before the builder (EncodeLayout, SpansLayout, DecodeLayout, RoundtripLayout: their formulas
are copied below as `before`).  tests/test_gpu_hostpath.py runs the calls themselves."""
import ctypes
import itertools

import pytest

ENCODE, SPANS, DECODE, ROUNDTRIP = range(4)
CUT, WORD, EDGES = 1, 2, 4
N_STR = (0, 1, 5)
N_BYTES = (0, 1, 7, 8, 4095, 4096, 4097)
SEGS = 7
CTR = 64   # sizeof(dpt::CounterBlock)


def al8(x):
    return (x + 7) & ~7


def spec(call, nb, n, t, flags, far):
    """(in, out): per segment (name, payload bytes, least slack bytes), None for an absent optional one."""
    def text(name, k, present=True):
        return (name, k, 1) if present else None

    def i32(name, k, present=True):
        return (name, 4 * k, 4) if present else None

    def off(name):
        return (name, 8 * (n + 1), 0)
    cut, word, edges = bool(flags & CUT), bool(flags & WORD), bool(flags & EDGES)
    if call == ENCODE:
        return ([text("text", nb), off("str_off"), text("cut", nb, cut)],
                [off("id_off"), i32("status", n), i32("capped", n), ("counters", CTR, 0), i32("ids", nb),
                 ("edges", 8 * nb, 8) if edges else None, ("far", 16 * far, 0) if far else None])
    if call == SPANS:
        return ([off("str_off"), off("id_off"), i32("ids", t), i32("status", n), text("text", nb), text("cut", nb, cut)],
                [i32("tok_end", t), i32("tok_word", t, word), i32("span_status", n)])
    if call == DECODE:   # nb: the decoded bytes
        return ([off("id_off"), off("out_off"), i32("ids", t), i32("status", n)],
                [i32("dec_status", n), text("bytes", nb), ("out_len", 8 * n, 0)])
    return ([off("id_off"), off("str_off"), i32("ids", t), i32("status", n), text("text", nb)],
            [i32("rt", n), i32("first_diff", n)])


def before(call, nb, n, t, flags, far):
    """The room (bytes up to the next segment) the layout structs before the builder gave each segment, by name."""
    cut, word, edges = bool(flags & CUT), bool(flags & WORD), bool(flags & EDGES)
    if call == ENCODE:
        # in_off = al8(n_bytes + 1); in_cut = in_off + 8 * (n_str + 1); in_bytes = in_cut + al8(n_bytes + 1);
        # st = 8 * (n_str + 1); capped = st + al8(4 * n_str + 4); ctr = capped + al8(4 * n_str + 4);
        # ids = ctr + sizeof(CounterBlock); edges = ids + al8(4 * (n_bytes + 1));
        # far = edges + (with_edges ? 8 * (n_bytes + 1) : 0); out_bytes = far + 16 * far_pairs;
        return {"text": al8(nb + 1), "str_off": 8 * (n + 1), "cut": al8(nb + 1), "id_off": 8 * (n + 1),
                "status": al8(4 * n + 4), "capped": al8(4 * n + 4), "counters": CTR, "ids": al8(4 * (nb + 1)),
                "edges": 8 * (nb + 1) if edges else 0, "far": 16 * far}
    if call == SPANS:
        # in_idoff = 8 * (n_str + 1); in_ids = 2 * in_idoff; in_st = in_ids + al8(4 * n_tok + 4);
        # in_text = in_st + al8(4 * n_str); in_cut = in_text + al8(n_bytes + 1); in_bytes = in_cut + (cut ? al8(n_bytes + 1) : 0);
        # word = al8(4 * n_tok + 4); ss = with_word ? 2 * word : word; out_bytes = ss + al8(4 * n_str);
        return {"str_off": 8 * (n + 1), "id_off": 8 * (n + 1), "ids": al8(4 * t + 4), "status": al8(4 * n),
                "text": al8(nb + 1), "cut": al8(nb + 1) if cut else 0, "tok_end": al8(4 * t + 4),
                "tok_word": al8(4 * t + 4) if word else 0, "span_status": al8(4 * n)}
    if call == DECODE:
        # in_outoff = 8 * (n_str + 1); in_ids = 2 * in_outoff; in_st = in_ids + al8(4 * n_tok + 4);
        # in_bytes = in_st + al8(4 * n_str + 4); len_bytes = 8 * n_str; bytes = al8(4 * n_str + 4);
        # and the decode pass's out side: bytes + al8(decoded + 1)
        return {"id_off": 8 * (n + 1), "out_off": 8 * (n + 1), "ids": al8(4 * t + 4), "status": al8(4 * n + 4),
                "out_len": 8 * n, "dec_status": al8(4 * n + 4), "bytes": al8(nb + 1)}
    # in_stroff = 8 * (n_str + 1); in_ids = 2 * in_stroff; in_st = in_ids + al8(4 * n_tok + 4);
    # in_text = in_st + al8(4 * n_str + 4); in_bytes = in_text + al8(n_bytes + 1); fd = al8(4 * n_str + 4); out_bytes = 2 * fd;
    return {"id_off": 8 * (n + 1), "str_off": 8 * (n + 1), "ids": al8(4 * t + 4), "status": al8(4 * n + 4),
            "text": al8(nb + 1), "rt": al8(4 * n + 4), "first_diff": al8(4 * n + 4)}


@pytest.fixture(scope="module")
def layout():
    from dptok import _lib
    L = _lib.lib()

    def call(kind, nb, n, t, flags=0, far=0, rc=0):
        out = (ctypes.c_uint64 * (2 * (2 + 3 * SEGS)))()
        assert L.dpt_debug_host_layout(kind, nb, n, t, flags, far, out) == rc
        v = list(out)
        sides = []
        for base in (0, 2 + 3 * SEGS):
            k = v[base]
            assert k <= SEGS
            sides.append((v[base + 1], [tuple(v[base + 2 + 3 * i: base + 5 + 3 * i]) for i in range(k)]))
        return sides
    return call


def _grid(call):
    flag_sets = {ENCODE: (0, CUT, EDGES, CUT | EDGES), SPANS: (0, CUT, WORD, CUT | WORD), DECODE: (0,), ROUNDTRIP: (0,)}[call]
    for n, nb, flags in itertools.product(N_STR, N_BYTES, flag_sets):
        for t in sorted({0, 1, nb}):
            for far in ((0, 3) if call == ENCODE and flags & EDGES else (0,)):
                yield nb, n, t, flags, far


@pytest.mark.parametrize("call", [ENCODE, SPANS, DECODE, ROUNDTRIP])
def test_segments_are_aligned_disjoint_and_keep_their_slack(layout, call):
    for nb, n, t, flags, far in _grid(call):
        want, old = spec(call, nb, n, t, flags, far), before(call, nb, n, t, flags, far)
        for (total, segs), names in zip(layout(call, nb, n, t, flags, far), want):
            what = (call, nb, n, t, flags, far)
            assert len(segs) == len(names), what
            end = 0
            for (offset, payload, slack), name in zip(segs, names):
                assert offset % 8 == 0 and offset >= end, (what, name)   # aligned, ascending, past the one before
                if name is None:   # an absent optional segment takes no room
                    assert payload == slack == 0
                    continue
                assert payload == name[1] and slack >= name[2], (what, name)
                end = offset + payload + slack
                assert al8(payload + slack) >= old[name[0]], (what, name)   # at least the room it had
            assert total == al8(end), what   # the side ends with its last segment


def test_encode_order(layout):
    """Text sits at in-offset 0 and id_off at out-offset 0 with the head -- status, capped, counters -- ahead of the
    ids: the zero-copy call passes the in buffer as the text, the large-batch download copies the head alone."""
    for nb, n, t, flags, far in _grid(ENCODE):
        (_, ins), (_, outs) = layout(ENCODE, nb, n, t, flags, far)
        assert ins[0][0] == 0 and outs[0][0] == 0
        id_off, status, capped, ctr, ids = outs[:5]
        assert id_off[0] < status[0] < capped[0] < ctr[0] and ctr[0] + CTR <= ids[0]
        assert all(o[0] >= ids[0] + ids[1] + ids[2] for o in outs[5:] if o[1] + o[2])


def test_decode_restage_keeps_the_in_side(layout):
    """dpt_decode_host stages again once it knows the decoded size: the in side and dec_status stay where they
    were (the ids are not copied in again), only the bytes' room grows."""
    for n, t in itertools.product(N_STR, (0, 1, 4097)):
        first = layout(DECODE, 0, n, t)
        for decoded in N_BYTES[1:]:
            again = layout(DECODE, decoded, n, t)
            assert again[0] == first[0]
            assert again[1][1][0] == first[1][1][0] and again[1][1][1][0] == first[1][1][1][0]


def test_bad_arguments(layout):
    for kind, flags in ((-1, 0), (4, 0), (ENCODE, 8)):
        layout(kind, 1, 1, 1, flags, rc=-1)
