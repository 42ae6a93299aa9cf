"""dpt_collate_pair on the device (include/dpt.h) against tests/collate_pair_ref.py, for exact equality: row edges
under every flag combination, both store paths at every output alignment, nullable arguments and mixed layouts,
failed rows, many rows and long rows, the one-sequence call as a cross-check, both source layouts behind a real
encode on a side stream, and the Python surface.  Every output sits between sentinel guards (and has sentinels in its
[row_len, row_stride) gaps), asserted untouched."""
import itertools

import numpy as np
import pytest

import matrix_corpus as mc
from collate_harness import (BOS_ID, EOS_ID, IGNORE, OOV, PAD_ID, SENT, SEP_ID, TEXTS, Out, Side, _llama_fixture, as_numpy, assert_equal,
                             random_batch)
from collate_harness import raw_reference as make_raw_reference
from collate_pair_ref import (BOS, EOS, I64, MASK_A, PAD_LEFT, SEP, TRIM_A_FIRST, TRUNC_LEFT, collate_pair_ref, n_special)

pytestmark = pytest.mark.gpu

SEVEN = (BOS, EOS, PAD_LEFT, TRUNC_LEFT, SEP, MASK_A, TRIM_A_FIRST)
ALL128 = [sum(f for f, on in zip(SEVEN, bits) if on) for bits in itertools.product((0, 1), repeat=7)]
ROW_OUTPUTS = ("input_ids", "mask", "labels", "types")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def run_pair(torch, a, b, L, flags, *, max_a=0, max_b=0, stride=0, base=0, null=(), stream=0, check=True):
    """One dpt_collate_pair call over two uploaded sides -> (input_ids, mask, labels, types, lengths, b_start) as
    numpy, each None when named in ``null`` ("status_a" / "status_b" there: that side's status is not passed); with
    ``check`` they are compared with collate_pair_ref."""
    from dptok import collate
    n_str = a.n_str
    dtype = torch.int64 if flags & I64 else torch.int32
    outs = [None if name in null else Out(torch, n_str, L, stride, dtype, base) for name in ROW_OUTPUTS]
    assert outs[0] is not None
    o_len = None if "lengths" in null else Out(torch, 1, n_str, 0, torch.int32, 1)
    o_bst = None if "b_start" in null else Out(torch, 1, n_str, 0, torch.int32, 3)
    collate.collate_pair_device(a.ptrs("status_a" not in null), b.ptrs("status_b" not in null), n_str, outs[0].ptr(), L,
                                mask_ptr=outs[1].ptr() if outs[1] else 0, labels_ptr=outs[2].ptr() if outs[2] else 0,
                                token_type_ptr=outs[3].ptr() if outs[3] else 0, lengths_ptr=o_len.ptr() if o_len else 0,
                                b_start_ptr=o_bst.ptr() if o_bst else 0, row_stride=stride, pad_id=PAD_ID,
                                bos_id=BOS_ID if flags & BOS else None, sep_id=SEP_ID if flags & SEP else None,
                                eos_id=EOS_ID if flags & EOS else None, ignore_id=IGNORE, max_a=max_a, max_b=max_b,
                                pad_left=bool(flags & PAD_LEFT), trunc_left=bool(flags & TRUNC_LEFT), int64=bool(flags & I64),
                                mask_a=bool(flags & MASK_A), trim_a_first=bool(flags & TRIM_A_FIRST), stream=stream)
    torch.cuda.synchronize()
    got = tuple(o.rows() if o else None for o in outs) + (o_len.rows()[0] if o_len else None, o_bst.rows()[0] if o_bst else None)
    if check:
        want = collate_pair_ref(a.lists("status_a" not in null), b.lists("status_b" not in null), row_len=L, pad_id=PAD_ID,
                                bos_id=BOS_ID, sep_id=SEP_ID, eos_id=EOS_ID, ignore_id=IGNORE, max_a=max_a, max_b=max_b, flags=flags)
        assert_equal(got, want, (L, flags, max_a, max_b, stride, base, null))
    return got


def pair_sides(torch, rng, counts_a, counts_b, **kw):
    """two CSR sides with the given token counts (A's ids under 50000, B's from 100000: a mixed-up side shows)"""
    return (Side(torch, *random_batch(rng, counts_a, first=3), **kw), Side(torch, *random_batch(rng, counts_b, first=0, lo=100000), **kw))


# ------------------------------------------------------------------ 1. row edges

@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 7, 8, 9])
def test_row_edges_every_flag_combination(L, torch):
    """every (nA, nB) in [0, L + 3]^2 in one batch, under all 128 combinations of the seven non-width flags that fit L"""
    rng = np.random.default_rng(L)
    na, nb = [x.ravel() for x in np.meshgrid(np.arange(L + 4), np.arange(L + 4), indexing="ij")]
    a, b = pair_sides(torch, rng, na, nb)
    caps = (0, 1, L // 2)
    ran = 0
    for k, flags in enumerate(ALL128):
        if L < n_special(flags):
            continue
        run_pair(torch, a, b, L, flags | (I64 if k & 1 else 0), max_a=caps[k % 3], max_b=caps[(k // 3) % 3])
        ran += 1
    assert ran == {1: 64, 2: 112}.get(L, 128)   # (L = 1 holds one special at the most, L = 2 two)


SIXTEEN = [0, 255 & ~I64, BOS | SEP | EOS, PAD_LEFT | TRUNC_LEFT, MASK_A | TRIM_A_FIRST, BOS | MASK_A | PAD_LEFT,
           SEP | TRUNC_LEFT | TRIM_A_FIRST, EOS | PAD_LEFT | MASK_A | SEP, BOS | TRUNC_LEFT, SEP | MASK_A, EOS | TRIM_A_FIRST,
           BOS | EOS | PAD_LEFT | TRIM_A_FIRST, SEP | EOS | TRUNC_LEFT | MASK_A, BOS | SEP | PAD_LEFT | TRUNC_LEFT | TRIM_A_FIRST,
           TRIM_A_FIRST | TRUNC_LEFT | PAD_LEFT | MASK_A | EOS, BOS | SEP | EOS | MASK_A]


def test_the_sixteen_combinations_hold_every_flag_both_ways():
    assert len(set(SIXTEEN)) == 16
    for f in SEVEN:
        assert any(c & f for c in SIXTEEN) and any(not c & f for c in SIXTEEN)


@pytest.mark.parametrize("L", [15, 16, 17, 63, 64, 65, 129])
def test_row_edges_longer_rows(L, torch):
    rng = np.random.default_rng(L)
    caps = (0, 1, L // 2)
    for k, flags in enumerate(SIXTEEN):
        room = L - n_special(flags)
        sizes = sorted({0, 1, L // 2, room - 1, room, room + 1, L + 3})
        na, nb = [x.ravel() for x in np.meshgrid(sizes, sizes, indexing="ij")]
        a, b = pair_sides(torch, rng, na, nb)
        run_pair(torch, a, b, L, flags | (I64 if k & 1 else 0), max_a=caps[k % 3], max_b=caps[(k // 3) % 3])
        run_pair(torch, a, b, L, flags | (0 if k & 1 else I64))


def test_row_shorter_than_its_specials_is_an_argument_error(torch):
    from dptok import DptError, collate
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    before = buf.clone()
    side = (buf.data_ptr(), buf.data_ptr(), 0, 0)
    with pytest.raises(DptError, match="row_len"):
        collate.collate_pair_device(side, side, 1, buf.data_ptr() + 256, 2, bos_id=1, sep_id=3, eos_id=2)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


# ------------------------------------------------------------------ 2. alignment, both store paths

@pytest.mark.parametrize("width", [0, I64])
@pytest.mark.parametrize("L", [8, 7])
def test_alignment(L, width, torch):
    rng = np.random.default_rng(100 + L)
    ids_a, off_a = random_batch(rng, rng.integers(0, L + 2, size=301), first=123457)   # shards of larger CSR arrays
    ids_b, off_b = random_batch(rng, rng.integers(0, L + 2, size=301), first=77, lo=100000)
    a, b = Side(torch, ids_a, off_a, shift=1), Side(torch, ids_b, off_b, shift=1)
    flags = BOS | SEP | EOS | MASK_A | width
    for base in (range(2) if width else range(4)):
        for stride in (0, L, L + 1, L + 3, L + 4):
            run_pair(torch, a, b, L, flags, stride=stride, base=base)
    a3, b3 = Side(torch, ids_a, off_a, shift=3), Side(torch, ids_b, off_b, shift=2)
    run_pair(torch, a3, b3, L, PAD_LEFT | TRUNC_LEFT | TRIM_A_FIRST | width, stride=L + 4)


# ------------------------------------------------------------------ 3. nullable arguments, mixed layouts

def layouts(torch, rng, n, L, poison=False):
    """both sides in both layouts over the same tokens counts: {"csr" | "padded": (Side a, Side b)}, with statuses"""
    out = {"csr": [], "padded": []}
    for k in range(2):
        counts = rng.integers(0, L + 3, size=n)
        status = np.where(rng.random(n) < 0.2, rng.integers(1, 5, size=n), 0).astype(np.int32)
        ids, off = random_batch(rng, counts, first=1000 * (k + 1) + 1, lo=100000 * k)   # off[0] != 0 on both sides
        out["csr"].append(Side(torch, ids, off, status=status))
        # the counts layout: ranges longer than the counts; a failed string's count may hold anything
        room = counts + rng.integers(0, 5, size=n)
        ids, off = random_batch(rng, room, first=77 * (k + 1), lo=100000 * k)
        cnt = counts.astype(np.uint64)
        if poison:
            cnt[status != 0] = np.uint64(1) << np.uint64(62)
        out["padded"].append(Side(torch, ids, off, counts=cnt, status=status))
    return out


@pytest.mark.parametrize("L", [8, 7])
def test_nullable_arguments_and_mixed_layouts(L, torch):
    rng = np.random.default_rng(7)
    sides = layouts(torch, rng, 200, L)
    mixes = [("csr", "csr"), ("csr", "padded"), ("padded", "csr"), ("padded", "padded")]
    names = ("mask", "labels", "types", "lengths", "b_start")
    stats = ((), ("status_a",), ("status_b",), ("status_a", "status_b"))
    k = 0
    for r in range(len(names) + 1):
        for null in itertools.combinations(names, r):
            for width in (0, I64):
                la, lb = mixes[k % 4]
                run_pair(torch, sides[la][0], sides[lb][1], L, SEP | EOS | MASK_A | width, null=null + stats[(k // 4) % 4])
                k += 1
    assert k == 64
    for (la, lb), st in itertools.product(mixes, stats):   # every layout mix with every status passed or not
        run_pair(torch, sides[la][0], sides[lb][1], L, BOS | PAD_LEFT | TRUNC_LEFT | I64, null=st, max_a=3)


# ------------------------------------------------------------------ 4. statuses

@pytest.mark.parametrize("L", [12, 13])
def test_statuses(L, torch):
    rng = np.random.default_rng(11)
    n = 400
    sides = layouts(torch, rng, n, L, poison=True)
    sa, sb = np.asarray(sides["csr"][0].status), np.asarray(sides["csr"][1].status)
    assert ((sa != 0) & (sb == 0)).any() and ((sa == 0) & (sb != 0)).any() and ((sa != 0) & (sb != 0)).any()
    failed = (sa != 0) | (sb != 0)
    assert (failed[1:-1] & ~failed[:-2] & ~failed[2:]).any()   # a failed row between two exact ones
    for la, lb in (("csr", "csr"), ("padded", "padded"), ("csr", "padded"), ("padded", "csr")):
        for flags in (0, BOS | SEP | EOS | PAD_LEFT | TRUNC_LEFT | MASK_A | I64):
            got = run_pair(torch, sides[la][0], sides[lb][1], L, flags)
            assert (got[0][failed] == PAD_ID).all() and not got[1][failed].any() and (got[2][failed] == IGNORE).all()
            assert not got[3][failed].any() and not got[4][failed].any() and not got[5][failed].any()


# ------------------------------------------------------------------ 5. many rows, long rows

@pytest.mark.parametrize("L,n,flags", [(3, 120001, BOS | MASK_A), (61, 60001, SEP | TRUNC_LEFT | TRIM_A_FIRST),
                                       (80, 70001, I64 | BOS | EOS | PAD_LEFT)])
def test_many_rows(L, n, flags, torch):
    """More rows than a chunk holds, so the reciprocal path runs (L = 3); with 61 (element path) and 80 int64 (16-byte
    path: 40 units) elements per row more units than one sweep of the capped grid (at most 1280 resident blocks on the
    MI355X x 2048 units), so the blocks stride."""
    rng = np.random.default_rng(L)
    a, b = pair_sides(torch, rng, rng.integers(0, L + 2, size=n), rng.integers(0, L + 2, size=n))
    a.status = (rng.random(n) < 0.01).astype(np.int32) * 3
    a.d_st = torch.from_numpy(a.status).cuda()
    run_pair(torch, a, b, L, flags, null=("mask",))


@pytest.mark.parametrize("L,flags", [(100003, BOS | SEP | EOS), (100003, I64 | PAD_LEFT | TRUNC_LEFT | EOS | MASK_A),
                                     (100004, TRUNC_LEFT | BOS | TRIM_A_FIRST), (100004, I64 | SEP)])
def test_long_rows(L, flags, torch):
    """a row spans several chunks: one row that is padded and one that is truncated"""
    rng = np.random.default_rng(5)
    a, b = pair_sides(torch, rng, np.array([30000, 99999]), np.array([45000, 70000]))
    run_pair(torch, a, b, L, flags)


# ------------------------------------------------------------------ 6. the one-sequence call as a cross-check

def test_empty_b_equals_dpt_collate(torch):
    from dptok import collate
    rng = np.random.default_rng(21)
    n, L = 500, 16
    counts = rng.integers(0, 2 * L, size=n)
    status = (rng.random(n) < 0.1).astype(np.int32)
    a = Side(torch, *random_batch(rng, counts, first=9), status=status)
    b = Side(torch, [], np.full(n + 1, 4, dtype=np.uint64))
    for flags in [x | e | p | t | w for x in (0, BOS) for e in (0, EOS) for p in (0, PAD_LEFT) for t in (0, TRUNC_LEFT) for w in (0, I64)]:
        for Lx in (L, L - 1):
            got = run_pair(torch, a, b, Lx, flags)
            dtype = torch.int64 if flags & I64 else torch.int32
            one = [torch.full((n, Lx), SENT, dtype=dtype, device="cuda") for _ in range(3)]
            lens = torch.full((n,), SENT, dtype=torch.int32, device="cuda")
            collate.collate_device(a.ids_ptr, a.d_off.data_ptr(), n, one[0].data_ptr(), Lx, status_ptr=a.d_st.data_ptr(),
                                   mask_ptr=one[1].data_ptr(), labels_ptr=one[2].data_ptr(), lengths_ptr=lens.data_ptr(),
                                   pad_id=PAD_ID, bos_id=BOS_ID if flags & BOS else None, eos_id=EOS_ID if flags & EOS else None,
                                   ignore_id=IGNORE, pad_left=bool(flags & PAD_LEFT), trunc_left=bool(flags & TRUNC_LEFT),
                                   int64=bool(flags & I64))
            torch.cuda.synchronize()
            for g, w in zip(got[:3] + (got[4],), one + [lens]):
                assert g.tobytes() == w.cpu().numpy().tobytes(), (flags, Lx)


# ------------------------------------------------------------------ 7. both source layouts behind an encode

@pytest.fixture(scope="module")
def raw_reference():
    """(Encoder, ids, id_off, status) of the RAW corpus through the host path, computed once."""
    return make_raw_reference(("base",))["base"]


def test_encode_then_collate_pair_both_layouts(raw_reference, torch):
    """sources = the corpus's first half, targets = its second half: one padded encode of all 2n strings with side B as
    the offset view, and two CSR encodes; no host synchronisation between an encode and the collate"""
    from dptok import collate
    enc, ref_ids, ref_off, ref_st = raw_reference
    text, offs, _ = mc.upload("raw")
    n = (len(offs) - 1) // 2
    offs = offs[:2 * n + 1]
    ref_off, ref_st = ref_off[:2 * n + 1].astype(np.int64), ref_st[:2 * n]
    st_a, st_b = ref_st[:n].tolist(), ref_st[n:].tolist()
    cnt = np.diff(ref_off)
    assert (ref_st[:n] != 0).any() and (ref_st[n:] != 0).any() and (cnt[:n] + cnt[n:] > 128).any() and (cnt[:n] + cnt[n:] < 100).any()
    flat = ref_ids.tolist()
    ref_a = (flat, ref_off[:n + 1].tolist(), None, st_a)
    ref_b = (flat[int(ref_off[n]):], ref_off[n:].tolist(), None, st_b)
    b0, n_bytes = int(offs[0]), int(offs[-1] - offs[0])
    mid = int(offs[n] - offs[0])   # the targets' first byte
    side = torch.cuda.Stream()
    h_text, h_offs = torch.from_numpy(text).pin_memory(), torch.from_numpy(offs.view(np.int64)).pin_memory()
    d_text = torch.empty(len(text), dtype=torch.uint8, device="cuda")
    d_offs = torch.empty(2 * n + 1, dtype=torch.int64, device="cuda")
    flags = BOS | SEP | EOS | MASK_A | I64
    for L, max_a in ((128, 0), (1024, 300)):
        want = collate_pair_ref(ref_a, ref_b, row_len=L, pad_id=PAD_ID, bos_id=BOS_ID, sep_id=SEP_ID, eos_id=EOS_ID,
                                ignore_id=IGNORE, max_a=max_a, flags=flags)
        results = []
        for padded in (False, True):
            ids = torch.full((n_bytes + 1,), SENT, dtype=torch.int32, device="cuda")
            ids_b = torch.full((n_bytes - mid + 1,), SENT, dtype=torch.int32, device="cuda")   # (CSR: the targets' own encode)
            aux = torch.full((2 * n + 2,), -1, dtype=torch.int64, device="cuda")   # counts, or the two id_off arrays
            st = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
            outs = [Out(torch, n, L, 0, torch.int64) for _ in range(4)]
            lens, bst = Out(torch, 1, n, 0, torch.int32), Out(torch, 1, n, 0, torch.int32)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                d_text.copy_(h_text, non_blocking=True)
                d_offs.copy_(h_offs, non_blocking=True)
                sid = side.cuda_stream
                if padded:
                    enc.encode_device_padded(d_text.data_ptr() + b0, n_bytes, d_offs.data_ptr(), 2 * n, ids.data_ptr(), n_bytes,
                                             aux.data_ptr(), st.data_ptr(), stream=sid)
                    sa = (ids.data_ptr(), d_offs.data_ptr(), aux.data_ptr(), st.data_ptr())
                    sb = (ids.data_ptr() + 4 * mid, d_offs.data_ptr() + 8 * n, aux.data_ptr() + 8 * n, st.data_ptr() + 4 * n)
                else:
                    enc.encode_device(d_text.data_ptr() + b0, mid, d_offs.data_ptr(), n, ids.data_ptr(), n_bytes, aux.data_ptr(),
                                      st.data_ptr(), stream=sid)
                    enc.encode_device(d_text.data_ptr() + b0 + mid, n_bytes - mid, d_offs.data_ptr() + 8 * n, n, ids_b.data_ptr(),
                                      n_bytes - mid + 1, aux.data_ptr() + 8 * (n + 1), st.data_ptr() + 4 * n, stream=sid)
                    sa = (ids.data_ptr(), aux.data_ptr(), 0, st.data_ptr())
                    sb = (ids_b.data_ptr(), aux.data_ptr() + 8 * (n + 1), 0, st.data_ptr() + 4 * n)
                collate.collate_pair_device(sa, sb, n, outs[0].ptr(), L, mask_ptr=outs[1].ptr(), labels_ptr=outs[2].ptr(),
                                            token_type_ptr=outs[3].ptr(), lengths_ptr=lens.ptr(), b_start_ptr=bst.ptr(),
                                            pad_id=PAD_ID, bos_id=BOS_ID, sep_id=SEP_ID, eos_id=EOS_ID, ignore_id=IGNORE,
                                            max_a=max_a, mask_a=True, stream=sid)
            side.synchronize()
            got = tuple(o.rows() for o in outs) + (lens.rows()[0], bst.rows()[0])
            assert np.array_equal(st.cpu().numpy(), ref_st)
            assert_equal(got, want, (L, "padded" if padded else "csr"))
            results.append(got)
        for x, y in zip(*results):
            assert np.array_equal(x, y)


# ------------------------------------------------------------------ 8. the Python surface

def _as_numpy(out):
    return as_numpy(out, ("input_ids", "attention_mask", "labels", "token_type_ids", "lengths", "b_start"))


def test_pair_model_inputs(torch):
    from dptok import collate
    rng = np.random.default_rng(3)
    n = 50
    ca, cb = rng.integers(0, 30, size=n), rng.integers(0, 30, size=n)
    ca[7], cb[7] = 40, 41
    ids_a, off_a = random_batch(rng, ca, first=5)
    status = np.zeros(n, dtype=np.int32)
    status[[3, 7]] = 1   # the longest pair failed (its target): it does not set the row length
    room_b = np.concatenate([[0], np.cumsum(cb + 2)]).astype(np.int64)   # side B in the counts layout
    ids_b = rng.integers(100000, 150000, size=int(room_b[-1])).astype(np.int32)
    longest = int((ca + cb)[status == 0].max())
    capped = int((np.minimum(ca, 9) + np.minimum(cb, 11))[status == 0].max())
    A = (torch.from_numpy(ids_a).cuda(), torch.from_numpy(off_a.view(np.int64)).cuda())
    B = (torch.from_numpy(ids_b).cuda(), torch.from_numpy(room_b).cuda(), torch.from_numpy(status).cuda(),
         torch.from_numpy(cb.astype(np.int64)).cuda())
    ref_a, ref_b = (ids_a.tolist(), off_a.tolist(), None, None), (ids_b.tolist(), room_b.tolist(), cb.tolist(), status.tolist())
    cases = [(dict(padding="longest"), longest + 2, 0), (dict(padding="longest", max_length=16), 16, 0),
             (dict(padding="longest", pad_to_multiple_of=8), -(-(longest + 2) // 8) * 8, 0),
             (dict(padding="longest", max_source=9, max_target=11), capped + 2, 0),
             (dict(padding="max_length", max_length=64, mask_source=True), 64, MASK_A),
             (dict(padding="max_length", max_length=13, pad_to_multiple_of=8, trim="source", padding_side="left",
                   truncation_side="left"), 16, TRIM_A_FIRST | PAD_LEFT | TRUNC_LEFT)]
    for kw, L, flags in cases:
        for int64, extra in ((True, True), (False, False)):
            out = collate.pair_model_inputs(A, B, sep_id=SEP_ID, eos_id=EOS_ID, pad_id=PAD_ID, labels=extra, token_type_ids=extra,
                                            int64=int64, **kw)
            assert set(out) == {"input_ids", "attention_mask", "lengths", "b_start"} | ({"labels", "token_type_ids"} if extra else set())
            for k in ("input_ids", "attention_mask") + (("labels", "token_type_ids") if extra else ()):
                assert out[k].shape == (n, L) and out[k].dtype == (torch.int64 if int64 else torch.int32) and out[k].is_cuda
            assert out["lengths"].shape == out["b_start"].shape == (n,) and out["b_start"].dtype == torch.int32
            want = collate_pair_ref(ref_a, ref_b, row_len=L, pad_id=PAD_ID, sep_id=SEP_ID, eos_id=EOS_ID, ignore_id=IGNORE,
                                    max_a=kw.get("max_source", 0), max_b=kw.get("max_target", 0), flags=flags | SEP | EOS)
            assert_equal(_as_numpy(out), want, kw)
    empty = collate.pair_model_inputs((A[0][:0], A[1][:1]), (B[0][:0], B[1][:1]), padding="longest", pad_to_multiple_of=8)
    assert empty["input_ids"].shape == (0, 8) and empty["b_start"].shape == (0,)
    with pytest.raises(ValueError):
        collate.pair_model_inputs(A, (B[0], B[1][:-1]))
    with pytest.raises(ValueError):
        collate.pair_model_inputs(A, B, trim="both")


SOURCES = TEXTS
TARGETS = ["nice weather", "x", "a longer target sentence for the shortest source", "b", "hello hello world", "y"]


def reference_collator(torch, sources, targets, pad_id):
    """ShortcutDataCollatorForSeq2Seq on features of (source ids, target ids): the concatenations, right-padded with the
    pad id; the labels are that same tensor"""
    from torch.nn.utils.rnn import pad_sequence
    rows = [torch.tensor(s + t, dtype=torch.int64) for s, t in zip(sources, targets)]
    padded = pad_sequence(rows, padding_value=pad_id, batch_first=True)
    return padded, padded


def _check_pair_adapter(torch, dp_tokenize, tokenizer, sources, targets, bad_text=None):
    from packages.tokenizer_utils import _special_ids
    src, tgt = dp_tokenize.batch(sources), dp_tokenize.batch(targets)
    _, _, pad = _special_ids(tokenizer)
    want_ids, want_labels = reference_collator(torch, src, tgt, pad)
    out = dp_tokenize.batch_pair_model_inputs(sources, targets)
    assert out["input_ids"].is_cuda and out["input_ids"].dtype == torch.int64 and "status_source" not in out
    assert torch.equal(out["input_ids"].cpu(), want_ids) and torch.equal(out["labels"].cpu(), want_labels)
    assert out["lengths"].tolist() == [len(s) + len(t) for s, t in zip(src, tgt)]
    assert out["b_start"].tolist() == [len(s) for s in src]
    assert torch.equal(out["attention_mask"].sum(1).int(), out["lengths"])
    # the other arguments reach the call
    flat = lambda lists: ([i for x in lists for i in x], np.concatenate([[0], np.cumsum([len(x) for x in lists])]).tolist(), None, None)  # noqa: E731
    got = dp_tokenize.batch_pair_model_inputs(sources, targets, max_length=12, padding="max_length", max_source=5, sep_id=SEP_ID,
                                              mask_source=True, ignore_id=-100, token_type_ids=True, trim="source",
                                              padding_side="left", truncation_side="left", pad_to_multiple_of=8)
    want = collate_pair_ref(flat(src), flat(tgt), row_len=16, pad_id=pad, sep_id=SEP_ID, ignore_id=-100, max_a=5,
                            flags=SEP | MASK_A | TRIM_A_FIRST | PAD_LEFT | TRUNC_LEFT | I64)
    assert_equal(_as_numpy(got), want, "arguments")
    with pytest.raises(ValueError):
        dp_tokenize.batch_pair_model_inputs(sources, targets[:-1])
    masked = dp_tokenize.batch_pair_model_inputs(sources, targets, errors="mask", max_length=9, padding="max_length")
    assert masked["status_source"].dtype == torch.int32 and not masked["status_source"].any() and not masked["status_target"].any()
    if bad_text is None:
        return
    # an untokenizable word in a source, and in a target two rows on: the exception of ``batch`` for the first in row
    # order, or the pad rows and their statuses
    bad_src = list(sources[:1]) + [bad_text] + list(sources[1:])
    bad_tgt = list(targets[:3]) + [bad_text + " x"] + list(targets[3:])
    ok_src, ok_tgt = list(sources[:1]) + ["x"] + list(sources[1:]), list(targets[:3]) + ["x"] + list(targets[3:])
    same_row = list(targets[:1]) + [bad_text + " x"] + list(targets[1:])   # (a row's source comes before its target)
    for s_list, t_list, first in ((bad_src, ok_tgt, bad_text), (ok_src, bad_tgt, bad_text + " x"), (bad_src, bad_tgt, bad_text),
                                  (bad_src, same_row, bad_text)):
        with pytest.raises(Exception) as e_batch:
            dp_tokenize.batch([first])
        with pytest.raises(type(e_batch.value)) as e_pair:
            dp_tokenize.batch_pair_model_inputs(s_list, t_list)
        assert type(e_batch.value) is ValueError and str(e_pair.value) == str(e_batch.value)
    out = dp_tokenize.batch_pair_model_inputs(bad_src, bad_tgt, errors="mask", max_length=9, padding="max_length")
    n = len(bad_src)
    assert out["status_source"].tolist() == [0, 1] + [0] * (n - 2) and out["status_target"].tolist() == [0, 0, 0, 1] + [0] * (n - 4)
    for r in (1, 3):
        assert (out["input_ids"][r] == pad).all() and not out["attention_mask"][r].any() and int(out["lengths"][r]) == 0
        assert (out["labels"][r] == pad).all() and int(out["b_start"][r]) == 0
    assert torch.equal(out["input_ids"][0], masked["input_ids"][0]) and torch.equal(out["input_ids"][4:], masked["input_ids"][3:])


def test_adapter_raw(torch):
    from packages.tokenizer_utils import dp_tokenize_llama
    tok = _llama_fixture()
    dp_tokenize, _ = dp_tokenize_llama(tok, "raw")
    _check_pair_adapter(torch, dp_tokenize, tok, SOURCES, TARGETS, OOV)
    with pytest.raises(IndexError):   # the empty string, as in ``batch``
        dp_tokenize.batch_pair_model_inputs(["a", "x"], ["y", ""])


def test_adapter_llama(torch):
    from packages.tokenizer_utils import dp_tokenize_llama
    tok = _llama_fixture()
    dp_tokenize, _ = dp_tokenize_llama(tok)   # default 'llama'
    _check_pair_adapter(torch, dp_tokenize, tok, SOURCES + [""], TARGETS + ["z"])


def test_adapter_bloom(torch, tmp_path):
    from bloom_fixture import bloom_tokenizer, make_hf_cache
    from packages.tokenizer_utils import dp_tokenize_bloom
    hf = make_hf_cache(str(tmp_path))
    tok = bloom_tokenizer(hf)
    dp_tokenize, _ = dp_tokenize_bloom(tok, hf)
    _check_pair_adapter(torch, dp_tokenize, tok, SOURCES + ["", "café 中文字 😀"], TARGETS + ["中文", ""])
    dp_device, _ = dp_tokenize_bloom(tok, hf, device_pretokenize=True)   # the words and atoms made on the device too
    out, host = dp_device.batch_pair_model_inputs(SOURCES, TARGETS), dp_tokenize.batch_pair_model_inputs(SOURCES, TARGETS)
    assert torch.equal(out["input_ids"], host["input_ids"]) and torch.equal(out["labels"], host["labels"])
