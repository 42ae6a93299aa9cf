"""Sequence packing on the device (include/dpt.h dpt_pack_sizes / dpt_pack_plan / dpt_pack_write) against
tests/packing_ref.py, for exact equality: the plan at the block edges the library reports, rows wider than blocks,
zero-length runs over whole blocks, one string per row, a row capacity under and over the need, a striding plan
launch, the rows under every flag combination on both store paths, a real encode on a side stream, and the Python
surface.  Every output sits between sentinel guards, asserted untouched."""
import itertools

import numpy as np
import pytest

import matrix_corpus as mc
import packing_ref as pr
from collate_harness import (BOS_ID, EOS_ID, GUARD, IGNORE, PAD_ID, SENT, TEXTS, Out, Side, _llama_fixture, assert_equal, random_batch)
from collate_harness import raw_reference as make_raw_reference
from collate_ref import BOS, EOS, I64, TRUNC_LEFT
from packing_ref import MASK_FIRST, random_lengths

pytestmark = pytest.mark.gpu

FIRST = 1000003   # tok_off[0]: the prefix sums need not start at 0


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def geometry():
    from dptok import packing
    return packing.pack_geometry()


def vec(torch, n, dtype=None, base=1):
    """n guarded elements (int32 unless given), ``base`` elements off the 16-byte boundary"""
    return Out(torch, 1, n, 0, dtype or torch.int32, base)


def u32(out):
    return out.rows()[0].view(np.uint32).astype(np.int64)


def want_plan(lengths, L, cap):
    """the plan's five outputs for ``row_cap = cap``, from the searchsorted chain"""
    n_str = len(lengths)
    str_row, str_col, starts, fills, n_rows = pr.plan_chain(lengths, L)
    row_first = np.concatenate([starts, np.full(cap + 1, n_str, dtype=np.int64)])[:cap + 1]
    row_fill = np.concatenate([fills, np.zeros(cap, dtype=np.int64)])[:cap]
    return str_row, str_col, row_first, row_fill, n_rows


def run_plan(torch, lengths, L, cap=None, null=(), check=True):
    """One dpt_pack_plan over the prefix sums of ``lengths`` (from FIRST on) with ``row_cap = cap`` (None: the need
    + 2) -> (str_row, str_col, row_first, row_fill, n_rows), compared with the chain."""
    from dptok import packing
    lengths = np.asarray(lengths, dtype=np.int64)
    n_str = len(lengths)
    want = want_plan(lengths, L, 0)[4] if cap is None else None
    cap = want + 2 if cap is None else cap
    tok_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]) + FIRST).cuda()
    outs = [None if k in null else vec(torch, n) for k, n in (("str_row", n_str), ("str_col", n_str), ("row_first", cap + 1), ("row_fill", cap))]
    n_rows = vec(torch, 1, torch.int64, 0)
    ws_bytes = packing.plan_workspace_bytes(n_str)
    ws = vec(torch, ws_bytes // 4, base=0)
    ptrs = [o.ptr() if o is not None else 0 for o in outs]
    packing.pack_plan_device(tok_off.data_ptr(), n_str, L, cap, n_rows.ptr(), ws.ptr() if n_str else 0, ws_bytes, str_row_ptr=ptrs[0],
                             str_col_ptr=ptrs[1], row_first_ptr=ptrs[2], row_fill_ptr=ptrs[3])
    torch.cuda.synchronize()
    ws.rows()   # (the guards around the workspace)
    got = [None if o is None else u32(o) for o in outs] + [int(n_rows.rows()[0][0])]
    if check:
        want = want_plan(lengths, L, cap)
        for k, (g, w) in enumerate(zip(got[:4], want[:4])):
            if g is not None:
                bad = np.flatnonzero(g != w)
                assert not len(bad), ("plan output %d" % k, n_str, L, cap, bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())
        assert got[4] == want[4], (n_str, L, cap)
    return got


# ------------------------------------------------------------------ 1. plan edges

@pytest.mark.parametrize("L", [1, 2, 7, 64, 2048])
def test_plan_edges(L, torch, geometry):
    B, _ = geometry
    rng = np.random.default_rng(L)
    for n_str in (0, 1, 2, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, 3 * B + 7):
        ln = random_lengths(rng, n_str, L)
        if n_str > 200:   # longer zero runs and a run of exact fills across a block edge
            ln[B // 2:B // 2 + 70] = 0
            ln[B - 3:B + 3] = L
        run_plan(torch, ln, L)
    assert run_plan(torch, [], L, cap=0)[4] == 0
    for only in (0, 1, L):
        got = run_plan(torch, [only], L)
        assert got[4] == (1 if only else 0)


# ------------------------------------------------------------------ 2. rows wider than blocks

@pytest.mark.parametrize("wide", [0, 1])
def test_rows_wider_than_blocks(wide, torch, geometry):
    B, _ = geometry
    L = 3 * B + 5 if wide else B
    n_str = 11 * B + 13
    rng = np.random.default_rng(5 + wide)
    ones = run_plan(torch, np.ones(n_str, dtype=np.int64), L)
    assert ones[4] == -(-n_str // L)
    starts = ones[2][:ones[4]]
    assert (np.diff(starts) == L).all()   # with L = 3B + 5 a row covers whole blocks no row starts in
    mixed = (rng.random(n_str) < 0.5).astype(np.int64)
    got = run_plan(torch, mixed, L)
    assert (np.diff(got[2][:got[4]]) >= L).all()
    if wide:
        blocks_with_start = set((got[2][:got[4]] // B).tolist())
        assert len(blocks_with_start) < n_str // B - 2   # entries skip whole blocks


# ------------------------------------------------------------------ 3. zero-length runs

@pytest.mark.parametrize("where", ["start", "middle", "end", "all"])
def test_zero_runs_over_whole_blocks(where, torch, geometry):
    B, _ = geometry
    L = 9
    rng = np.random.default_rng(17)
    n_str = 7 * B + 11
    ln = rng.integers(1, L + 1, size=n_str)
    run = 3 * B + 3   # covers at least two whole blocks wherever it begins
    a = {"start": 0, "middle": B + B // 3, "end": n_str - run, "all": 0}[where]
    ln[a:a + (n_str if where == "all" else run)] = 0
    got = run_plan(torch, ln, L)
    if where == "all":
        assert got[4] == 0 and (got[0] == pr.NONE).all() and (got[2] == n_str).all()
    else:
        empty_blocks = [b for b in range(n_str // B) if not ln[b * B:(b + 1) * B].any()]
        assert len(empty_blocks) >= 2
        assert (got[0][a:a + run] == pr.NONE).all() and (got[1][a:a + run] == 0).all()


# ------------------------------------------------------------------ 4. one string per row

@pytest.mark.parametrize("case", ["full", "alternate", "L1"])
def test_one_string_per_row(case, torch, geometry):
    B, _ = geometry
    n_str = 2 * B + 37
    L = 1 if case == "L1" else 12
    ln = np.full(n_str, L, dtype=np.int64)
    if case == "alternate":
        ln[1::2] = 1
    got = run_plan(torch, ln, L)
    assert got[4] == n_str and (got[0] == np.arange(n_str)).all() and (got[1] == 0).all()
    assert (got[2][:n_str] == np.arange(n_str)).all() and (got[3][:n_str] == ln).all()


# ------------------------------------------------------------------ 5. the row capacity

def test_row_cap_under_and_over_the_need(torch, geometry):
    B, _ = geometry
    L = 16
    rng = np.random.default_rng(23)
    ln = random_lengths(rng, 2 * B + 5, L)
    need = run_plan(torch, ln, L)[4]
    assert need > 40
    for cap in (0, 1, need // 2, need - 1, need, need + 1, need + B + 9):
        assert run_plan(torch, ln, L, cap=cap)[4] == need   # (the guards: nothing written past row_cap)
    for k in range(5):
        names = ("str_row", "str_col", "row_first", "row_fill")
        for null in itertools.combinations(names, k):
            run_plan(torch, ln[:B + 3], L, cap=need // 4, null=null)


# ------------------------------------------------------------------ 6. one striding plan call

def test_plan_strides_over_the_grid_cap(torch, geometry):
    B, grid_cap = geometry
    n_str = grid_cap * B + B + 1
    rng = np.random.default_rng(29)
    L = 512
    ln = rng.integers(0, 65, size=n_str)
    ln[rng.random(n_str) < 0.1] = 0
    ln[5 * B - 7:7 * B + 9] = 0
    ln[grid_cap * B - 2:grid_cap * B + 2] = L   # full rows across the edge of the second sweep
    got = run_plan(torch, ln, L)
    assert got[4] > n_str // 40


# ------------------------------------------------------------------ 7. the rows

ALL16 = [b | e | t | m for b in (0, BOS) for e in (0, EOS) for t in (0, TRUNC_LEFT) for m in (0, MASK_FIRST)]


def n_special(flags):
    return bool(flags & BOS) + bool(flags & EOS)


def make_want(ids, off, L, flags, counts, status, cap):
    lengths = pr.lengths_ref(off, counts, status, row_len=L, flags=flags)
    plan = want_plan(np.asarray(lengths), L, cap)
    rows = pr.rows_ref(np.asarray(ids).tolist(), [int(x) for x in off], None if counts is None else [int(x) for x in counts],
                       None if status is None else np.asarray(status).tolist(), row_len=L, row_cap=cap, pad_id=PAD_ID, bos_id=BOS_ID,
                       eos_id=EOS_ID, ignore_id=IGNORE, flags=flags)
    return lengths, plan, rows


def run_pack(torch, ids, off, L, flags, *, counts=None, status=None, stride=0, base=0, ids_shift=0, null=(), cap=None, extra=2,
             stream=0, want=None):
    """sizes -> cumsum -> plan -> write over host arrays (uploaded here), nothing read back in between -> the four row
    outputs as numpy (None when named in ``null``), all compared with packing_ref.  ``cap`` None: the need + ``extra``
    rows.  ``want``: make_want's result for these arguments, when the caller has it."""
    from dptok import packing
    n_str = len(off) - 1
    st = None if "status" in null else status
    dtype = torch.int64 if flags & I64 else torch.int32
    if want is None:
        need = pr.plan_chain(pr.lengths_ref(off, counts, st, row_len=L, flags=flags), L)[4]
        cap = need + extra if cap is None else cap
        want = make_want(ids, off, L, flags & ~I64, counts, st, cap)
    cap = len(want[1][3])
    src = Side(torch, ids, off, counts, st, shift=ids_shift)
    ids_ptr, off_ptr, counts_ptr, status_ptr = src.ptrs()
    kw = dict(bos_id=BOS_ID if flags & BOS else None, eos_id=EOS_ID if flags & EOS else None)
    o_len = vec(torch, n_str)
    packing.pack_sizes_device(off_ptr, n_str, o_len.ptr(), L, counts_ptr=counts_ptr, status_ptr=status_ptr, stream=stream, **kw)
    tok_off = torch.full((n_str + 1,), FIRST, dtype=torch.int64, device="cuda")
    d_len = o_len.whole[GUARD + 1:GUARD + 1 + n_str]
    tok_off[1:] += torch.cumsum(d_len, 0, dtype=torch.int64)
    row_first, row_fill, n_rows = vec(torch, cap + 1), vec(torch, cap), vec(torch, 1, torch.int64, 0)
    ws_bytes = packing.plan_workspace_bytes(n_str)
    ws = torch.empty(ws_bytes // 4 + 1, dtype=torch.int32, device="cuda")
    packing.pack_plan_device(tok_off.data_ptr(), n_str, L, cap, n_rows.ptr(), ws.data_ptr(), ws_bytes, row_first_ptr=row_first.ptr(),
                             row_fill_ptr=row_fill.ptr(), stream=stream)
    names = ("input_ids", "position_ids", "segment_ids", "labels")
    outs = [None if k in null else Out(torch, cap, L, stride, dtype, base) for k in names]
    ptrs = [o.ptr() if o is not None else 0 for o in outs]
    packing.pack_write_device((ids_ptr, off_ptr, counts_ptr, status_ptr), n_str, tok_off.data_ptr(), row_first.ptr(), n_rows.ptr(), cap,
                              ptrs[0], L, position_ids_ptr=ptrs[1], segment_ids_ptr=ptrs[2], labels_ptr=ptrs[3], row_stride=stride,
                              pad_id=PAD_ID, ignore_id=IGNORE, trunc_left=bool(flags & TRUNC_LEFT), int64=bool(flags & I64),
                              mask_first=bool(flags & MASK_FIRST), stream=stream, **kw)
    torch.cuda.synchronize()
    lengths, plan, rows = want
    what = (L, flags, stride, base, cap)
    assert u32(o_len).tolist() == lengths, what
    assert int(n_rows.rows()[0][0]) == plan[4] and u32(row_first).tolist() == plan[2].tolist() and u32(row_fill).tolist() == plan[3].tolist(), what
    got = tuple(o.rows() if o is not None else None for o in outs)
    assert_equal(got, rows, what)
    return got


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 129, 257])
def test_rows_every_flag_combination(L, torch):
    rng = np.random.default_rng(L)
    n = np.concatenate([np.arange(0, L + 9), [2 * L, 3 * L + 1, 0, 0, 1]])   # strings up to and over the room, of every flag set
    rng.shuffle(n)
    ids, off = random_batch(rng, n, first=77)
    room = n + rng.integers(0, 4, size=len(n))
    wide_ids, wide_off = random_batch(rng, room, first=5)
    ran = 0
    for flags in ALL16:
        if L < n_special(flags):
            continue
        for layout in ("csr", "counts"):
            a_ids, a_off, a_cnt = (ids, off, None) if layout == "csr" else (wide_ids, wide_off, n)
            want = None
            for width in (0, I64):
                need = pr.plan_chain(pr.lengths_ref(a_off, a_cnt, None, row_len=L, flags=flags), L)[4]
                want = want or make_want(a_ids, a_off, L, flags, a_cnt, None, need + 2)
                run_pack(torch, a_ids, a_off, L, flags | width, counts=a_cnt, want=want)
                ran += 1
    assert ran == (64 if L >= 2 else 48)   # (L = 1 has no room for BOS and EOS together)


@pytest.mark.parametrize("width", [0, I64])
@pytest.mark.parametrize("L", [8, 7])
def test_alignment(L, width, torch):
    rng = np.random.default_rng(100 + L)
    counts = rng.integers(0, 2 * L, size=301)
    ids, off = random_batch(rng, counts, first=123457)
    flags = BOS | EOS | MASK_FIRST | width
    want = make_want(ids, off, L, flags & ~I64, None, None, pr.plan_chain(pr.lengths_ref(off, row_len=L, flags=flags), L)[4] + 1)
    for base in (range(2) if width else range(4)):
        for stride in (0, L, L + 1, L + 3, L + 4):
            run_pack(torch, ids, off, L, flags, stride=stride, base=base, ids_shift=1, want=want)
    run_pack(torch, ids, off, L, TRUNC_LEFT | width, stride=L + 4, ids_shift=3)


@pytest.mark.parametrize("L", [8, 7])
def test_nullable_outputs_and_statuses(L, torch):
    rng = np.random.default_rng(7)
    n = 300
    counts = rng.integers(0, 2 * L, size=n)
    status = rng.choice([0, 0, 0, 1, 2, 3, 4], size=n).astype(np.int32)
    ids, off = random_batch(rng, counts)
    assert ((status != 0) & (counts > 0)).any()
    names = ("position_ids", "segment_ids", "labels", "status")
    for k in range(len(names) + 1):
        for null in itertools.combinations(names, k):
            for width in (0, I64):
                run_pack(torch, ids, off, L, EOS | width, status=status, null=null)
    # the counts layout: ranges longer than the counts, failed strings with a count and a range of their own
    room = counts + rng.integers(0, 5, size=n)
    wide_ids, wide_off = random_batch(rng, room, first=77)
    for flags in (EOS, BOS | TRUNC_LEFT | MASK_FIRST | I64):
        run_pack(torch, wide_ids, wide_off, L, flags, counts=counts, status=status)


def test_write_row_cap(torch):
    """row_cap under the need: the rows below it are written and nothing else (the guards); over it: the surplus rows
    are pad.  Long rows on both store paths, more units than one chunk."""
    rng = np.random.default_rng(31)
    for L in (2500, 2501):
        counts = rng.integers(0, 700, size=150)
        ids, off = random_batch(rng, counts)
        need = pr.plan_chain(pr.lengths_ref(off, row_len=L, flags=EOS), L)[4]
        assert need > 6
        for cap in (1, need - 1, need, need + 3):
            run_pack(torch, ids, off, L, EOS | I64, cap=cap)
    run_pack(torch, ids, off, 9, BOS, cap=0)


# ------------------------------------------------------------------ 8. behind a real encode, on a side stream

@pytest.fixture(scope="module")
def raw_reference():
    return make_raw_reference(("base",))


def test_encode_then_pack_on_a_side_stream(raw_reference, torch):
    from dptok import packing
    enc, ref_ids, ref_off, ref_st = raw_reference["base"]
    counts = np.diff(ref_off.astype(np.int64))
    L = 128
    assert (ref_st != 0).any() and (counts > L).any()
    text, offs, _ = mc.upload("raw")
    n, b0, n_bytes = len(offs) - 1, int(offs[0]), int(offs[-1] - offs[0])
    side = torch.cuda.Stream()
    h_text, h_offs = torch.from_numpy(text).pin_memory(), torch.from_numpy(offs.view(np.int64)).pin_memory()
    d_text = torch.empty(len(text), dtype=torch.uint8, device="cuda")
    d_offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ids = torch.full((n_bytes + 1,), SENT, dtype=torch.int32, device="cuda")
    id_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    lengths = torch.empty(n, dtype=torch.int32, device="cuda")
    tok_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    row_first = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    n_rows = torch.empty(1, dtype=torch.int64, device="cuda")
    ws_bytes = packing.plan_workspace_bytes(n)
    ws = torch.empty(ws_bytes // 4 + 1, dtype=torch.int32, device="cuda")
    outs = [Out(torch, n, L, 0, torch.int64) for _ in range(3)]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_text.copy_(h_text, non_blocking=True)
        d_offs.copy_(h_offs, non_blocking=True)
        sid = side.cuda_stream
        enc.encode_device(d_text.data_ptr() + b0, n_bytes, d_offs.data_ptr(), n, ids.data_ptr(), n_bytes, id_off.data_ptr(), st.data_ptr(),
                          stream=sid)
        # no host synchronisation from the encode to the rows
        packing.pack_sizes_device(id_off.data_ptr(), n, lengths.data_ptr(), L, status_ptr=st.data_ptr(), stream=sid)
        torch.cumsum(lengths, 0, dtype=torch.int64, out=tok_off[1:])
        packing.pack_plan_device(tok_off.data_ptr(), n, L, n, n_rows.data_ptr(), ws.data_ptr(), ws_bytes, row_first_ptr=row_first.data_ptr(),
                                 stream=sid)
        packing.pack_write_device((ids.data_ptr(), id_off.data_ptr(), 0, st.data_ptr()), n, tok_off.data_ptr(), row_first.data_ptr(),
                                  n_rows.data_ptr(), n, outs[0].ptr(), L, position_ids_ptr=outs[1].ptr(), segment_ids_ptr=outs[2].ptr(),
                                  pad_id=PAD_ID, stream=sid)
    side.synchronize()
    assert np.array_equal(st.cpu().numpy(), ref_st)
    rows, pos, seg = (o.rows() for o in outs)
    need = int(n_rows.item())
    want_len = np.where(ref_st != 0, 0, np.minimum(counts, L))
    assert need == pr.plan_chain(want_len, L)[4] and 0 < need < n
    assert (seg[need:] == 0).all() and (rows[need:] == PAD_ID).all()
    # unpacking the rows by segment gives back every string's ids, in order
    live = seg != 0
    placed = np.flatnonzero(want_len)
    o0 = int(ref_off[0])
    flat = np.concatenate([ref_ids[int(ref_off[s]) - o0:int(ref_off[s]) - o0 + int(want_len[s])] for s in placed])
    assert np.array_equal(rows[live], flat)
    key = (np.arange(n)[:, None] * (n + 2) + seg)[live]   # (row, segment), increasing along the flattened rows
    edges = np.flatnonzero(np.diff(key)) + 1
    assert np.array_equal(np.diff(np.concatenate([[0], edges, [len(key)]])), want_len[placed])
    assert np.array_equal(pos[live], np.concatenate([np.arange(k) for k in want_len[placed]]))


# ------------------------------------------------------------------ 9. the Python surface and the adapters

def test_packed_inputs_and_plan_lengths(torch):
    from dptok import packing
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 40, size=60)
    ids, off = random_batch(rng, counts)
    status = np.zeros(60, dtype=np.int32)
    status[[3, 7]] = 1
    d_ids, d_off, d_st = torch.from_numpy(ids).cuda(), torch.from_numpy(off.view(np.int64)).cuda(), torch.from_numpy(status).cuda()
    L = 48
    for rows, int64 in ((None, True), (100, False), (3, True)):
        out = packing.packed_inputs(d_ids, d_off, d_st, max_length=L, rows=rows, labels=True, mask_first=True, eos_id=EOS_ID, pad_id=PAD_ID,
                                    int64=int64)
        lengths = pr.lengths_ref(off, None, status, row_len=L, flags=EOS)
        need = pr.plan_loop(lengths, L)[4]
        cap = need if rows is None else rows
        str_row, str_col, row_first, row_fill, _ = pr.plan_loop(lengths, L, row_cap=cap)
        want = pr.rows_ref(ids.tolist(), off.tolist(), None, status.tolist(), row_len=L, row_cap=cap, pad_id=PAD_ID, eos_id=EOS_ID,
                           ignore_id=IGNORE, flags=EOS | MASK_FIRST)
        assert (out["n_rows"] == need if rows is None else int(out["n_rows"]) == need and out["n_rows"].is_cuda)
        for k in ("input_ids", "position_ids", "segment_ids", "labels"):
            assert out[k].shape == (cap, L) and out[k].dtype == (torch.int64 if int64 else torch.int32) and out[k].is_cuda
        assert_equal(tuple(out[k].cpu().numpy() for k in ("input_ids", "position_ids", "segment_ids", "labels")), want, rows)
        assert out["lengths"].cpu().tolist() == lengths
        assert (out["str_row"].cpu().numpy().view(np.uint32) == np.array(str_row)).all() and out["str_col"].cpu().tolist() == str_col
        assert out["row_first"].cpu().tolist() == row_first and out["row_fill"].cpu().tolist() == row_fill
    few = packing.packed_inputs(d_ids, d_off, max_length=L, position_ids=False, segment_ids=False)
    assert set(few) == {"input_ids", "lengths", "str_row", "str_col", "row_first", "row_fill", "n_rows"}
    empty = packing.packed_inputs(d_ids[:0], d_off[:1], max_length=8, rows=2, labels=True)
    assert empty["input_ids"].shape == (2, 8) and int(empty["n_rows"]) == 0 and (empty["labels"] == -100).all()
    assert packing.packed_inputs(d_ids[:0], d_off[:1], max_length=8)["input_ids"].shape == (0, 8)
    with pytest.raises(ValueError, match="max_length"):
        packing.packed_inputs(d_ids, d_off, max_length=1, bos_id=1, eos_id=2)
    # plan_lengths: any integer lengths
    ln = rng.integers(0, 10, size=500)
    for dtype in (torch.int32, torch.int64):
        plan = packing.plan_lengths(torch.from_numpy(ln).to("cuda", dtype), 9)
        want = pr.plan_loop(ln.tolist(), 9)
        assert plan["n_rows"] == want[4] and plan["row_fill"].cpu().tolist() == want[3] and plan["row_first"].cpu().tolist() == want[2]
        assert (plan["str_row"].cpu().numpy().view(np.uint32) == np.array(want[0])).all()
    assert packing.plan_lengths(torch.zeros(0, dtype=torch.int32, device="cuda"), 4)["n_rows"] == 0


def _check_adapter(torch, dp_tokenize, tokenizer, texts):
    from packages.tokenizer_utils import _special_ids
    lists = dp_tokenize.batch(texts)
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).tolist()
    flat = [i for x in lists for i in x]
    bos, eos, pad = _special_ids(tokenizer)
    cases = [(dict(max_length=16), 0, 16), (dict(max_length=6, labels=True, mask_first=True, truncation_side="left"), TRUNC_LEFT | MASK_FIRST, 6)]
    if eos is not None:
        cases.append((dict(max_length=9, add_eos=True, labels=True), EOS, 9))
    if bos is not None:
        cases.append((dict(max_length=12, add_bos=True), BOS, 12))
    for kw, flags, L in cases:
        out = dp_tokenize.batch_packed_inputs(texts, **kw)
        want = pr.rows_ref(flat, off, row_len=L, pad_id=pad, bos_id=bos or 0, eos_id=eos or 0, flags=flags)
        assert out["input_ids"].is_cuda and out["input_ids"].dtype == torch.int64 and "status" not in out
        assert out["n_rows"] == len(want[0]) and ("labels" in out) == bool(kw.get("labels"))
        got = tuple(out[k].cpu().numpy() if k in out else None for k in ("input_ids", "position_ids", "segment_ids", "labels"))
        assert_equal(got, want, kw)
        # every sequence lies at str_row * L + str_col of the flattened rows, lengths[s] long (cu_seqlens)
        placed = out["str_row"] >= 0
        begin = (out["str_row"].long() * L + out["str_col"])[placed]
        length = out["lengths"].long()[placed]
        pos = out["position_ids"].reshape(-1)
        assert (pos[begin] == 0).all() and (pos[begin + length - 1] == length - 1).all()
        assert (begin[1:] >= (begin + length)[:-1]).all() and int(length.sum()) == int((out["segment_ids"] != 0).sum())
    masked = dp_tokenize.batch_packed_inputs(texts, max_length=16, errors="mask")
    assert masked["status"].dtype == torch.int32 and not masked["status"].any()
    with pytest.raises(ValueError, match="errors"):
        dp_tokenize.batch_packed_inputs(texts, max_length=16, errors="ignore")
    return masked


def test_adapter_raw_and_llama(torch):
    from collate_harness import OOV
    from packages.tokenizer_utils import dp_tokenize_llama
    tok = _llama_fixture()
    dp_tokenize, _ = dp_tokenize_llama(tok)   # default 'llama'
    _check_adapter(torch, dp_tokenize, tok, TEXTS + [""])
    raw, _ = dp_tokenize_llama(tok, "raw")
    masked = _check_adapter(torch, raw, tok, TEXTS)
    # an untokenizable word: the exception of ``batch``, or an unplaced string and its status
    mixed = list(TEXTS[:2]) + [OOV] + list(TEXTS[2:])
    with pytest.raises(ValueError) as e_batch:
        raw.batch(mixed)
    with pytest.raises(ValueError) as e_packed:
        raw.batch_packed_inputs(mixed, max_length=16)
    assert str(e_packed.value) == str(e_batch.value)
    out = raw.batch_packed_inputs(mixed, max_length=16, errors="mask")
    assert out["status"].cpu().tolist() == [0, 0, 1] + [0] * (len(TEXTS) - 2)
    assert int(out["str_row"][2]) == -1 and int(out["lengths"][2]) == 0
    assert torch.equal(out["input_ids"], masked["input_ids"]) and out["n_rows"] == masked["n_rows"]
    # (a failed string still counts in the segment numbers of the strings after it in its row)
    keep = [0, 1] + list(range(3, len(mixed)))
    assert torch.equal(out["str_row"][keep], masked["str_row"]) and torch.equal(out["str_col"][keep], masked["str_col"])


def test_adapter_bloom_and_compare_rows(torch, tmp_path):
    from bloom_fixture import bloom_texts, bloom_tokenizer, make_hf_cache
    from packages.tokenizer_utils import dp_tokenize_bloom
    hf = make_hf_cache(str(tmp_path))
    tok = bloom_tokenizer(hf)
    dp_tokenize, _ = dp_tokenize_bloom(tok, hf, device_pretokenize=True)
    _check_adapter(torch, dp_tokenize, tok, TEXTS + ["", "café 中文字 😀"])
    assert dp_tokenize.pretok_stats.default_off is None, dp_tokenize.pretok_stats.default_off
    texts = bloom_texts()[:150]
    plain = dp_tokenize.batch_compare(texts)
    assert "dp_rows" not in plain and "default_rows" not in plain
    for L in (8, 64):
        c = dp_tokenize.batch_compare(texts, pack_length=L)
        assert set(c) == set(plain) | {"dp_rows", "default_rows"}
        for key, lens in (("dp_rows", c["dp_lengths"]), ("default_rows", c["default_lengths"])):
            assert c[key] == pr.plan_loop(np.minimum(lens, L).tolist(), L)[4] > 0
        assert all(np.array_equal(c[k], plain[k]) for k in ("dp_lengths", "default_lengths", "improved"))
