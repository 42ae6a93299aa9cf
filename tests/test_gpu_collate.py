"""dpt_collate on the device (include/dpt.h) against tests/collate_ref.py, for exact equality: row edges under
every flag combination, both store paths at every output alignment, nullable arguments, failed strings, the
shape extremes, both source layouts behind a real encode on a side stream, and the Python surface.  Every
output sits between sentinel guards (and has sentinels in its [row_len, row_stride) gaps), asserted untouched."""
import itertools

import numpy as np
import pytest

import matrix_corpus as mc
from collate_harness import (BOS_ID, EOS_ID, IGNORE, OOV, PAD_ID, SENT, TEXTS, Out, Side, _llama_fixture, as_numpy, assert_equal,
                             random_batch)
from collate_harness import raw_reference as make_raw_reference
from collate_ref import BOS, EOS, I64, PAD_LEFT, TRUNC_LEFT, collate_ref

pytestmark = pytest.mark.gpu

ALL16 = [b | e | p | t for b in (0, BOS) for e in (0, EOS) for p in (0, PAD_LEFT) for t in (0, TRUNC_LEFT)]


def n_special(flags):
    return bool(flags & BOS) + bool(flags & EOS)


def run_collate(torch, ids, off, L, flags, *, counts=None, status=None, stride=0, base=0, ids_shift=0,
                null=(), stream=0, check=True):
    """One dpt_collate call over host arrays (uploaded here) -> (input_ids, mask, labels, lengths) as numpy, each
    None when named in ``null``; with ``check`` they are compared with collate_ref."""
    from dptok import collate
    n_str = len(off) - 1
    dtype = torch.int64 if flags & I64 else torch.int32
    src = Side(torch, ids, off, counts, None if "status" in null else status, shift=ids_shift)
    ids_ptr, off_ptr, counts_ptr, status_ptr = src.ptrs()
    o_ids = Out(torch, n_str, L, stride, dtype, base)
    o_mask = None if "mask" in null else Out(torch, n_str, L, stride, dtype, base)
    o_lab = None if "labels" in null else Out(torch, n_str, L, stride, dtype, base)
    o_len = None if "lengths" in null else Out(torch, 1, n_str, 0, torch.int32, 1)
    collate.collate_device(ids_ptr, off_ptr, n_str, o_ids.ptr(), L, counts_ptr=counts_ptr, status_ptr=status_ptr,
                           mask_ptr=o_mask.ptr() if o_mask else 0, labels_ptr=o_lab.ptr() if o_lab else 0,
                           lengths_ptr=o_len.ptr() if o_len else 0, row_stride=stride, pad_id=PAD_ID,
                           bos_id=BOS_ID if flags & BOS else None, eos_id=EOS_ID if flags & EOS else None, ignore_id=IGNORE,
                           pad_left=bool(flags & PAD_LEFT), trunc_left=bool(flags & TRUNC_LEFT), int64=bool(flags & I64),
                           stream=stream)
    torch.cuda.synchronize()
    got = (o_ids.rows(), o_mask.rows() if o_mask else None, o_lab.rows() if o_lab else None,
           o_len.rows()[0] if o_len else None)
    if check:
        want = collate_ref(np.asarray(ids).tolist(), [int(x) for x in off], None if counts is None else [int(x) for x in counts],
                           None if src.d_st is None else np.asarray(status).tolist(), row_len=L, pad_id=PAD_ID, bos_id=BOS_ID, eos_id=EOS_ID,
                           ignore_id=IGNORE, flags=flags)
        assert_equal(got, want, (L, flags, stride, base))
    return got


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ------------------------------------------------------------------ 1. row edges

@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257])
def test_row_edges(L, torch):
    rng = np.random.default_rng(L)
    ids, off = random_batch(rng, np.arange(0, L + 71))
    ran = 0
    for flags, width in itertools.product(ALL16, (0, I64)):
        if L < n_special(flags):
            continue
        run_collate(torch, ids, off, L, flags | width)
        ran += 1
    assert ran == (32 if L >= 2 else 24)   # (L = 1 has no room for BOS and EOS together)


def test_row_shorter_than_its_specials_is_an_argument_error(torch):
    from dptok import DptError, collate
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    before = buf.clone()
    with pytest.raises(DptError, match="row_len"):
        collate.collate_device(buf.data_ptr(), buf.data_ptr(), 1, buf.data_ptr() + 256, 1, bos_id=1, eos_id=2)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


# ------------------------------------------------------------------ 2. alignment, both store paths

@pytest.mark.parametrize("width", [0, I64])
@pytest.mark.parametrize("L", [8, 7])
def test_alignment(L, width, torch):
    rng = np.random.default_rng(100 + L)
    counts = rng.integers(0, 2 * L, size=301)
    ids, off = random_batch(rng, counts, first=123457)   # a shard of a larger CSR array, not rebased
    flags = BOS | EOS | width
    for base in (range(2) if width else range(4)):
        for stride in (0, L, L + 1, L + 3, L + 4):
            run_collate(torch, ids, off, L, flags, stride=stride, base=base, ids_shift=1)
    run_collate(torch, ids, off, L, PAD_LEFT | TRUNC_LEFT | width, stride=L + 4, ids_shift=3)


# ------------------------------------------------------------------ 3. nullable arguments

@pytest.mark.parametrize("L", [8, 7])
def test_nullable_arguments(L, torch):
    rng = np.random.default_rng(7)
    counts = rng.integers(0, 2 * L, size=200)
    ids, off = random_batch(rng, counts)
    status = np.where(rng.random(200) < 0.2, 1, 0).astype(np.int32)
    names = ("mask", "labels", "lengths", "status")
    for k in range(len(names) + 1):
        for null in itertools.combinations(names, k):
            for width in (0, I64):
                run_collate(torch, ids, off, L, EOS | width, status=status, null=null)


# ------------------------------------------------------------------ 4. statuses

@pytest.mark.parametrize("L", [12, 13])
def test_statuses(L, torch):
    rng = np.random.default_rng(11)
    n = 400
    counts = rng.integers(0, 2 * L, size=n)
    status = rng.choice([0, 0, 0, 1, 2, 3, 4], size=n).astype(np.int32)
    assert set(status.tolist()) == {0, 1, 2, 3, 4}
    # CSR: failed strings keep a non-empty range; it is not read
    ids, off = random_batch(rng, counts)
    assert ((status != 0) & (counts > 0)).any()
    for flags in (0, BOS | EOS | PAD_LEFT | TRUNC_LEFT | I64):
        run_collate(torch, ids, off, L, flags, status=status)
    # counts layout: ids at the strings' byte offsets (ranges longer than the counts), failed strings with a
    # non-zero count and a non-empty range
    room = counts + rng.integers(0, 5, size=n)
    ids, off = random_batch(rng, room, first=77)
    for flags in (EOS, BOS | PAD_LEFT | TRUNC_LEFT | I64):
        run_collate(torch, ids, off, L, flags, counts=counts, status=status)


# ------------------------------------------------------------------ 5. shape extremes

@pytest.mark.parametrize("L,flags", [(3, BOS), (3, I64 | EOS), (61, TRUNC_LEFT), (80, I64 | BOS | PAD_LEFT)])
def test_many_rows(L, flags, torch):
    """70 001 rows: more rows than one grid dimension holds blocks; with 61 (element path) and 80 int64 (16-byte
    path: 40 units) elements per row also more units than one sweep of the capped grid (the resident blocks,
    1280 on the MI355X, x 2048 units), so the blocks stride."""
    rng = np.random.default_rng(L)
    n = 70001
    counts = rng.integers(0, 2 * L, size=n)
    ids, off = random_batch(rng, counts)
    status = (rng.random(n) < 0.01).astype(np.int32) * 3
    run_collate(torch, ids, off, L, flags, status=status, null=("labels",))


@pytest.mark.parametrize("L,flags", [(100003, BOS | EOS), (100003, I64 | PAD_LEFT | TRUNC_LEFT | EOS), (100004, TRUNC_LEFT | BOS),
                                     (100004, I64)])
def test_long_rows(L, flags, torch):
    rng = np.random.default_rng(5)
    ids, off = random_batch(rng, np.array([0, 99999, 250000]))
    run_collate(torch, ids, off, L, flags)


# ------------------------------------------------------------------ 6. both source layouts behind an encode

@pytest.fixture(scope="module")
def raw_reference():
    """vocab -> (Encoder, ids, id_off, status) of the RAW corpus through the host path, computed once."""
    return make_raw_reference(("base", "long+40000"))


@pytest.mark.parametrize("vocab", ["base", "long+40000"])
def test_encode_then_collate_both_layouts(vocab, raw_reference, torch):
    from dptok import collate
    enc, ref_ids, ref_off, ref_st = raw_reference[vocab]
    counts = np.diff(ref_off.astype(np.int64))
    longest = int(counts.max())
    assert longest > 4000 and (ref_st != 0).any() and (counts > 128 - 2).any()   # failed and truncated strings
    text, offs, _ = mc.upload("raw")
    n, b0, n_bytes = len(offs) - 1, int(offs[0]), int(offs[-1] - offs[0])
    side = torch.cuda.Stream()
    h_text, h_offs = torch.from_numpy(text).pin_memory(), torch.from_numpy(offs.view(np.int64)).pin_memory()
    d_text = torch.empty(len(text), dtype=torch.uint8, device="cuda")
    d_offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    flags = BOS | EOS | I64
    for L in (128, longest):
        want = collate_ref(ref_ids.tolist(), ref_off.tolist(), None, ref_st.tolist(), row_len=L, pad_id=PAD_ID, bos_id=BOS_ID,
                           eos_id=EOS_ID, ignore_id=IGNORE, flags=flags)
        results = []
        for padded in (False, True):
            ids = torch.full((n_bytes + 1,), SENT, dtype=torch.int32, device="cuda")
            aux = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")   # id_off or counts
            st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            outs = [Out(torch, n, L, 0, torch.int64) for _ in range(3)]
            lens = Out(torch, 1, n, 0, torch.int32)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                d_text.copy_(h_text, non_blocking=True)
                d_offs.copy_(h_offs, non_blocking=True)
                sid = side.cuda_stream
                call = enc.encode_device_padded if padded else enc.encode_device
                call(d_text.data_ptr() + b0, n_bytes, d_offs.data_ptr(), n, ids.data_ptr(), n_bytes, aux.data_ptr(),
                     st.data_ptr(), stream=sid)
                # no host synchronisation between the encode and the collate
                collate.collate_device(ids.data_ptr(), d_offs.data_ptr() if padded else aux.data_ptr(), n, outs[0].ptr(), L,
                                       counts_ptr=aux.data_ptr() if padded else 0, status_ptr=st.data_ptr(),
                                       mask_ptr=outs[1].ptr(), labels_ptr=outs[2].ptr(), lengths_ptr=lens.ptr(),
                                       pad_id=PAD_ID, bos_id=BOS_ID, eos_id=EOS_ID, ignore_id=IGNORE, stream=sid)
            side.synchronize()
            got = (outs[0].rows(), outs[1].rows(), outs[2].rows(), lens.rows()[0])
            assert np.array_equal(st.cpu().numpy(), ref_st)
            assert_equal(got, want, (vocab, L, "padded" if padded else "csr"))
            results.append(got)
        for a, b in zip(*results):
            assert np.array_equal(a, b)


# ------------------------------------------------------------------ 7. the Python surface

def test_model_inputs(torch):
    from dptok import collate
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 40, size=50)
    counts[7] = 43
    ids, off = random_batch(rng, counts)
    status = np.zeros(50, dtype=np.int32)
    status[[3, 7]] = 1   # the longest string failed: it does not set the row length
    longest_ok = int(counts[status == 0].max())
    d_ids, d_off = torch.from_numpy(ids).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
    d_st = torch.from_numpy(status).cuda()
    cases = [(dict(padding="longest"), longest_ok + 1), (dict(padding="longest", max_length=16), 16),
             (dict(padding="longest", pad_to_multiple_of=8), -(-(longest_ok + 1) // 8) * 8),
             (dict(padding="max_length", max_length=64), 64), (dict(padding="max_length", max_length=13, pad_to_multiple_of=8), 16)]
    for kw, L in cases:
        for int64, lab in ((True, True), (False, False)):
            out = collate.model_inputs(d_ids, d_off, d_st, eos_id=EOS_ID, pad_id=PAD_ID, labels=lab, int64=int64, **kw)
            assert set(out) == {"input_ids", "attention_mask", "lengths"} | ({"labels"} if lab else set())
            for k in ("input_ids", "attention_mask") + (("labels",) if lab else ()):
                assert out[k].shape == (50, L) and out[k].dtype == (torch.int64 if int64 else torch.int32) and out[k].is_cuda
            assert out["lengths"].shape == (50,) and out["lengths"].dtype == torch.int32
            want = collate_ref(ids.tolist(), off.tolist(), None, status.tolist(), row_len=L, pad_id=PAD_ID, eos_id=EOS_ID,
                               ignore_id=IGNORE, flags=EOS | (I64 if int64 else 0))
            got = (out["input_ids"].cpu().numpy(), out["attention_mask"].cpu().numpy(),
                   out["labels"].cpu().numpy() if lab else None, out["lengths"].cpu().numpy())
            assert_equal(got, want, kw)
    # the counts layout, left sides, and an empty batch
    cnt = torch.from_numpy(counts.astype(np.int64)).cuda()
    room = np.concatenate([[0], np.cumsum(counts + 2)]).astype(np.int64)
    wide_ids = rng.integers(0, 50000, size=int(room[-1])).astype(np.int32)
    out = collate.model_inputs(torch.from_numpy(wide_ids).cuda(), torch.from_numpy(room).cuda(), d_st, cnt, bos_id=BOS_ID,
                               padding_side="left", truncation_side="left", max_length=20)
    want = collate_ref(wide_ids.tolist(), room.tolist(), counts.tolist(), status.tolist(), row_len=20, bos_id=BOS_ID,
                       flags=BOS | PAD_LEFT | TRUNC_LEFT | I64)
    assert_equal((out["input_ids"].cpu().numpy(), out["attention_mask"].cpu().numpy(), None, out["lengths"].cpu().numpy()),
                 want, "counts")
    empty = collate.model_inputs(d_ids[:0], d_off[:1], padding="longest", pad_to_multiple_of=8)
    assert empty["input_ids"].shape == (0, 8) and empty["lengths"].shape == (0,)


def _as_numpy(out):
    return as_numpy(out, ("input_ids", "attention_mask", "labels", "lengths"))


def _check_adapter(torch, dp_tokenize, tokenizer, texts, bad_text=None):
    """batch_model_inputs against collate_ref over the lists ``batch`` returns; ``bad_text``: a text with an
    untokenizable word (raw mode only: the llama fixture falls back to byte pieces and BLOOM's atoms are bytes of
    its alphabet, so every word of theirs has a tokenization)."""
    from packages.tokenizer_utils import _special_ids
    lists = dp_tokenize.batch(texts)
    longest = max(len(x) for x in lists)
    assert longest > 6 >= min(len(x) for x in lists)   # max_length = 6 truncates some and pads others
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).tolist()
    flat = [i for x in lists for i in x]
    bos, eos, pad = _special_ids(tokenizer)
    cases = [(dict(), 0, longest), (dict(max_length=6, padding="max_length", labels=True), 0, 6),
             (dict(max_length=6, padding_side="left", truncation_side="left", pad_to_multiple_of=4), PAD_LEFT | TRUNC_LEFT, 8)]
    if bos is not None:
        cases.append((dict(pad_to_multiple_of=8, add_bos=True), BOS, -(-(longest + 1) // 8) * 8))
    else:
        with pytest.raises(ValueError, match="BOS"):
            dp_tokenize.batch_model_inputs(texts, add_bos=True)
    if eos is not None:
        cases.append((dict(max_length=5, add_eos=True, labels=True), EOS, 5))
    else:
        with pytest.raises(ValueError, match="EOS"):
            dp_tokenize.batch_model_inputs(texts, add_eos=True)
    for kw, flags, L in cases:
        out = dp_tokenize.batch_model_inputs(texts, **kw)
        want = collate_ref(flat, off, row_len=L, pad_id=pad, bos_id=bos or 0, eos_id=eos or 0, flags=flags | I64)
        assert out["input_ids"].is_cuda and out["input_ids"].dtype == torch.int64 and "status" not in out
        assert out["input_ids"].shape == (len(texts), L) and ("labels" in out) == bool(kw.get("labels"))
        assert_equal(_as_numpy(out), want, kw)
    masked = dp_tokenize.batch_model_inputs(texts, errors="mask", max_length=6, padding="max_length")
    assert masked["status"].dtype == torch.int32 and not masked["status"].any()
    if bad_text is None:
        return
    # an untokenizable word: the exception of ``batch``, or the pad row and its status
    mixed = list(texts[:2]) + [bad_text] + list(texts[2:])
    with pytest.raises(Exception) as e_batch:
        dp_tokenize.batch(mixed)
    with pytest.raises(type(e_batch.value)) as e_inputs:
        dp_tokenize.batch_model_inputs(mixed)
    assert type(e_batch.value) is ValueError and str(e_inputs.value) == str(e_batch.value)
    out = dp_tokenize.batch_model_inputs(mixed, errors="mask", max_length=6, padding="max_length")
    assert out["status"].cpu().tolist() == [0, 0, 1] + [0] * (len(texts) - 2)
    assert (out["input_ids"][2] == pad).all() and not out["attention_mask"][2].any() and int(out["lengths"][2]) == 0
    keep = [0, 1] + list(range(3, len(mixed)))
    assert torch.equal(out["input_ids"][keep], masked["input_ids"]) and torch.equal(out["attention_mask"][keep], masked["attention_mask"])


def test_adapter_raw(torch):
    from packages.tokenizer_utils import dp_tokenize_llama
    tok = _llama_fixture()
    dp_tokenize, _ = dp_tokenize_llama(tok, "raw")
    _check_adapter(torch, dp_tokenize, tok, TEXTS, OOV)
    with pytest.raises(IndexError):   # the empty string, as in ``batch``
        dp_tokenize.batch_model_inputs(["a", ""])


def test_adapter_llama(torch):
    from packages.tokenizer_utils import dp_tokenize_llama
    tok = _llama_fixture()
    dp_tokenize, _ = dp_tokenize_llama(tok)   # default 'llama'
    _check_adapter(torch, dp_tokenize, tok, TEXTS + [""])
    assert dp_tokenize.batch([OOV])   # (byte pieces: no llama-mode word is untokenizable)


def test_adapter_bloom(torch, tmp_path):
    from bloom_fixture import bloom_tokenizer, make_hf_cache
    from packages.tokenizer_utils import dp_tokenize_bloom
    hf = make_hf_cache(str(tmp_path))
    tok = bloom_tokenizer(hf)
    dp_tokenize, _ = dp_tokenize_bloom(tok, hf)
    _check_adapter(torch, dp_tokenize, tok, TEXTS + ["", "café 中文字 😀"])
