#!/usr/bin/env python3
"""Time of dpt_collate_pair on one encoded batch of source + target pairs, device path, against torch ops and
against dpt_collate.

Default: 1M pairs, sources and targets cfg2-shaped at half length each (2M x 128-byte random printable ASCII strings,
the first million the sources, the second the targets; the synthetic 32k vocabulary, raw mode), encoded by ONE
dpt_encode_padded of all 2M strings: side B is the same buffers from string n on.  Everything runs on the same device
buffers in one process; each figure is a HIP event pair around `reps` back-to-back calls after warm-up, the repetitions
chosen so that each timed section lasts at least --min-seconds.  The row length is the longest pair's ids rounded up to
8 (nothing is truncated); the products are int64 input_ids + labels (ignore_id -100).  Timed in the same session:

  pair_ms      dpt_collate_pair alone, from the padded encode's layout
  torch_ms     the same two tensors from the same buffers with torch ops alone, what a user would otherwise write: a
               position grid against the two counts, one gather of the ids through a where of the two bases, the pad
               fill and cast, and a where for the labels
  single_ms    the yardstick: dpt_collate on ONE batch with the same rows -- the CSR arrays of the concatenated pairs
               (made here from the pair call's own output), so the same output bytes and the same id count
and the ratios torch_over_pair and pair_over_single.  The three products are checked for equality once.

--tag names the record in --out (default "default"): with DPT_LIB pointing at a variant library
(make variant VSRC=dpt_collate.hip V=pu4 DEFS=-DDPT_COLLATE_PAIR_UNITS=4) two runs record both knob values:

    python tools/collate_pair_bench.py --out profiles/collate_pair_bench.json
    DPT_LIB=.../var_pu4/libdpt.so python tools/collate_pair_bench.py --out profiles/collate_pair_bench.json --tag units4
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dp-tokenization_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=256, help="bytes of a source and its target together")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--hbm-gbs", type=float, default=6290.0)
    ap.add_argument("--tag", default="default")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from dptok import Encoder, Vocab, _lib, collate, synth

    n, half = args.pairs, args.length // 2
    text, offs = synth.random_ascii_corpus(2 * n, half, seed=args.seed)
    n_bytes = int(offs[-1])
    enc = Encoder(Vocab(synth.llama_shaped_vocab(), 0))
    dev = "cuda"
    d_text = torch.from_numpy(text).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    ids = torch.empty(n_bytes, dtype=torch.int32, device=dev)
    counts = torch.empty(2 * n, dtype=torch.int64, device=dev)
    st = torch.empty(2 * n, dtype=torch.int32, device=dev)
    enc.reserve(n_bytes, 2 * n)
    stream = torch.cuda.current_stream().cuda_stream
    enc.encode_device_padded(d_text.data_ptr(), n_bytes, d_off.data_ptr(), 2 * n, ids.data_ptr(), n_bytes, counts.data_ptr(),
                             st.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    del d_text

    def timed(fn):
        """ms per call: warm up, size the repetitions from a first timed run, then time them."""
        for _ in range(args.warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 1
        while True:
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= args.min_seconds * 1e3:
                return ms / reps
            reps = max(reps * 2, int(reps * args.min_seconds * 1.2e3 / max(ms, 1e-3)) + 1)

    ok = (st[:n] == 0) & (st[n:] == 0)
    na, nb = counts[:n].masked_fill(~ok, 0), counts[n:].masked_fill(~ok, 0)
    n_tok = int((na + nb).sum())
    longest = int((na + nb).max())
    L = -(-longest // 8) * 8
    pad_id, ignore = 0, -100
    first_b = int(offs[n])
    side_a = (ids.data_ptr(), d_off.data_ptr(), counts.data_ptr(), st.data_ptr())
    side_b = (ids.data_ptr() + 4 * first_b, d_off.data_ptr() + 8 * n, counts.data_ptr() + 8 * n, st.data_ptr() + 4 * n)
    rows = [torch.empty((n, L), dtype=torch.int64, device=dev) for _ in range(2)]

    def pair():
        collate.collate_pair_device(side_a, side_b, n, rows[0].data_ptr(), L, labels_ptr=rows[1].data_ptr(), pad_id=pad_id,
                                    ignore_id=ignore, stream=stream)

    ar = torch.arange(L, device=dev)
    base_a, base_b = d_off[:n], d_off[n:2 * n]

    def torch_ops():
        in_a = ar[None, :] < na[:, None]
        in_seq = ar[None, :] < (na + nb)[:, None]
        idx = torch.where(in_a, base_a[:, None] + ar[None, :], (base_b - na)[:, None] + ar[None, :])
        inp = torch.where(in_seq, ids[idx.clamp_(0, n_bytes - 1)].to(torch.int64), pad_id)
        return inp, torch.where(in_seq, inp, ignore)

    # the yardstick's batch: the concatenated pairs as one CSR batch (the same rows, so the same ids and bytes)
    probe = torch.empty((n, L), dtype=torch.int32, device=dev)
    mask = torch.empty((n, L), dtype=torch.int32, device=dev)
    collate.collate_pair_device(side_a, side_b, n, probe.data_ptr(), L, mask_ptr=mask.data_ptr(), pad_id=pad_id, int64=False,
                                stream=stream)
    one_ids = probe[mask.bool()].contiguous()
    one_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    one_off[1:] = mask.sum(1).cumsum(0)
    assert int(one_off[-1]) == n_tok == one_ids.numel()
    del probe, mask
    rows1 = [torch.empty((n, L), dtype=torch.int64, device=dev) for _ in range(2)]

    def single():
        collate.collate_device(one_ids.data_ptr(), one_off.data_ptr(), n, rows1[0].data_ptr(), L, labels_ptr=rows1[1].data_ptr(),
                               pad_id=pad_id, ignore_id=ignore, stream=stream)

    # equality, once
    for r in rows + rows1:
        r.fill_(-1)
    pair()
    single()
    want = torch_ops()
    for got, one, w in zip(rows, rows1, want):
        assert torch.equal(got, w), "dpt_collate_pair differs from the torch ops"
        assert torch.equal(got, one), "dpt_collate_pair differs from dpt_collate on the concatenated batch"
    del want

    out_bytes = n * L * 8 * 2
    moved = out_bytes + n_tok * 4 + 2 * n * (8 + 8 + 4)     # rows written; ids, offsets, counts and statuses read
    moved1 = out_bytes + n_tok * 4 + n * 8
    pair_ms, torch_ms, single_ms = timed(pair), timed(torch_ops), timed(single)
    pair_ms2 = timed(pair)                                   # again after the others: the session's drift
    floor = moved / (args.hbm_gbs * 1e9) * 1e3
    res = {"workload": "%d pairs, source and target %d random printable ASCII bytes each, synthetic 32k vocabulary, raw mode, "
                       "one dpt_encode_padded of all %d strings; int64 input_ids + labels" % (n, half, 2 * n),
           "device": torch.cuda.get_device_name(0), "lib": os.path.relpath(_lib.LIB_PATH, ROOT), "n_pairs": n, "n_tokens": n_tok,
           "longest_pair": longest, "row_len": L, "failed_rows": int((~ok).sum()), "hbm_gbs": args.hbm_gbs,
           "min_seconds": args.min_seconds,
           "pair": {"pair_ms": pair_ms, "pair_ms_again": pair_ms2, "bytes_moved": moved, "gbs": moved / (pair_ms * 1e-3) / 1e9,
                    "floor_ms": floor, "pair_over_floor": pair_ms / floor},
           "torch": {"torch_ms": torch_ms, "torch_over_pair": torch_ms / pair_ms},
           "single": {"single_ms": single_ms, "bytes_moved": moved1, "gbs": moved1 / (single_ms * 1e-3) / 1e9,
                      "pair_over_single": pair_ms / single_ms},
           "pair_faster_than_torch": bool(pair_ms < torch_ms)}

    torch.cuda.synchronize()
    doc = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as fh:
            doc = json.load(fh)
    doc[args.tag] = res
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
