#!/usr/bin/env python3
"""Time of dpt_collate on one encoded batch, device path, against its traffic floor and against torch ops.

Default: bench.py's cfg2 (1M x 256-byte random printable ASCII, the synthetic 32k vocabulary, raw mode).
Everything runs on the same device buffers in one process; each figure is a HIP event pair around `reps`
back-to-back calls after warm-up, the repetitions chosen so that each timed section lasts at least
--min-seconds.  The row length is the longest string's ids rounded up to 8 (nothing is truncated).  Per
element width (int32, int64):

  collate_ms      dpt_collate alone: from dpt_encode's CSR layout and from dpt_encode_padded's byte-offset
                  layout, input_ids + attention_mask + lengths, with and without labels
  floor_ms        the bytes the call has to move (rows written, 4 bytes per id read, the offsets / counts /
                  statuses read, the lengths written) over --hbm-gbs (default: the 6290 GB/s a streaming copy
                  measured on this part)
  torch_ms        the same tensors from the same CSR arrays with torch ops alone: an arange-vs-lengths mask,
                  a masked scatter of the ids, the mask cast, and (labels) a where
and for int64 without labels the whole step: dpt_encode + collate against dpt_encode_padded + collate.
The collate's tensors are checked for equality with torch's once.

--variant element sets DPT_COLLATE_NO_WIDE=1 before the library loads (every call through the element path);
the result is merged into --out under the variant's name, so two runs record both store paths:

    python tools/collate_bench.py --out profiles/collate_bench.json
    python tools/collate_bench.py --out profiles/collate_bench.json --variant element
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
    ap.add_argument("--strings", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=256)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--hbm-gbs", type=float, default=6290.0)
    ap.add_argument("--variant", choices=("wide", "element"), default="wide")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.variant == "element":
        os.environ["DPT_COLLATE_NO_WIDE"] = "1"

    import numpy as np
    import torch
    from dptok import Encoder, Vocab, collate, synth

    text, offs = synth.random_ascii_corpus(args.strings, args.length, seed=args.seed)
    n, n_bytes = len(offs) - 1, int(offs[-1])
    enc = Encoder(Vocab(synth.llama_shaped_vocab(), 0))
    dev = "cuda"
    d_text = torch.from_numpy(text).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    ids = torch.empty(n_bytes, dtype=torch.int32, device=dev)        # CSR
    id_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    ids_p = torch.empty(n_bytes, dtype=torch.int32, device=dev)      # byte-offset layout
    counts = torch.empty(n, dtype=torch.int64, device=dev)
    st_p = torch.empty(n, dtype=torch.int32, device=dev)
    lengths = torch.empty(n, dtype=torch.int32, device=dev)
    enc.reserve(n_bytes, n)
    stream = torch.cuda.current_stream().cuda_stream

    def encode():
        enc.encode_device(d_text.data_ptr(), n_bytes, d_off.data_ptr(), n, ids.data_ptr(), n_bytes, id_off.data_ptr(),
                          st.data_ptr(), stream=stream)

    def encode_padded():
        enc.encode_device_padded(d_text.data_ptr(), n_bytes, d_off.data_ptr(), n, ids_p.data_ptr(), n_bytes, counts.data_ptr(),
                                 st_p.data_ptr(), stream=stream)

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

    encode()
    encode_padded()
    torch.cuda.synchronize()
    n_tok = int(id_off[-1])
    longest = int((id_off[1:] - id_off[:-1]).max())
    L = -(-longest // 8) * 8
    pad_id, ignore = 0, -100
    res = {"workload": "cfg2 raw, %d x %d bytes, synthetic 32k vocabulary, device path" % (n, args.length),
           "device": torch.cuda.get_device_name(0), "variant": args.variant, "n_str": n, "n_bytes": n_bytes, "n_tokens": n_tok,
           "longest": longest, "row_len": L, "hbm_gbs": args.hbm_gbs, "min_seconds": args.min_seconds}

    for int64 in (False, True):
        dtype, width = (torch.int64, 8) if int64 else (torch.int32, 4)
        rows = [torch.empty((n, L), dtype=dtype, device=dev) for _ in range(3)]

        def run(padded, labels):
            collate.collate_device(ids_p.data_ptr() if padded else ids.data_ptr(), d_off.data_ptr() if padded else id_off.data_ptr(),
                                   n, rows[0].data_ptr(), L, counts_ptr=counts.data_ptr() if padded else 0,
                                   status_ptr=st_p.data_ptr() if padded else st.data_ptr(), mask_ptr=rows[1].data_ptr(),
                                   labels_ptr=rows[2].data_ptr() if labels else 0, lengths_ptr=lengths.data_ptr(),
                                   pad_id=pad_id, ignore_id=ignore, int64=int64, stream=stream)

        ar = torch.arange(L, device=dev)

        def torch_ops(labels):
            lens = id_off[1:] - id_off[:-1]
            mask = ar[None, :] < lens[:, None]
            inp = torch.full((n, L), pad_id, dtype=dtype, device=dev)
            inp.masked_scatter_(mask, ids[:n_tok].to(dtype))
            out = [inp, mask.to(dtype)]
            if labels:
                out.append(torch.where(mask, inp, ignore))
            return out

        # equality, once (a failed string has no ids in the CSR layout, so its torch row is all pad too)
        want = torch_ops(True)
        for padded in (False, True):
            for r in rows:
                r.fill_(-1)
            run(padded, True)
            for got, w in zip(rows, want):
                assert torch.equal(got, w), "dpt_collate differs from the torch ops"
            assert torch.equal(lengths.long(), want[1].sum(1)), "lengths differ"
        del want
        sec = {}
        for labels in (False, True):
            outs = 3 if labels else 2
            for padded in (False, True):
                moved = n * L * width * outs + n * 4 + n_tok * 4 + n * (12 + (16 if padded else 8))
                ms = timed(lambda: run(padded, labels))
                floor = moved / (args.hbm_gbs * 1e9) * 1e3
                sec["%s%s" % ("padded" if padded else "csr", "+labels" if labels else "")] = {
                    "collate_ms": ms, "bytes_moved": moved, "gbs": moved / (ms * 1e-3) / 1e9, "floor_ms": floor,
                    "collate_over_floor": ms / floor}
            t_ms = timed(lambda: torch_ops(labels))
            key = "csr+labels" if labels else "csr"
            sec["torch%s" % ("+labels" if labels else "")] = {"torch_ms": t_ms, "torch_over_collate": t_ms / sec[key]["collate_ms"]}
        if int64:
            e_ms, p_ms = timed(encode), timed(encode_padded)
            both = timed(lambda: (encode(), run(False, False)))
            both_p = timed(lambda: (encode_padded(), run(True, False)))
            sec["whole_step"] = {"encode_ms": e_ms, "encode_padded_ms": p_ms, "encode+collate_ms": both,
                                 "encode_padded+collate_ms": both_p, "padded_over_csr": both_p / both}
        res["int64" if int64 else "int32"] = sec
        del rows

    torch.cuda.synchronize()
    doc = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as fh:
            doc = json.load(fh)
    doc[args.variant] = res
    text_out = json.dumps(doc, indent=1)
    print(json.dumps(res, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text_out + "\n")


if __name__ == "__main__":
    main()
