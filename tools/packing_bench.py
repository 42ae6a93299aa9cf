#!/usr/bin/env python3
"""Time of the three packing calls on one encoded batch, device path, against the two routes a caller has without
them.

Batches: ``ascii`` (bench.py's cfg2: 1M x 256-byte random printable ASCII) and ``s2orc`` (200k abstract-shaped
strings), both through the synthetic 32k vocabulary in raw mode.  Row lengths 512 and 2048, int64 rows, input_ids +
position_ids + segment_ids.  Every figure is a HIP event pair around --steps back-to-back calls after --warmup, in ms
per call:

  sizes_ms, cumsum_ms, plan_ms, write_ms   dpt_pack_sizes, torch.cumsum into tok_off, dpt_pack_plan (str_row, str_col,
                  row_first, row_fill, row_cap = n_rows), dpt_pack_write
  collate_ms      dpt_collate of the same batch to [n_str, min(longest, L)] (input_ids + attention_mask)
  host_ms         today's host route, wall clock: the lengths copied back, the row of every string from a numpy
                  searchsorted chain, the placement copied up, and a torch scatter of the ids into the rows
  fill            T / (n_rows x L) of the packed rows against collate's T / (n_str x row)

The plan's three kernels are not separated here: run this script under a kernel trace with --trace-only (the plan
alone, --steps times) and read plan_walk_kernel's share from the trace.

    python tools/packing_bench.py --out profiles/packing_bench.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dp-tokenization_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", default="ascii,s2orc")
    ap.add_argument("--ascii-strings", type=int, default=1_000_000)
    ap.add_argument("--s2orc-strings", type=int, default=200_000)
    ap.add_argument("--row-lens", default="512,2048")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--procs", type=int, default=12)
    ap.add_argument("--trace-only", action="store_true", help="run the plan alone (for a kernel trace)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    from dptok import synth
    corpora = {}
    for name in args.batches.split(","):   # (generated before any GPU work: the generator forks)
        if name == "ascii":
            corpora[name] = synth.random_ascii_corpus(args.ascii_strings, 256, seed=1)
        else:
            corpora[name] = synth.generate_parallel("s2orc", args.s2orc_strings, procs=args.procs, seed=4)

    import torch
    from dptok import Encoder, Vocab, collate, packing
    dev = "cuda"
    enc = Encoder(Vocab(synth.llama_shaped_vocab(), 0))
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.steps

    res = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "batches": {}}
    for name, (text, offs) in corpora.items():
        n, n_bytes = len(offs) - 1, int(offs[-1])
        d_text = torch.from_numpy(text).to(dev)
        d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
        ids = torch.empty(n_bytes, dtype=torch.int32, device=dev)
        id_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        st = torch.empty(n, dtype=torch.int32, device=dev)
        enc.reserve(n_bytes, n)
        enc.encode_device(d_text.data_ptr(), n_bytes, d_off.data_ptr(), n, ids.data_ptr(), n_bytes, id_off.data_ptr(), st.data_ptr(),
                          stream=stream)
        torch.cuda.synchronize()
        del d_text
        n_tok = int(id_off[-1])
        longest = int((id_off[1:] - id_off[:-1]).max())
        batch = {"n_str": n, "n_bytes": n_bytes, "n_tokens": n_tok, "longest": longest, "failed": int((st != 0).sum()), "row_lens": {}}
        lengths = torch.empty(n, dtype=torch.int32, device=dev)
        tok_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        str_row, str_col = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        n_rows_d = torch.empty(1, dtype=torch.int64, device=dev)
        ws_bytes = packing.plan_workspace_bytes(n)
        ws = torch.empty(ws_bytes // 4 + 1, dtype=torch.int32, device=dev)
        side = (ids.data_ptr(), id_off.data_ptr(), 0, st.data_ptr())
        for L in (int(x) for x in args.row_lens.split(",")):
            def sizes():
                packing.pack_sizes_device(id_off.data_ptr(), n, lengths.data_ptr(), L, status_ptr=st.data_ptr(), stream=stream)

            def cumsum():
                torch.cumsum(lengths, 0, dtype=torch.int64, out=tok_off[1:])

            sizes()
            cumsum()
            packing.pack_plan_device(tok_off.data_ptr(), n, L, 0, n_rows_d.data_ptr(), ws.data_ptr(), ws_bytes, stream=stream)
            n_rows = int(n_rows_d.item())
            T = int(tok_off[-1])
            row_first = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
            row_fill = torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev)

            def plan():
                packing.pack_plan_device(tok_off.data_ptr(), n, L, n_rows, n_rows_d.data_ptr(), ws.data_ptr(), ws_bytes,
                                         str_row_ptr=str_row.data_ptr(), str_col_ptr=str_col.data_ptr(), row_first_ptr=row_first.data_ptr(),
                                         row_fill_ptr=row_fill.data_ptr(), stream=stream)

            if args.trace_only:
                timed(plan)
                continue
            rows = [torch.empty((n_rows, L), dtype=torch.int64, device=dev) for _ in range(3)]

            def write():
                packing.pack_write_device(side, n, tok_off.data_ptr(), row_first.data_ptr(), n_rows_d.data_ptr(), n_rows, rows[0].data_ptr(),
                                          L, position_ids_ptr=rows[1].data_ptr(), segment_ids_ptr=rows[2].data_ptr(), stream=stream)

            r = {"n_rows": n_rows, "kept_tokens": T, "fill": T / (n_rows * L), "sizes_ms": timed(sizes), "cumsum_ms": timed(cumsum),
                 "plan_ms": timed(plan), "write_ms": timed(write)}
            r["packing_ms"] = r["sizes_ms"] + r["cumsum_ms"] + r["plan_ms"] + r["write_ms"]
            r["write_gbs"] = 3 * n_rows * L * 8 / (r["write_ms"] * 1e-3) / 1e9

            # today's host route: lengths back, the numpy chain, the placement up, a torch scatter
            def host_route():
                ln = lengths.cpu().numpy().astype(np.int64)
                P = np.concatenate([[0], np.cumsum(ln)])
                starts, s = [], int(np.searchsorted(P, 0, "right")) - 1
                while s < n:
                    starts.append(s)
                    s = int(np.searchsorted(P, P[s] + L, "right")) - 1
                starts = np.asarray(starts, dtype=np.int64)
                row_of = np.searchsorted(starts, np.arange(n), "right") - 1
                begin = torch.from_numpy(row_of * L + (P[:-1] - P[starts[np.maximum(row_of, 0)]])).to(dev)
                d_ln = lengths.long()
                tok_str = torch.repeat_interleave(torch.arange(n, device=dev), d_ln)
                k = torch.arange(T, device=dev) - (tok_off[:-1] - tok_off[0])[tok_str]
                src = (id_off[:-1] - id_off[0])[tok_str] + k
                out = torch.zeros(len(starts) * L, dtype=torch.int64, device=dev)
                out[begin[tok_str] + k] = ids[src].long()
                torch.cuda.synchronize()
                return out.view(-1, L)

            want = host_route()
            write()
            assert want.shape[0] == n_rows and torch.equal(want, rows[0]), "dpt_pack_write differs from the host route"
            t0 = time.perf_counter()
            for _ in range(3):
                host_route()
            r["host_ms"] = (time.perf_counter() - t0) / 3 * 1e3
            del want, rows

            # dpt_collate of the same batch, one row per string
            Lc = min(longest, L)
            crow = [torch.empty((n, Lc), dtype=torch.int64, device=dev) for _ in range(2)]
            r["collate_ms"] = timed(lambda: collate.collate_device(ids.data_ptr(), id_off.data_ptr(), n, crow[0].data_ptr(), Lc,
                                                                   status_ptr=st.data_ptr(), mask_ptr=crow[1].data_ptr(), stream=stream))
            r["collate_row_len"] = Lc
            r["collate_fill"] = T / (n * Lc)
            del crow
            batch["row_lens"][str(L)] = r
            print(name, L, json.dumps(r), flush=True)
        res["batches"][name] = batch
        del ids, id_off, st

    torch.cuda.synchronize()
    if args.out and not args.trace_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
