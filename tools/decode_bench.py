#!/usr/bin/env python3
"""Decode and round-trip timing (dpt_decode_sizes / dpt_decode / dpt_roundtrip) on the ids of the bench
workloads, next to the encode that produced them and two yardsticks measured in the same run:

* the ceiling: a flat device copy moving the same number of bytes (half read, half written);
* the floor: the host round trip the device call replaces -- SentencePiece's own decode of every string plus
  the compare, on 16 processes, over a fixed 4096-string subsample (ids: the SentencePiece model's own
  encoding of those strings; run before this process touches the GPU).

HIP events around each call on one stream, a warm-up, then the median of --steps (>= 20) steps.

  python tools/decode_bench.py --workload cfg2 --out profiles/decode_bench_cfg2.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SP_MODEL = os.path.join(ROOT, "tests", "golden", "sp_llama32k.model")
_SP = None


def _host_roundtrip(chunk):
    """(worker) decode + compare of one chunk of (ids, text): the number of strings that came back equal."""
    global _SP
    if _SP is None:
        import sentencepiece as spm
        _SP = spm.SentencePieceProcessor(model_file=SP_MODEL)
    return sum(_SP.decode(ids) == t for ids, t in chunk)


def host_floor(texts, procs=16, reps=3):
    """Seconds (best of reps) of the host round trip over ``texts`` on ``procs`` processes, and what it found."""
    import multiprocessing as mp
    import sentencepiece as spm
    sp = spm.SentencePieceProcessor(model_file=SP_MODEL)
    ids = sp.encode(list(texts))
    pairs = list(zip(ids, texts))
    k = 4 * procs
    chunks = [pairs[len(pairs) * i // k:len(pairs) * (i + 1) // k] for i in range(k)]
    with mp.get_context("spawn").Pool(procs) as pool:
        pool.map(_host_roundtrip, chunks)   # warm-up: the workers load the model
        best, equal = None, 0
        for _ in range(reps):
            t0 = time.perf_counter()
            equal = sum(pool.map(_host_roundtrip, chunks))
            dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
    dec_bytes = sum(len(sp.decode(i).encode("utf-8")) for i in ids)
    return {"strings": len(texts), "processes": procs, "seconds": best, "equal": equal, "ids": sum(len(i) for i in ids),
            "decoded_bytes": dec_bytes, "strings_per_s": len(texts) / best, "decoded_GBps": dec_bytes / best / 1e9}


def timed(torch, stream, fn, steps, warmup):
    """Median milliseconds of fn() on ``stream`` by HIP events."""
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            fn()
        stream.synchronize()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def corpus(synth, name, n):
    if name == "cfg2":
        return synth.random_ascii_corpus(n or 1_000_000, 256, seed=1)
    return synth.generate_parallel("s2orc", n or 200_000, start=0, procs=16, seed=4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["cfg2", "cfg4"], default="cfg2")
    ap.add_argument("--strings", type=int, default=None, help="default 1M (cfg2), 200k (cfg4)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-host-floor", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20")
    sys.path.insert(0, os.path.join(ROOT, "dp-tokenization_amd"))
    import numpy as np
    from dptok import synth
    text, offs = corpus(synth, args.workload, args.strings)
    n = len(offs) - 1
    n_bytes = int(offs[-1])
    res = {"workload": args.workload, "strings": n, "text_bytes": n_bytes, "steps": args.steps, "warmup": args.warmup}
    if not args.no_host_floor:   # before the GPU is opened: the workers are fresh processes without it
        res["host_floor"] = host_floor(synth.unpack(text[: int(offs[4096]) + 1], offs[:4097]))

    import torch
    from dptok import RT_DIFFERS, RT_EQUAL, Detok, Encoder, Vocab
    t2i = synth.llama_shaped_vocab()
    enc, dk = Encoder(Vocab(t2i, 0)), Detok(t2i, "sp")
    stream = torch.cuda.Stream()
    d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    d_offs = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).cuda()
    ids = torch.empty(n_bytes, dtype=torch.int32, device="cuda")
    id_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    lens = torch.empty(n, dtype=torch.int64, device="cuda")
    out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    dst, rt = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    fd = torch.empty(n, dtype=torch.int32, device="cuda")
    enc.reserve(n_bytes, n)
    sid = stream.cuda_stream
    p = {k: t.data_ptr() for k, t in (("text", d_text), ("offs", d_offs), ("ids", ids), ("id_off", id_off), ("st", st),
                                      ("lens", lens), ("out_off", out_off), ("dst", dst), ("rt", rt), ("fd", fd))}

    def encode():
        enc.encode_device(p["text"], n_bytes, p["offs"], n, p["ids"], n_bytes, p["id_off"], p["st"], stream=sid)

    def sizes():
        dk.sizes_device(p["ids"], p["id_off"], n, p["lens"], status_ptr=p["st"], strip_space=True, stream=sid)

    res["encode_ms"], res["encode_ms_min"] = timed(torch, stream, encode, args.steps, args.warmup)
    res["sizes_ms"], res["sizes_ms_min"] = timed(torch, stream, sizes, args.steps, args.warmup)
    with torch.cuda.stream(stream):
        torch.cumsum(lens, 0, out=out_off[1:])
    stream.synchronize()
    n_tok, dec_bytes = int(id_off[-1].item()), int(out_off[-1].item())
    out = torch.empty(dec_bytes + 8, dtype=torch.uint8, device="cuda")

    def decode():
        dk.decode_device(p["ids"], p["id_off"], n, out.data_ptr(), p["out_off"], p["dst"], status_ptr=p["st"], strip_space=True,
                         stream=sid)

    def roundtrip():
        dk.roundtrip_device(p["ids"], p["id_off"], p["text"], p["offs"], n, p["rt"], first_diff_ptr=p["fd"], status_ptr=p["st"],
                            strip_space=True, stream=sid)

    res["decode_ms"], res["decode_ms_min"] = timed(torch, stream, decode, args.steps, args.warmup)
    res["roundtrip_ms"], res["roundtrip_ms_min"] = timed(torch, stream, roundtrip, args.steps, args.warmup)
    stream.synchronize()
    h_st, h_rt, h_dst = st.cpu().numpy(), rt.cpu().numpy(), dst.cpu().numpy()
    res.update(ids=n_tok, decoded_bytes=dec_bytes, encoded_ok=int((h_st == 0).sum()),
               rt_equal=int(((h_rt == RT_EQUAL) & (h_st == 0)).sum()), rt_differs=int((h_rt == RT_DIFFERS).sum()),
               decode_status_ok=bool(np.array_equal(h_dst, h_st)))
    # the ceiling: a flat copy that moves as many bytes as the call reads and writes
    moved = {"decode": 4 * n_tok + 16 * n + dec_bytes, "roundtrip": 4 * n_tok + 16 * n + n_bytes, "sizes": 4 * n_tok + 16 * n}
    for k, b in moved.items():
        src, dstb = torch.empty(b // 2, dtype=torch.uint8, device="cuda"), torch.empty(b // 2, dtype=torch.uint8, device="cuda")
        res["copy_bound_%s_ms" % k], _ = timed(torch, stream, lambda: dstb.copy_(src), args.steps, args.warmup)
        res["moved_bytes_%s" % k] = b
        del src, dstb
    for k in ("decode", "roundtrip", "sizes"):
        res["%s_decoded_GBps" % k] = dec_bytes / (res["%s_ms" % k] * 1e-3) / 1e9
    res["encode_text_GBps"] = n_bytes / (res["encode_ms"] * 1e-3) / 1e9
    res["roundtrip_over_encode"] = res["roundtrip_ms"] / res["encode_ms"]
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
