#!/usr/bin/env python3
"""Device pre-tokenization timing (dpt_pretok_sizes / dpt_pretok_write) next to the dpt_encode PRESPLIT call the
two passes feed, on two corpora -- 1M x 256-byte random ASCII strings and the S2ORC-shaped corpus -- and, at the
drop-in's level, ``dp_tokenize.batch`` in llama mode over real SentencePiece with ``device_pretokenize`` on
against off.

The condition the kernels have to meet: sizes + write together take less time than the encode they feed, on both
corpora; otherwise pre-tokenization is still the bottleneck of llama mode.  Beside the times: the bytes each pass
moves, the rate that gives, and a flat device copy of as many bytes measured in the same run (the ceiling; what
tools/micro/copy_bound.hip measures for the decode walk).

HIP events around each call on one stream, a warm-up, then the median of --steps (>= 20) steps; the adapter level
is a host clock around calls that end in device-to-host copies, on and off alternating.

  python tools/pretok_bench.py --out profiles/pretok_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from decode_bench import timed  # noqa: E402


def kernel_level(torch, np, synth, name, text, offs, steps, warmup):
    from dptok import Encoder, Pretok, Vocab
    t2i = synth.llama_shaped_vocab()
    lits = [x for x in ("<unk>", "<s>", "</s>") if x in t2i]
    pretok, enc = Pretok(t2i, "<s>", lits, 0), Encoder(Vocab(t2i, 0))
    n, n_bytes = len(offs) - 1, int(offs[-1] - offs[0])
    stream = torch.cuda.Stream()
    sid = stream.cuda_stream
    d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    d_offs = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).cuda()
    out_len = torch.empty(n, dtype=torch.int64, device="cuda")
    pre = torch.empty(n, dtype=torch.int32, device="cuda")
    offs2 = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    res = {"corpus": name, "strings": n, "text_bytes": n_bytes}

    def sizes():
        pretok.sizes_device(d_text.data_ptr(), d_offs.data_ptr(), n, out_len.data_ptr(), pre.data_ptr(), sid)

    res["sizes_ms"], res["sizes_ms_min"] = timed(torch, stream, sizes, steps, warmup)
    with torch.cuda.stream(stream):
        torch.cumsum(out_len, 0, out=offs2[1:])
    stream.synchronize()
    total = int(offs2[-1].item())
    text2 = torch.empty(total + 8, dtype=torch.uint8, device="cuda")
    cut = torch.empty(total + 8, dtype=torch.uint8, device="cuda")

    def write():
        pretok.write_device(d_text.data_ptr(), d_offs.data_ptr(), n, pre.data_ptr(), text2.data_ptr(), offs2.data_ptr(),
                            cut.data_ptr(), sid)

    res["write_ms"], res["write_ms_min"] = timed(torch, stream, write, steps, warmup)
    ids = torch.empty(total, dtype=torch.int32, device="cuda")
    id_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    enc.reserve(total, n)

    def encode():
        enc.encode_device(text2.data_ptr(), total, offs2.data_ptr(), n, ids.data_ptr(), total, id_off.data_ptr(), st.data_ptr(),
                          cut_ptr=cut.data_ptr(), stream=sid, mode="presplit")

    res["encode_presplit_ms"], res["encode_presplit_ms_min"] = timed(torch, stream, encode, steps, warmup)
    stream.synchronize()
    h_pre, h_st = pre.cpu().numpy(), st.cpu().numpy()
    res.update(presplit_bytes=total, refused=int((h_pre != 0).sum()), encoded_ok=int((h_st == 0).sum()), ids=int(id_off[-1].item()))
    # what each pass reads and writes, and a flat copy of as many bytes (half read, half written)
    moved = {"sizes": n_bytes + 8 * (n + 1) + 12 * n, "write": n_bytes + 16 * (n + 1) + 4 * n + 2 * total}
    for k, b in moved.items():
        src, dst = torch.empty(b // 2, dtype=torch.uint8, device="cuda"), torch.empty(b // 2, dtype=torch.uint8, device="cuda")
        res["copy_bound_%s_ms" % k], _ = timed(torch, stream, lambda: dst.copy_(src), steps, warmup)
        res["moved_bytes_%s" % k] = b
        res["%s_moved_GBps" % k] = b / (res["%s_ms" % k] * 1e-3) / 1e9
        del src, dst
    res["pretok_ms"] = res["sizes_ms"] + res["write_ms"]
    res["pretok_text_GBps"] = n_bytes / (res["pretok_ms"] * 1e-3) / 1e9
    res["encode_presplit_GBps"] = total / (res["encode_presplit_ms"] * 1e-3) / 1e9
    res["pretok_over_encode"] = res["pretok_ms"] / res["encode_presplit_ms"]
    res["pretok_faster_than_encode"] = res["pretok_ms"] < res["encode_presplit_ms"]
    return res


def adapter_level(synth, text, offs, n, reps):
    """dp_tokenize.batch over the first n strings with real SentencePiece, device_pretokenize on against off."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from sp_llama import SPLlama
    from packages.tokenizer_utils import dp_tokenize_llama
    texts = synth.unpack(text[: int(offs[n]) + 1], offs[: n + 1])
    n_bytes = int(offs[n] - offs[0])
    tok = SPLlama()
    on, _ = dp_tokenize_llama(tok, "llama", device_pretokenize=True)
    off, _ = dp_tokenize_llama(tok, "llama")
    sample = texts[:2000]
    same = on.batch(sample) == off.batch(sample)   # (also the warm-up of both paths)
    off.batch(texts[:8192])                        # the worker pool starts
    t = {"on": [], "off": []}
    for _ in range(reps):
        for k, f in (("on", on), ("off", off)):
            t0 = time.perf_counter()
            f.batch(texts)
            t[k].append(time.perf_counter() - t0)
        stats = tuple(on.pretok_stats)
    s_on, s_off = statistics.median(t["on"]), statistics.median(t["off"])
    return {"strings": n, "text_bytes": n_bytes, "reps": reps, "same_ids_on_sample": bool(same), "on_s": s_on, "off_s": s_off,
            "on_s_all": t["on"], "off_s_all": t["off"], "on_MBps": n_bytes / s_on / 1e6, "off_MBps": n_bytes / s_off / 1e6,
            "on_over_off": s_off / s_on, "certified": stats[0], "sent_to_host": stats[1],
            "refused_share": stats[1] / max(n, 1), "on_faster": s_on < s_off}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ascii-strings", type=int, default=1_000_000)
    ap.add_argument("--s2orc-strings", type=int, default=200_000)
    ap.add_argument("--adapter-strings", type=int, default=100_000)
    ap.add_argument("--adapter-reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-adapter", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20")
    sys.path.insert(0, os.path.join(ROOT, "dp-tokenization_amd"))
    import numpy as np
    from dptok import synth
    ascii_corpus = synth.random_ascii_corpus(args.ascii_strings, 256, seed=1)
    s2orc = synth.generate_parallel("s2orc", max(args.s2orc_strings, args.adapter_strings), start=0, procs=16, seed=4)
    import torch
    res = {"steps": args.steps, "warmup": args.warmup, "kernels": []}
    for name, (text, offs) in (("ascii_256", ascii_corpus), ("s2orc", (s2orc[0], s2orc[1][: args.s2orc_strings + 1]))):
        res["kernels"].append(kernel_level(torch, np, synth, name, text, offs, args.steps, args.warmup))
        print(json.dumps(res["kernels"][-1]), file=sys.stderr, flush=True)
    res["condition_met"] = all(k["pretok_faster_than_encode"] for k in res["kernels"])
    if not args.no_adapter:
        res["adapter"] = adapter_level(synth, s2orc[0], s2orc[1], args.adapter_strings, args.adapter_reps)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
