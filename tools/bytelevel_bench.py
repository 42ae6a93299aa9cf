#!/usr/bin/env python3
"""Device byte-level pre-tokenization timing (dpt_bytelevel_sizes / dpt_bytelevel_write) next to the dpt_encode ATOMS
call the two passes feed, on the BLOOM-scale vocabulary with the text of ``bench.py --workload bloom`` (its
pre-tokenized strings with every 'Ġ' put back to the space it stands for) -- and, at the drop-in's level,
``dp_tokenize.batch`` of the BLOOM adapter with ``device_pretokenize`` on against off.

The condition the kernels have to meet: sizes + write together take less time than the encode they feed; otherwise
pre-tokenization is still the bottleneck of the BLOOM path.  Beside the times: the bytes each pass moves, the rate
that gives, a flat device copy of as many bytes measured in the same run, and whether the device's output is the
benchmark's input byte for byte.

HIP events around each call on one stream, a warm-up, then the median of --steps (>= 20) steps; the adapter level
is a host clock around calls that end in device-to-host copies, on and off alternating, over as many strings as the
host path finishes in seconds.

  python tools/bytelevel_bench.py --out profiles/bytelevel_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from decode_bench import timed  # noqa: E402


def raw_text(np, text, offs):
    """The benchmark's pre-tokenized strings as the text they came from: 'Ġ' (C4 A0) -> ' ' (every other byte is an
    ASCII letter) -> (text u8, offs int64)."""
    raw = text.tobytes()
    o = offs.astype(np.int64)
    parts = [raw[o[i]:o[i + 1]].replace(b"\xc4\xa0", b" ") for i in range(len(o) - 1)]
    out = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in parts], out=out[1:])
    return np.frombuffer(b"".join(parts) + b"\0", dtype=np.uint8).copy(), out


def kernel_level(torch, np, t2i, text, offs, want_text, want_cut, steps, warmup):
    from dptok import ByteLevelSplit, Encoder, Vocab
    split, enc = ByteLevelSplit(device=0), Encoder(Vocab(t2i, 0))
    n, n_bytes = len(offs) - 1, int(offs[-1] - offs[0])
    stream = torch.cuda.Stream()
    sid = stream.cuda_stream
    d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    d_offs = torch.from_numpy(np.ascontiguousarray(offs)).cuda()
    out_len = torch.empty(n, dtype=torch.int64, device="cuda")
    pre = torch.empty(n, dtype=torch.int32, device="cuda")
    offs2 = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    res = {"corpus": "bloom", "strings": n, "text_bytes": n_bytes}

    def sizes():
        split.sizes_device(d_text.data_ptr(), d_offs.data_ptr(), n, out_len.data_ptr(), pre.data_ptr(), sid)

    res["sizes_ms"], res["sizes_ms_min"] = timed(torch, stream, sizes, steps, warmup)
    with torch.cuda.stream(stream):
        torch.cumsum(out_len, 0, out=offs2[1:])
    stream.synchronize()
    total = int(offs2[-1].item())
    text2 = torch.empty(total + 8, dtype=torch.uint8, device="cuda")
    cut = torch.empty(total + 8, dtype=torch.uint8, device="cuda")

    def write():
        split.write_device(d_text.data_ptr(), d_offs.data_ptr(), n, pre.data_ptr(), text2.data_ptr(), offs2.data_ptr(),
                           cut.data_ptr(), sid)

    res["write_ms"], res["write_ms_min"] = timed(torch, stream, write, steps, warmup)
    ids = torch.empty(total, dtype=torch.int32, device="cuda")
    id_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    enc.reserve(total, n)

    def encode():
        enc.encode_device(text2.data_ptr(), total, offs2.data_ptr(), n, ids.data_ptr(), total, id_off.data_ptr(), st.data_ptr(),
                          cut_ptr=cut.data_ptr(), stream=sid, mode="atoms")

    res["encode_atoms_ms"], res["encode_atoms_ms_min"] = timed(torch, stream, encode, steps, warmup)
    stream.synchronize()
    h_pre, h_st = pre.cpu().numpy(), st.cpu().numpy()
    same = (total == len(want_text) and text2[:total].cpu().numpy().tobytes() == want_text.tobytes()
            and cut[:total].cpu().numpy().tobytes() == want_cut.tobytes())
    res.update(atoms_bytes=total, refused=int((h_pre != 0).sum()), encoded_ok=int((h_st == 0).sum()), ids=int(id_off[-1].item()),
               output_is_the_benchmark_input=bool(same))
    # what each pass reads and writes, and a flat copy of as many bytes (half read, half written)
    moved = {"sizes": n_bytes + 8 * (n + 1) + 12 * n, "write": n_bytes + 16 * (n + 1) + 4 * n + 2 * total}
    for k, b in moved.items():
        src, dst = torch.empty(b // 2, dtype=torch.uint8, device="cuda"), torch.empty(b // 2, dtype=torch.uint8, device="cuda")
        res["copy_bound_%s_ms" % k], _ = timed(torch, stream, lambda: dst.copy_(src), steps, warmup)
        res["moved_bytes_%s" % k] = b
        res["%s_moved_GBps" % k] = b / (res["%s_ms" % k] * 1e-3) / 1e9
        del src, dst
    res["bytelevel_ms"] = res["sizes_ms"] + res["write_ms"]
    res["bytelevel_text_GBps"] = n_bytes / (res["bytelevel_ms"] * 1e-3) / 1e9
    res["encode_atoms_GBps"] = total / (res["encode_atoms_ms"] * 1e-3) / 1e9
    res["bytelevel_over_encode"] = res["bytelevel_ms"] / res["encode_atoms_ms"]
    res["bytelevel_faster_than_encode"] = res["bytelevel_ms"] < res["encode_atoms_ms"]
    return res


def adapter_level(texts, reps, large):
    """dp_tokenize.batch of the BLOOM adapter over ``texts`` on the BLOOM-scale tokenizer, device_pretokenize on
    against off; and the on path alone over ``large``, a batch of a size its users would run."""
    from bloom_fixture import bloom_tokenizer, make_hf_cache
    from packages.tokenizer_utils import dp_tokenize_bloom
    n_bytes = sum(len(t.encode("utf-8")) for t in texts)
    with tempfile.TemporaryDirectory() as d:
        hf = make_hf_cache(d, big=True)
        tok = bloom_tokenizer(hf)
        on, _ = dp_tokenize_bloom(tok, hf, device_pretokenize=True)
        off, _ = dp_tokenize_bloom(tok, hf)
    sample = texts[:500]
    same = on.batch(sample) == off.batch(sample)   # (also the warm-up of both paths)
    t = {"on": [], "off": []}
    for _ in range(reps):
        for k, f in (("on", on), ("off", off)):
            t0 = time.perf_counter()
            f.batch(texts)
            t[k].append(time.perf_counter() - t0)
        stats = tuple(on.pretok_stats)
    s_on, s_off = statistics.median(t["on"]), statistics.median(t["off"])
    big = []
    for _ in range(reps):
        t0 = time.perf_counter()
        on.batch(large)
        big.append(time.perf_counter() - t0)
    big_bytes = sum(len(x.encode("utf-8")) for x in large)
    return {"on_large_strings": len(large), "on_large_text_bytes": big_bytes, "on_large_s": statistics.median(big), "on_large_s_all": big,
            "on_large_MBps": big_bytes / statistics.median(big) / 1e6,
            "strings": len(texts), "text_bytes": n_bytes, "reps": reps, "same_ids_on_sample": bool(same), "on_s": s_on, "off_s": s_off,
            "on_s_all": t["on"], "off_s_all": t["off"], "on_MBps": n_bytes / s_on / 1e6, "off_MBps": n_bytes / s_off / 1e6,
            "on_over_off": s_off / s_on, "on_device": stats[0], "sent_to_host": stats[1], "on_faster": s_on < s_off}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strings", type=int, default=500_000)
    ap.add_argument("--adapter-strings", type=int, default=4000, help="what the host path finishes in seconds")
    ap.add_argument("--adapter-large-strings", type=int, default=200_000, help="the on path alone, at a size it is meant for")
    ap.add_argument("--adapter-reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-adapter", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20")
    sys.path.insert(0, os.path.join(ROOT, "dp-tokenization_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    from bloom_fixture import big_vocab
    from dptok import synth
    t2i = big_vocab()
    atoms_text, atoms_offs, atoms_cut = synth.bloom_like_parallel(args.strings, t2i, start=0, procs=16, length=256)   # (forks: before torch)
    text, offs = raw_text(np, atoms_text, atoms_offs)
    import torch
    res = {"steps": args.steps, "warmup": args.warmup}
    res["kernels"] = kernel_level(torch, np, t2i, text, offs, atoms_text[:int(atoms_offs[-1])], atoms_cut[:int(atoms_offs[-1])],
                                  args.steps, args.warmup)
    print(json.dumps(res["kernels"]), file=sys.stderr, flush=True)
    res["condition_met"] = bool(res["kernels"]["bytelevel_faster_than_encode"])
    if not args.no_adapter:
        n, big = min(args.adapter_strings, args.strings), min(args.adapter_large_strings, args.strings)
        texts = synth.unpack(text[:int(offs[big]) + 1], offs[:big + 1].astype(np.uint64))
        res["adapter"] = adapter_level(texts[:n], args.adapter_reps, texts)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
