#!/usr/bin/env python3
"""Device default-encoding timing: dpt_bpe_encode next to the dpt_encode (DPT_MODE_ATOMS) on the same ATOMS text in the
same session -- the S2ORC-shaped corpus and the 1M x 256-byte corpus through the llama rule (dpt_pretok_write_atoms,
the recorded SentencePiece model's pair table), the BLOOM workload of ``bench.py --workload bloom`` on the BLOOM-scale
table -- and, at the adapters' level, ``dp_tokenize.batch_default`` against the host tokenizer it replaces.

The one condition: at adapter level the device path beats ``[tokenizer.encode(t) for t in texts]`` by more than the
spread of the alternating runs.  The kernel's time relative to dpt_encode is recorded, not bounded.

HIP events around each call on one stream, a warm-up, then the median of --steps (>= 20) steps; the adapter level is a
host clock around calls that end in device-to-host copies, device and host alternating.

  python tools/bpe_bench.py --out profiles/bpe_bench.json
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


def kernel_level(torch, name, bpe, enc, text2, offs2, cut, steps, warmup):
    """One ATOMS batch on the device: dpt_bpe_encode and dpt_encode over it."""
    n, total = int(offs2.numel()) - 1, int(text2.numel())
    stream = torch.cuda.Stream()
    sid = stream.cuda_stream
    ids = torch.empty(total, dtype=torch.int32, device="cuda")
    words = torch.empty(total, dtype=torch.int32, device="cuda")
    counts = torch.empty(n, dtype=torch.int64, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    id_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    enc.reserve(total, n)
    res = {"corpus": name, "strings": n, "atoms_bytes": total, "atoms": int((cut != 0).sum().item())}

    def default(w):
        bpe.encode_padded_device(enc.vocab, text2.data_ptr(), total, offs2.data_ptr(), cut.data_ptr(), n, ids.data_ptr(), total,
                                 counts.data_ptr(), st.data_ptr(), w, sid)

    def dp():
        enc.encode_device(text2.data_ptr(), total, offs2.data_ptr(), n, ids.data_ptr(), total, id_off.data_ptr(), st.data_ptr(),
                          cut_ptr=cut.data_ptr(), stream=sid, mode="atoms")

    res["bpe_ms"], res["bpe_ms_min"] = timed(torch, stream, lambda: default(0), steps, warmup)
    res["bpe_tok_word_ms"], _ = timed(torch, stream, lambda: default(words.data_ptr()), steps, warmup)
    stream.synchronize()
    res.update(bpe_ok=int((st == 0).sum().item()), default_ids=int(counts.sum().item()))
    res["encode_atoms_ms"], res["encode_atoms_ms_min"] = timed(torch, stream, dp, steps, warmup)
    stream.synchronize()
    res.update(dp_ok=int((st == 0).sum().item()), dp_ids=int(id_off[-1].item()))
    # what the call reads and writes: text + mask, offsets, ids, counts + status (the table's lines come from L2 / MALL)
    res["bpe_moved_bytes"] = 2 * total + 8 * (n + 1) + 4 * res["default_ids"] + 12 * n
    res["bpe_moved_GBps"] = res["bpe_moved_bytes"] / (res["bpe_ms"] * 1e-3) / 1e9
    res["bpe_atoms_GBps"] = total / (res["bpe_ms"] * 1e-3) / 1e9
    res["bpe_over_encode"] = res["bpe_ms"] / res["encode_atoms_ms"]
    res["lookups_per_s"] = (res["atoms"] + 2 * (res["atoms"] - res["default_ids"])) / (res["bpe_ms"] * 1e-3)
    return res


def adapter_level(name, dp, tok, texts, reps):
    """``dp.batch_default(texts)`` against ``[tok.encode(t) for t in texts]``, alternating."""
    n_bytes = sum(len(t.encode("utf-8")) for t in texts)
    same = dp.batch_default(texts[:500]) == [list(tok.encode(t)) for t in texts[:500]]   # (also the warm-up)
    t = {"device": [], "host": []}
    for _ in range(reps):
        t0 = time.perf_counter()
        dp.batch_default(texts)
        t["device"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        [tok.encode(x) for x in texts]
        t["host"].append(time.perf_counter() - t0)
    d, h = statistics.median(t["device"]), statistics.median(t["host"])
    spread = max(max(v) - min(v) for v in t.values())
    return {"adapter": name, "strings": len(texts), "text_bytes": n_bytes, "reps": reps, "same_ids_on_sample": bool(same),
            "device_s": d, "host_s": h, "device_s_all": t["device"], "host_s_all": t["host"], "device_MBps": n_bytes / d / 1e6,
            "host_MBps": n_bytes / h / 1e6, "device_over_host": h / d, "spread_s": spread,
            "device_beats_host_by_more_than_the_spread": bool(h - d > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s2orc-strings", type=int, default=200_000)
    ap.add_argument("--cfg2-strings", type=int, default=1_000_000)
    ap.add_argument("--bloom-strings", type=int, default=200_000)
    ap.add_argument("--adapter-strings", type=int, default=4000)
    ap.add_argument("--adapter-reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20")
    sys.path.insert(0, os.path.join(ROOT, "dp-tokenization_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    from bloom_fixture import big_tokenizer_bytes, big_vocab, bloom_tokenizer, make_hf_cache
    from dptok import synth
    big = big_vocab()
    b_text, b_offs, b_cut = synth.bloom_like_parallel(args.bloom_strings, big, start=0, procs=16, length=256)   # (forks: before torch)
    s_text, s_offs = synth.generate_parallel("s2orc", args.s2orc_strings, start=0, procs=16, seed=4)
    c_text, c_offs = synth.random_ascii_corpus(args.cfg2_strings, 256, seed=1)
    import torch
    from dptok import Bpe, Encoder, Pretok, Vocab
    from dptok.bpe import pairs_from_merges, pairs_from_scores
    from packages.tokenizer_utils import dp_tokenize_bloom, dp_tokenize_llama
    from sp_llama import SPLlama, hf_llama
    res = {"steps": args.steps, "warmup": args.warmup, "kernels": [], "adapters": []}

    # the llama side: the recorded SentencePiece model
    sp_tok = SPLlama()
    sp, t2i = sp_tok.sp, sp_tok.get_vocab()
    n = sp.get_piece_size()
    exclude = [i for i in range(n) if sp.is_control(i) or sp.is_unknown(i) or sp.is_unused(i) or sp.is_byte(i)]
    bpe = Bpe(*pairs_from_scores(t2i, {sp.id_to_piece(i): sp.get_score(i) for i in range(n)}, exclude))
    enc, pretok = Encoder(Vocab(t2i, 0)), Pretok(t2i, "<s>", ["<unk>", "<s>", "</s>"], 0)
    for name, text, offs in (("s2orc", s_text, s_offs), ("cfg2_1Mx256", c_text, c_offs)):
        d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
        d_offs = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).cuda()
        text2, offs2, cut, pre = pretok.presplit(d_text, d_offs, atoms=True)
        r = kernel_level(torch, name, bpe, enc, text2, offs2, cut, args.steps, args.warmup)
        r.update(text_bytes=int(offs[-1] - offs[0]), refused=int((pre != 0).sum().item()))
        print(json.dumps(r), file=sys.stderr, flush=True)
        res["kernels"].append(r)
        del d_text, text2, cut
    # the BLOOM side: the BLOOM-scale table over the benchmark's ATOMS input
    model = json.loads(big_tokenizer_bytes())["model"]
    bpe_b, enc_b = Bpe(*pairs_from_merges(model["vocab"], model["merges"], model)), Encoder(Vocab(big, 0))
    nb = int(b_offs[-1])
    r = kernel_level(torch, "bloom", bpe_b, enc_b, torch.from_numpy(np.ascontiguousarray(b_text[:nb])).cuda(),
                     torch.from_numpy(np.ascontiguousarray(b_offs).view(np.int64)).cuda(),
                     torch.from_numpy(np.ascontiguousarray(b_cut[:nb])).cuda(), args.steps, args.warmup)
    print(json.dumps(r), file=sys.stderr, flush=True)
    res["kernels"].append(r)

    # adapters
    k = args.adapter_strings
    s_texts = synth.unpack(s_text[:int(s_offs[k]) + 1], s_offs[:k + 1])
    for name, tok in (("llama_sentencepiece", sp_tok), ("llama_hf_tokenizers", hf_llama())):
        dp, _ = dp_tokenize_llama(tok, "llama", device_pretokenize=True)
        res["adapters"].append(adapter_level(name, dp, tok, s_texts, args.adapter_reps))
    b_texts = [b_text[int(a):int(b)].tobytes().replace(b"\xc4\xa0", b" ").decode("utf-8")   # 'Ġ' back to the space it stands for
               for a, b in zip(b_offs[:k].tolist(), b_offs[1:k + 1].tolist())]
    with tempfile.TemporaryDirectory() as d:
        hf = make_hf_cache(d, big=True)
        tok = bloom_tokenizer(hf)
        dp, _ = dp_tokenize_bloom(tok, hf, device_pretokenize=True)
    res["adapters"].append(adapter_level("bloom_tokenizers", dp, tok, b_texts, args.adapter_reps))
    res["condition_met"] = all(a["device_beats_host_by_more_than_the_spread"] and a["same_ids_on_sample"] for a in res["adapters"])
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
