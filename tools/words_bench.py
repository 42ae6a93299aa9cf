#!/usr/bin/env python3
"""Time of the per-word comparison (dpt_word_compare_sizes + dpt_word_compare_write), one process per run.

--part kernel: on the S2ORC-shaped corpus and the 1M x 256-byte corpus in their llama ATOMS form (dpt_pretok_write_atoms,
the recorded SentencePiece model's pair table -- the batches of tools/bpe_bench.py), the two producing calls that feed
the comparison, dpt_token_spans (over a dpt_encode in atoms mode) and dpt_bpe_encode with tok_word, and then the sizes
and the write pass with every output, each by HIP events on one stream: a warm-up, then the median of --steps steps.
``compare_over_producers`` = (sizes + write) / (spans + bpe).  ``compare_device_ms`` is a host clock around
``dptok.words.compare_device``, which adds the two cumsums, the allocation and the one host read.

--part e2e --route words|host: the first --strings texts of the S2ORC-shaped corpus through the llama adapter
(SentencePiece object, device_pretokenize=True), a host clock around one of two routes to the same three lists:
  words   ``batch_compare(texts, words=True)``
  host    what a caller had before the keyword: ``batch_compare(texts)``, then ``batch_spans`` and ``batch_default``
          for the ids, and a Python loop over the counts that slices the token strings of the improved words
and a digest of the lists, so that two runs can be compared.  With DPT_LIB pointing at a library built before the
word-compare calls the host route runs on that library.  Alternate the runs:

    python tools/words_bench.py --part kernel --out profiles/words_bench.json
    for k in 1 2 3; do
      DPT_LIB=.../parent/libdpt.so python tools/words_bench.py --part e2e --route host --tag parent_host_$k --out profiles/words_bench.json
      python tools/words_bench.py --part e2e --route words --tag words_$k --out profiles/words_bench.json
    done
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dp-tokenization_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from decode_bench import timed  # noqa: E402


def kernel_part(args):
    import numpy as np
    from dptok import synth
    s_text, s_offs = synth.generate_parallel("s2orc", args.s2orc_strings, start=0, procs=16, seed=4)   # (forks: before torch)
    c_text, c_offs = synth.random_ascii_corpus(args.cfg2_strings, 256, seed=1)
    import torch
    from dptok import Bpe, Encoder, Pretok, Vocab, words
    from dptok.bpe import pairs_from_scores
    from sp_llama import SPLlama
    sp_tok = SPLlama()
    sp, t2i = sp_tok.sp, sp_tok.get_vocab()
    n_piece = sp.get_piece_size()
    exclude = [i for i in range(n_piece) if sp.is_control(i) or sp.is_unknown(i) or sp.is_unused(i) or sp.is_byte(i)]
    bpe = Bpe(*pairs_from_scores(t2i, {sp.id_to_piece(i): sp.get_score(i) for i in range(n_piece)}, exclude))
    enc, pretok = Encoder(Vocab(t2i, 0)), Pretok(t2i, "<s>", ["<unk>", "<s>", "</s>"], 0)
    out = []
    for name, text, offs in (("s2orc", s_text, s_offs), ("cfg2_1Mx256", c_text, c_offs)):
        d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
        d_offs = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).cuda()
        text2, offs2, cut, pre = pretok.presplit(d_text, d_offs, atoms=True)
        del d_text
        n, total = int(offs2.numel()) - 1, int(text2.numel())
        stream = torch.cuda.Stream()
        sid = stream.cuda_stream
        dev = "cuda"
        ids, end, word, b_ids, b_word = (torch.empty(total, dtype=torch.int32, device=dev) for _ in range(5))
        id_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        b_cnt = torch.empty(n, dtype=torch.int64, device=dev)
        st, sst, b_st = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
        enc.reserve(total, n)

        def encode():
            enc.encode_device(text2.data_ptr(), total, offs2.data_ptr(), n, ids.data_ptr(), total, id_off.data_ptr(), st.data_ptr(),
                              cut_ptr=cut.data_ptr(), stream=sid, mode="atoms")

        def spans():
            enc.spans_device(text2.data_ptr(), total, offs2.data_ptr(), n, ids.data_ptr(), id_off.data_ptr(), st.data_ptr(), end.data_ptr(),
                             sst.data_ptr(), tok_word_ptr=word.data_ptr(), cut_ptr=cut.data_ptr(), stream=sid, mode="atoms")

        def default():
            bpe.encode_padded_device(enc.vocab, text2.data_ptr(), total, offs2.data_ptr(), cut.data_ptr(), n, b_ids.data_ptr(), total,
                                     b_cnt.data_ptr(), b_st.data_ptr(), b_word.data_ptr(), sid)

        r = {"corpus": name, "strings": n, "atoms_bytes": total, "refused": int((pre != 0).sum().item())}
        r["encode_atoms_ms"], _ = timed(torch, stream, encode, args.steps, args.warmup)
        r["spans_ms"], r["spans_ms_min"] = timed(torch, stream, spans, args.steps, args.warmup)
        r["bpe_tok_word_ms"], r["bpe_tok_word_ms_min"] = timed(torch, stream, default, args.steps, args.warmup)
        stream.synchronize()
        side_a = (id_off.data_ptr(), 0, sst.data_ptr(), word.data_ptr(), end.data_ptr())
        side_b = (offs2.data_ptr(), b_cnt.data_ptr(), b_st.data_ptr(), b_word.data_ptr(), 0)
        per_str = torch.zeros((5, n), dtype=torch.int32, device=dev)
        flags = words.WORDS_LESS

        def sizes():
            words.sizes_device(side_a, side_b, n, flags, per_str[0].data_ptr(), per_str[1].data_ptr(), per_str[4].data_ptr(),
                               len_a_ptr=per_str[2].data_ptr(), len_b_ptr=per_str[3].data_ptr(), stream=sid)

        r["sizes_ms"], r["sizes_ms_min"] = timed(torch, stream, sizes, args.steps, args.warmup)
        stream.synchronize()
        offs_w = torch.zeros((2, n + 1), dtype=torch.int64, device=dev)
        torch.cumsum(per_str[:2], dim=1, out=offs_w[:, 1:])
        n_words, n_sel = (int(x) for x in offs_w[:, -1].tolist())
        per_word = torch.empty((2, max(n_words, 1)), dtype=torch.int32, device=dev)
        per_sel = torch.empty((8, max(n_sel, 1)), dtype=torch.int32, device=dev)
        wst = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def write():
            words.write_device(side_a, side_b, n, flags, wst.data_ptr(), word_off_ptr=offs_w[0].data_ptr(), cnt_a_ptr=per_word[0].data_ptr(),
                               cnt_b_ptr=per_word[1].data_ptr(), sel_off_ptr=offs_w[1].data_ptr(),
                               **{k + "_ptr": per_sel[i].data_ptr() for i, k in enumerate(("sel_str", "sel_word", "sel_begin", "sel_end",
                                                                                          "sel_a_first", "sel_a_count", "sel_b_first",
                                                                                          "sel_b_count"))}, stream=sid)

        r["write_ms"], r["write_ms_min"] = timed(torch, stream, write, args.steps, args.warmup)
        stream.synchronize()
        assert torch.equal(wst, per_str[4]), "the write pass's statuses differ from the sizes pass's"
        r.update(ok=int((wst == 0).sum().item()), internal=int((wst == 4).sum().item()), words=n_words, improved_words=n_sel,
                 dp_ids=int(per_str[2].sum().item()), default_ids=int(per_str[3].sum().item()))
        a = words.Side(id_off, word, status=sst, tok_end=end)
        b = words.Side(offs2, b_word, counts=b_cnt, status=b_st)
        t = []
        for _ in range(args.warmup + 5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            words.compare_device(a, b, flags)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        r["compare_device_ms"] = statistics.median(t[args.warmup:])
        # what the two passes read and write: both streams twice, the offsets, counts and statuses; the counts and records
        r["compare_moved_bytes"] = 2 * 4 * (r["dp_ids"] + r["default_ids"]) + 2 * n * (8 + 8 + 8 + 4 + 4) + 5 * 4 * n + 2 * 4 * n_words + 8 * 4 * n_sel
        r["compare_ms"] = r["sizes_ms"] + r["write_ms"]
        r["compare_moved_GBps"] = r["compare_moved_bytes"] / (r["compare_ms"] * 1e-3) / 1e9
        r["compare_over_producers"] = r["compare_ms"] / (r["spans_ms"] + r["bpe_tok_word_ms"])
        print(json.dumps(r), file=sys.stderr, flush=True)
        out.append(r)
        del text2, cut
    return {"steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "kernels": out}


def host_route(dp, texts, dp_piece):
    """The three lists from the calls there were before ``words=True``."""
    c = dp.batch_compare(texts)
    spans = dp.batch_spans(texts)
    default = dp.batch_default(texts)
    word_ids, improved, worse = [], [], []
    for k in range(len(texts)):
        w = c["default_word_counts"][k]
        if w is None:
            word_ids.append(None), improved.append(None), worse.append(None)
            continue
        sel = [int(x) for x in (c["dp_word_counts"][k] < w).nonzero()[0]]
        a_start = [0] + c["dp_word_counts"][k].cumsum().tolist()
        b_start = [0] + w.cumsum().tolist()
        word_ids.append(sel)
        improved.append([[dp_piece[i] for i in spans[k].ids[a_start[x]:a_start[x + 1]]] for x in sel])
        worse.append([[dp_piece[i] for i in default[k][b_start[x]:b_start[x + 1]]] for x in sel])
    return word_ids, improved, worse


def e2e_part(args):
    from dptok import synth
    s_text, s_offs = synth.generate_parallel("s2orc", max(args.strings, 16), start=0, procs=16, seed=4)
    k = args.strings
    texts = synth.unpack(s_text[:int(s_offs[k]) + 1], s_offs[:k + 1])
    import torch
    from dptok import _lib
    from packages.tokenizer_utils import dp_tokenize_llama
    from sp_llama import SPLlama
    tok = SPLlama()
    dp, _ = dp_tokenize_llama(tok, "llama", device_pretokenize=True)
    assert dp.pretok_stats.default_off is None, dp.pretok_stats.default_off
    piece = {i: t for t, i in tok.get_vocab().items()}

    def words_route():
        c = dp.batch_compare(texts, words=True)
        return c["improved_word_ids"], c["improved_tokens"], c["worse_tokens"]

    route = words_route if args.route == "words" else (lambda: host_route(dp, texts, piece))
    route()                                                                  # the warm-up
    t, lists = [], None
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lists = route()
        t.append(time.perf_counter() - t0)
    digest = hashlib.sha256(json.dumps(lists, ensure_ascii=False).encode("utf-8")).hexdigest()
    return {"route": args.route, "lib": os.path.relpath(_lib.LIB_PATH, ROOT), "has_words": _lib.has_words(), "strings": k,
            "text_bytes": sum(len(x.encode("utf-8")) for x in texts), "reps": args.reps, "seconds": statistics.median(t), "seconds_all": t,
            "device_taken": sum(x is not None for x in lists[0]), "improved_words": sum(len(x) for x in lists[0] if x is not None),
            "lists_sha256": digest, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--part", choices=["kernel", "e2e"], required=True)
    ap.add_argument("--route", choices=["words", "host"], default="words")
    ap.add_argument("--s2orc-strings", type=int, default=200_000)
    ap.add_argument("--cfg2-strings", type=int, default=1_000_000)
    ap.add_argument("--strings", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    res = kernel_part(args) if args.part == "kernel" else e2e_part(args)
    tag = args.tag or (args.part if args.part == "kernel" else "%s_%s" % (args.part, args.route))
    doc = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as fh:
            doc = json.load(fh)
    doc[tag] = res
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
