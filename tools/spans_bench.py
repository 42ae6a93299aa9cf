#!/usr/bin/env python3
"""Time of dpt_token_spans against the dpt_encode call it follows, on one batch, device path.

Default: bench.py's cfg2 (1M x 256-byte random printable ASCII, the synthetic 32k vocabulary, raw
mode).  Both calls run on the same device buffers in one process; each is timed with a HIP event pair
around `reps` back-to-back calls after warm-up, the repetitions chosen so that each timed section
lasts at least --min-seconds.  The result is checked once (every span_status is its status, every
string's last token ends at its length) and written as one JSON document.

The bytes the spans pass has to move follow from the shapes: the text once, 4 bytes per id read and
8 written (tok_end, tok_word), 16 bytes of offsets and 8 of statuses per string; `floor_ms` is that
over --hbm-gbs (default: the 6290 GB/s a streaming copy measured on this part).

    python tools/spans_bench.py --out profiles/spans_bench.json
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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--hbm-gbs", type=float, default=6290.0)
    ap.add_argument("--no-words", action="store_true", help="tok_word = NULL (4 bytes less per id)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch
    from dptok import Encoder, Vocab, synth

    text, offs = synth.random_ascii_corpus(args.strings, args.length, seed=args.seed)
    n, n_bytes = len(offs) - 1, int(offs[-1])
    enc = Encoder(Vocab(synth.llama_shaped_vocab(), 0))
    dev = "cuda"
    d_text = torch.from_numpy(text).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64)).to(dev)
    ids = torch.empty(n_bytes, dtype=torch.int32, device=dev)
    id_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    tok_end = torch.empty(n_bytes, dtype=torch.int32, device=dev)
    tok_word = None if args.no_words else torch.empty(n_bytes, dtype=torch.int32, device=dev)
    ss = torch.empty(n, dtype=torch.int32, device=dev)
    enc.reserve(n_bytes, n)
    stream = torch.cuda.current_stream().cuda_stream

    def encode():
        enc.encode_device(d_text.data_ptr(), n_bytes, d_off.data_ptr(), n, ids.data_ptr(), n_bytes, id_off.data_ptr(),
                          st.data_ptr(), stream=stream)

    def spans():
        enc.spans_device(d_text.data_ptr(), n_bytes, d_off.data_ptr(), n, ids.data_ptr(), id_off.data_ptr(), st.data_ptr(),
                         tok_end.data_ptr(), ss.data_ptr(), tok_word_ptr=0 if tok_word is None else tok_word.data_ptr(),
                         stream=stream)

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
                return ms / reps, reps
            reps = max(reps * 2, int(reps * args.min_seconds * 1.2e3 / max(ms, 1e-3)) + 1)

    encode()
    torch.cuda.synchronize()
    enc_ms, enc_reps = timed(encode)
    spans_ms, spans_reps = timed(spans)
    torch.cuda.synchronize()

    h_off, h_st, h_ss = id_off.cpu().numpy(), st.cpu().numpy(), ss.cpu().numpy()
    n_tok = int(h_off[-1])
    assert np.array_equal(h_ss, h_st), "span_status differs from status"
    ok = h_st == 0
    last = (h_off[1:] - 1)[ok & (h_off[1:] > h_off[:-1])]
    ends = tok_end.cpu().numpy().view(np.uint32)
    want = np.diff(offs.astype(np.int64))[ok & (h_off[1:] > h_off[:-1])]
    assert np.array_equal(ends[last], want), "a string's last token does not end at its length"

    moved = n_bytes + n_tok * (4 + 4 + (0 if tok_word is None else 4)) + n * (16 + 8)
    res = {"workload": "cfg2 raw, %d x %d bytes, synthetic 32k vocabulary, device path" % (n, args.length),
           "device": torch.cuda.get_device_name(0), "n_str": n, "n_bytes": n_bytes, "n_tokens": n_tok,
           "ids_per_byte": n_tok / max(n_bytes, 1), "tok_word": tok_word is not None,
           "encode_ms": enc_ms, "encode_reps": enc_reps, "spans_ms": spans_ms, "spans_reps": spans_reps,
           "spans_over_encode": spans_ms / enc_ms, "spans_bytes_moved": moved,
           "spans_gbs": moved / (spans_ms * 1e-3) / 1e9, "hbm_gbs": args.hbm_gbs,
           "floor_ms": moved / (args.hbm_gbs * 1e9) * 1e3, "spans_over_floor": spans_ms / (moved / (args.hbm_gbs * 1e9) * 1e3)}
    doc = json.dumps(res, indent=1)
    print(doc)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(doc + "\n")


if __name__ == "__main__":
    main()
