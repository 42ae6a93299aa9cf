#!/usr/bin/env python3
"""Generator of tests/golden/bloom_pretok_cases.json.gz: what the `tokenizers` library's BLOOM-shaped pre-tokenizer
(Split(Regex(SPLIT), isolated) then ByteLevel without prefix space or regex; the object of
bloom_synth_tokenizer.json.gz) answers, recorded as data for tests/test_bytelevel_ref.py:

  separators   every Unicode scalar value c for which "a" + c + "a" is not one word (a sweep over all 1,112,064)
  cases        texts with their ``pre_tokenize_str`` words: bloom_texts(), bloom_big_texts() and random strings over
               spaces, separators, ASCII, accents, CJK, emoji, brackets, tabs and newlines

  python tests/golden/make_bloom_pretok.py
"""
import gzip
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

N_RANDOM = 400


def random_texts(separators, n=N_RANDOM, seed=41):
    rnd = random.Random(seed)
    pool = ([" "] * 12 + [chr(c) for c in separators] + list("abcxyzABC019-_'\"[]{}<>#/\\:;~") + list("éüßñ") + list("中文字龍")
            + ["😀", "🤖", "𝄞"] + ["\t", "\n", "\r\n"] + list("ءبي"))
    out = []
    while len(out) < n:
        out.append("".join(rnd.choice(pool) for _ in range(rnd.randint(0, 40))))
    return out


def main():
    from tokenizers import Tokenizer
    from bloom_fixture import big_vocab, bloom_big_texts, bloom_texts
    with gzip.open(os.path.join(HERE, "bloom_synth_tokenizer.json.gz"), "rb") as fh:
        pre = Tokenizer.from_str(fh.read().decode("utf-8")).pre_tokenizer
    seps = [cp for cp in range(0x110000) if not 0xD800 <= cp <= 0xDFFF and len(pre.pre_tokenize_str("a" + chr(cp) + "a")) != 1]
    texts = bloom_texts() + bloom_big_texts(big_vocab()) + random_texts(seps)
    cases = [{"text": t, "words": [w for w, _ in pre.pre_tokenize_str(t)]} for t in texts]
    out = {"separators": seps, "n_fixture": 300, "n_big": 400, "n_random": N_RANDOM, "cases": cases}
    with gzip.GzipFile(os.path.join(HERE, "bloom_pretok_cases.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(out, ensure_ascii=False).encode("utf-8"))
    print("bloom_pretok_cases written:", len(seps), "separators,", len(cases), "cases")


if __name__ == "__main__":
    main()
