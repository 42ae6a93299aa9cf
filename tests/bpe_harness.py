"""What the GPU tests of dpt_bpe_encode share: the guarded run of ``Bpe.encode_padded_device`` over ATOMS strings --
every output between 0xAA canaries that must survive, the slots a string does not use still 0xAA -- and its
comparison with tests/bpe_ref.py."""
import numpy as np

import bpe_ref

G = 67   # canary bytes on each side of an output


def run(bpe, vocab, lens, text2, cut, pad=3, off0=1_000_003, tok_word=True):
    """One call over the strings of ``lens`` bytes that text2 / cut hold back to back -> per string (status, ids,
    tok_word or None).  The text and the mask sit at odd addresses, str_off starts at off0."""
    import torch
    dev = torch.device("cuda", 0)
    n, nb = len(lens), len(text2)
    assert len(cut) == nb and int(np.sum(lens)) == nb
    d_text = torch.from_numpy(np.frombuffer(b"\xbf" * pad + text2 + b"\x80" * 8, dtype=np.uint8).copy()).to(dev)
    d_cut = torch.from_numpy(np.frombuffer(b"\x03" * pad + cut + b"\x03" * 8, dtype=np.uint8).copy()).to(dev)
    offs = np.full(n + 1, off0, dtype=np.int64)
    offs[1:] += np.cumsum(np.asarray(lens, dtype=np.int64))
    d_offs = torch.from_numpy(offs).to(dev)

    def guarded(nbytes, align):
        buf = torch.full((G + nbytes + G + align,), 0xAA, dtype=torch.uint8, device=dev)
        skip = (-(buf.data_ptr() + G)) % align
        return buf[skip:skip + G + nbytes + G]

    def inner(buf, nbytes):
        got = buf.cpu().numpy()
        assert (got[:G] == 0xAA).all() and (got[G + nbytes:] == 0xAA).all(), "a store outside the output"
        return got[G:G + nbytes].copy()

    b_ids, b_word, b_cnt, b_st = guarded(4 * nb, 4), guarded(4 * nb, 4), guarded(8 * n, 8), guarded(4 * n, 4)
    bpe.encode_padded_device(vocab, d_text.data_ptr() + pad, nb, d_offs.data_ptr(), d_cut.data_ptr() + pad, n, b_ids.data_ptr() + G,
                             nb, b_cnt.data_ptr() + G, b_st.data_ptr() + G, b_word.data_ptr() + G if tok_word else 0)
    torch.cuda.synchronize()
    ids, words = inner(b_ids, 4 * nb).view(np.int32), inner(b_word, 4 * nb).view(np.uint32)
    counts, status = inner(b_cnt, 8 * n).view(np.uint64), inner(b_st, 4 * n).view(np.int32)
    if not tok_word:
        assert (words == 0xAAAAAAAA).all()
    out, o = [], 0
    for s in range(n):
        c, ln = int(counts[s]), int(lens[s])
        assert c <= ln
        if status[s] == 0:
            # (a string's slots past its count hold tokens-in-progress or the canary; never another string's data)
            out.append((0, ids[o:o + c].tolist(), words[o:o + c].tolist() if tok_word else None))
        else:
            assert c == 0
            out.append((int(status[s]), [], [] if tok_word else None))
        o += ln
    return out


def check(bpe, vocab, piece_id, table, lens, text2, cut, want=None, **kw):
    """``run`` equals the model (or ``want``, the model's answer computed before); returns the model's answer."""
    if want is None:
        want = bpe_ref.encode(piece_id, table, lens, text2, cut)
    got = run(bpe, vocab, lens, text2, cut, **kw)
    if kw.get("tok_word", True) is False:
        want_cmp = [(st, ids, None) for st, ids, _ in want]
    else:
        want_cmp = want
    bad = [i for i, (g, w) in enumerate(zip(got, want_cmp)) if g != w]
    if bad:
        i = bad[0]
        o = int(np.sum(lens[:i]))
        raise AssertionError((len(bad), "strings differ; first", i, text2[o:o + int(lens[i])][:120], got[i], want_cmp[i]))
    return want
