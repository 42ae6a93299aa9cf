"""What the GPU tests of dpt_collate and dpt_collate_pair share: sentinel-guarded outputs, uploaded sources, random
batches, the comparison, and the fixtures of the adapter and encode tests."""
import numpy as np

import matrix_corpus as mc

GUARD = 64   # elements; a multiple of 16 bytes for both widths, so ``base`` below is the offset from a 16-byte boundary
SENT = -0x5A5A5A5B
PAD_ID, BOS_ID, SEP_ID, EOS_ID, IGNORE = -7, 40001, 40003, 40002, -100

OOV = "hello 字 world"   # raw mode: a word no vocabulary here tokenizes (status 1, ValueError in ``batch``)
TEXTS = ["the weather is nice", "hello world", "a", "optimal length tokenization of a longer sentence here", "x y", "it's 7:45"]


class Out:
    """[n_str, L] rows of ``stride`` elements inside a sentinel-filled tensor, ``base`` elements past GUARD."""

    def __init__(self, torch, n_str, L, stride, dtype, base=0):
        self.n_str, self.L, self.stride, self.base = n_str, L, stride or L, base
        self.span = (n_str - 1) * self.stride + L if n_str else 0
        self.whole = torch.full((GUARD + base + self.span + GUARD,), SENT, dtype=dtype, device="cuda")
        assert self.whole.data_ptr() % 16 == 0

    def ptr(self):
        return self.whole.data_ptr() + (GUARD + self.base) * self.whole.element_size()

    def rows(self):
        """the rows as a numpy [n_str, L] array, after asserting that nothing else was written"""
        w = self.whole.cpu().numpy()
        lo = GUARD + self.base
        assert (w[:lo] == SENT).all() and (w[lo + self.span:] == SENT).all(), "guard zone written"
        full = np.full(self.n_str * self.stride, SENT, dtype=w.dtype)
        full[:self.span] = w[lo:lo + self.span]
        full = full.reshape(self.n_str, self.stride)
        assert (full[:, self.L:] == SENT).all(), "row gap written"
        return full[:, :self.L]


class Side:
    """One source's host arrays, uploaded once: CSR (``counts`` None) or the counts layout; ``shift``: the ids start
    that many elements into their tensor (a 4-byte aligned ids pointer)."""

    def __init__(self, torch, ids, off, counts=None, status=None, shift=0):
        self.ids, self.off, self.counts, self.status = np.asarray(ids, dtype=np.int32), np.asarray(off, dtype=np.uint64), counts, status
        self.n_str = len(off) - 1
        self.d_ids = torch.zeros(max(len(ids), 1) + shift, dtype=torch.int32, device="cuda")
        self.d_ids[shift:shift + len(ids)] = torch.from_numpy(self.ids)
        self.ids_ptr = self.d_ids.data_ptr() + 4 * shift
        self.d_off = torch.from_numpy(self.off.view(np.int64)).cuda()
        self.d_cnt = None if counts is None else torch.from_numpy(np.asarray(counts, dtype=np.uint64).view(np.int64)).cuda()
        self.d_st = None if status is None else torch.from_numpy(np.asarray(status, dtype=np.int32)).cuda()

    def ptrs(self, status=True):
        return (self.ids_ptr, self.d_off.data_ptr(), self.d_cnt.data_ptr() if self.d_cnt is not None else 0,
                self.d_st.data_ptr() if status and self.d_st is not None else 0)

    def lists(self, status=True):
        """the side as collate_pair_ref takes it; a failed string's count is not handed over (it may be poison)"""
        st = None if not status or self.status is None else np.asarray(self.status).tolist()
        cnt = None if self.counts is None else [int(c) if not (st and st[s]) else 0 for s, c in enumerate(self.counts)]
        return self.ids.tolist(), [int(x) for x in self.off], cnt, st


def assert_equal(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        if g is None:
            continue
        w = np.array(w, dtype=np.int64).reshape(g.shape)
        assert g.dtype in (np.int32, np.int64)
        bad = np.argwhere(g != w)
        assert not len(bad), (what, "output %d" % k, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def random_batch(rng, counts, first=0, lo=0):
    """CSR (ids, off) of strings with the given token counts; off starts at ``first``; ids from ``lo`` up."""
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64) + np.uint64(first)
    ids = rng.integers(lo, lo + 50000, size=int(off[-1] - off[0]), dtype=np.int64).astype(np.int32)
    if len(ids) > 3:
        ids[1], ids[3] = -1, -2 ** 31
    return ids, off


def as_numpy(out, keys):
    """the tensors of a model-inputs dictionary named in ``keys`` as numpy arrays, None for one it does not hold"""
    return tuple(out[k].cpu().numpy() if k in out else None for k in keys)


def raw_reference(names):
    """vocab name -> (Encoder, ids, id_off, status) of the RAW corpus through the host path"""
    from dptok import Encoder, Vocab
    text, offs, _ = mc.form("raw")
    out = {}
    for name in names:
        enc = Encoder(Vocab(mc.vocabularies()[name], 0))
        ids, id_off, st, _ = enc.encode_csr(text, offs)
        out[name] = (enc, ids, id_off, st)
    return out


def _llama_fixture():
    from fake_llama import FakeLlamaTokenizer

    class Tok(FakeLlamaTokenizer):   # the fixture plus the special-token attributes of a transformers tokenizer
        bos_token_id, eos_token_id, pad_token_id = 1, 2, None

    t2i = mc.vocabularies()["base"]
    assert t2i["<s>"] == 1 and t2i["</s>"] == 2
    return Tok(t2i)
