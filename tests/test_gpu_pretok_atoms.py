"""dpt_pretok_write_atoms against the llama ATOMS model of tests/bpe_ref.py, byte for byte and between canaries: the
recorded SentencePiece texts, the strings on the kernel's 64-byte round edges, a literal "<0x41>" beside a
byte-fallback character -- and dpt_pretok_write on the same input unchanged.  Then the chain the feature is for:
text -> dpt_pretok_write_atoms -> dpt_bpe_encode equals the tokenizer's own encode."""
import numpy as np
import pytest

import bpe_ref
import pretok_ref as pr
import split_harness
from test_gpu_pretok import _pair, edge_length_strings

pytestmark = pytest.mark.gpu


class AtomsSide:
    """A Pretok whose write pass is dpt_pretok_write_atoms."""

    def __init__(self, pretok):
        self.sizes_device = pretok.sizes_device
        self.write_device = lambda *a: pretok.write_device(*a, atoms=True)


@pytest.fixture(scope="module")
def tables():
    return {"runs_ok": _pair(), "no_bos": _pair(bos="")}


def _check_both(pair, strings, **kw):
    pretok, table = pair
    want = split_harness.check(AtomsSide(pretok), lambda strs: bpe_ref.atoms(table, strs), strings, **kw)
    plain = split_harness.check(pretok, lambda strs: pr.presplit(table, strs), strings, **kw)   # the existing call: unchanged
    assert plain[2] == want[2] and bytes(c & 1 for c in want[3]) == plain[3]
    return want


def test_recorded_texts_and_round_edges(tables):
    from sp_llama import llama_texts
    strings = [t.encode("utf-8", "surrogatepass") for t in llama_texts()]
    st, ln, text2, cut = _check_both(tables["runs_ok"], strings)
    assert int((st == 0).sum()) > 250 and b"<0xF0><0x9F>" in text2 and set(cut) == {0, 2, 3}
    for which, kw in (("runs_ok", {}), ("no_bos", {"pad": 1, "off0": 0, "out0": 0})):
        st, _, _, _ = _check_both(tables[which], edge_length_strings(), **kw)
        assert not st.any()


def test_literal_byte_piece_beside_byte_fallback(tables):
    # '\n' and '~' are not in the known set: byte fallback; "<0x41>" typed in the text is six known characters
    strings = [b"<0x41>\n", b"a<0x0A>\n~<0x7E>", b"\n<0x0A>", b"x" * 60 + b"<0x41>\n<0x41>", "<0x41>é\n€".encode(), b"\n" * 70 + b"<0x0A>"]
    st, ln, text2, cut = _check_both(tables["runs_ok"], strings)
    assert not st.any()
    n0 = int(ln[0])
    assert text2[:n0] == "<s>▁<0x41><0x0A>".encode() and list(cut[:n0]) == [3, 0, 0, 3, 0, 0] + [2] * 6 + [2, 0, 0, 0, 0, 0]


def test_text_to_default_ids_on_the_device():
    import torch
    pytest.importorskip("sentencepiece")
    from dptok import Bpe, Pretok, Vocab, pack_strings
    from dptok.bpe import pairs_from_scores
    from sp_llama import SPLlama, llama_texts
    tok = SPLlama()
    sp, t2i = tok.sp, tok.get_vocab()
    n = sp.get_piece_size()
    exclude = [i for i in range(n) if sp.is_control(i) or sp.is_unknown(i) or sp.is_unused(i) or sp.is_byte(i)]
    bpe = Bpe(*pairs_from_scores(t2i, {sp.id_to_piece(i): sp.get_score(i) for i in range(n)}, exclude))
    vocab, pretok = Vocab(t2i, 0), Pretok(t2i, "<s>", ["<unk>", "<s>", "</s>"], 0)
    texts = llama_texts()
    text, offs = pack_strings(texts)
    text2, offs2, cut, pre = pretok.presplit(torch.from_numpy(text.copy()).cuda(), torch.from_numpy(offs.view(np.int64)).cuda(), atoms=True)
    ids, counts, status, words = bpe.encode_atoms(vocab, text2, offs2, cut, tok_word=True)
    pre, o, ids, counts, words = pre.cpu().numpy(), offs2.cpu().numpy(), ids.cpu().numpy(), counts.cpu().numpy(), words.cpu().numpy()
    assert int((pre == 0).sum()) == 292 and not status.cpu().numpy().any()
    for k, t in enumerate(texts):
        if pre[k] == 0:
            got = ids[o[k]:o[k] + counts[k]].tolist()
            assert got == tok.encode(t), t
            w = words[o[k]:o[k] + counts[k]]
            assert w[0] == 0 and (np.diff(w) >= 0).all() and int(w[-1]) == t.count(" ") + (1 if t else 0)
        else:
            assert counts[k] == 0 and o[k + 1] == o[k]
