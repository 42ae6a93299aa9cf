"""Drop-in for the reference's ``packages/tokenizer_utils.py`` (L2 adapters) backed by the
MI355X engine.  Same names, argument meaning and error behaviour:

* ``dp_tokenize_llama(llama_tokenizer, pretokenize_option='llama')`` -> ``(dp_tokenize,
  decode_dp_tokenization)`` (reference :52-96).  ``dp_tokenize(str) -> List[int]`` runs the
  per-word shortest-tokenization DP + longest-token selection on the GPU:
  - ``'raw'``: the pre-tokenizer runs inside the kernel (pretokenize_raw semantics, :33-50);
  - ``'llama'``: SentencePiece pieces from ``llama_tokenizer.encode`` are merged into words on
    the host (pretokenize_with_llama + merge_tokens, :7-31) and the GPU runs in pre-split mode.
  The DP call is the evident-intent 4-argument call; the shipped 5-argument call at :71 raises
  TypeError (SURVEY.md §0 finding 3), which this drop-in does not reproduce.
  Failures re-raise the reference's exceptions: a word with no tokenization -> ValueError
  (reference: ipdb.set_trace then max([]) at dp_tokenize.py:84), an empty word -> IndexError
  (dp_tokenize.py:49).  An unknown ``pretokenize_option`` fails at call time with NameError,
  like the reference's unbound ``pretokenize_func``.
* ``dp_tokenize_llama(llama_tokenizer, 'llama', device_pretokenize=True)``: the same pair with llama mode's
  pre-tokenization on the GPU (dptok/pretok.py; the rule: include/dpt.h dpt_pretok_create) for every string
  whose words are a per-character function of its text; the strings the rule does not certify go through the
  host path below as one sub-batch.  Same ids and exceptions; ``dp_tokenize.pretok_stats`` reads as
  (certified, sent to the host) of the last call.  Construction checks a probe list against the tokenizer object
  and raises DptError when a certified probe's words differ.  The default leaves the host path untouched.
* ``dp_tokenize_bloom(bloom_tokenizer, HF_CACHE_DIR, device_pretokenize=True)``: the BLOOM adapter with its words and
  atoms made on the GPU too (dptok/bytelevel.py; the rule: include/dpt.h dpt_bytelevel_create).  The rule is exact, so
  only text that is not well-formed UTF-8 goes through the host path; construction checks the pre-tokenizer's shape,
  the byte alphabet and a probe list, and raises DptError on the first difference.
* with ``device_pretokenize=True`` both adapters also carry ``dp_tokenize.batch_default(List[str])`` --
  ``[tokenizer.encode(t) for t in texts]`` with the certified strings pre-tokenized and BPE-merged on the GPU
  (dptok/bpe.py; include/dpt.h dpt_bpe_encode) -- and ``dp_tokenize.batch_compare(List[str])``, the lengths and per-word
  token counts of the shortest tokenization next to the default one (reference main_analyze_s2orc.py:269-297,
  main_biomed_translation.py:74-77); with ``words=True`` also which words improve and their tokens on both sides, found
  on the device (dptok/words.py; reference main_analyze_s2orc.py:277-290).  Construction checks a probe list against
  ``tokenizer.encode`` and leaves both off, with the reason in ``dp_tokenize.pretok_stats.default_off``, when they
  disagree.
* ``dp_tokenize.batch(List[str]) -> List[List[int]]``: the batched form (one GPU launch, in both
  modes).
* ``dp_tokenize.batch_spans(List[str]) -> List[TokenSpans]``: the batch's ids aligned to the text --
  per string ``(ids, offsets, word_ids, text)``: ``text`` is the string the engine tokenized (the input
  in raw mode, the concatenated pieces in llama mode, the concatenated atoms for BLOOM), ``offsets[k]``
  the (start, end) of token k in characters of ``text``, ``word_ids[k]`` the 0-based word it lies in
  (what the probe at reference main_analyze_s2orc.py:275-290 re-tokenizes every word to learn).  Same
  exceptions as ``batch``.
* ``dp_tokenize.batch_model_inputs(List[str], ...) -> dict``: the batch as padded ``input_ids`` /
  ``attention_mask`` / ``labels`` / ``lengths`` tensors on the GPU (dpt_encode_padded + dpt_collate; what
  reference main_analyze_s2orc.py:61-93 and the collator build on the host); see its docstring.
* ``dp_tokenize.batch_pair_model_inputs(sources, targets, ...) -> dict``: source + target rows as padded
  ``input_ids`` / ``attention_mask`` / ``labels`` tensors on the GPU (one dpt_encode_padded + one dpt_collate_pair;
  what reference main_biomed_translation.py:138-145 and its collator, :104-124, build on the host); see its docstring.
* ``dp_tokenize.batch_packed_inputs(List[str], max_length, ...) -> dict``: the batch packed in order into rows of
  ``max_length`` tokens on the GPU, with ``position_ids`` / ``segment_ids`` and every string's row and column
  (dpt_encode_padded + dpt_pack_sizes / dpt_pack_plan / dpt_pack_write); see its docstring.
* ``decode_dp_tokenization.batch(List[List[int]]) -> List[str]`` and ``dp_tokenize.batch_roundtrip(List[str])
  -> List[Optional[int]]``: the tokenizer's own decode of a batch, and the caller's round-trip assert
  (reference main_analyze_s2orc.py:84-87), each in one GPU launch; ``decode_dp_tokenization`` itself stays
  the tokenizer object's ``decode``.
* ``merge_tokens``, ``pretokenize_with_llama``, ``pretokenize_raw``: the reference's host-side
  string utilities with identical behaviour (pre-tokenization, not the DP).
"""
from __future__ import annotations

import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from dptok import Detok, DptError, Encoder, Vocab, raise_for_status  # noqa: E402
from dptok import _lib as _dpt  # noqa: E402
from dptok.engine import raise_and_collect as _raise_and_collect  # noqa: E402
from dptok.pack import (PieceTable, TokenSpans, _pack_id_lists, csr_token_spans, pack_presplit_words,  # noqa: E402
                        pack_strings, pack_word_atoms, presplit_outcome)
from dptok.hostpool import shared_pool  # noqa: E402

SPACE_TOKEN = "▁"


class _InverseDict(dict):
    """Minimal stand-in for ``bidict`` (reference uses ``.inverse``)."""

    @property
    def inverse(self):
        return {v: k for k, v in self.items()}


def merge_tokens(tokens, sep="Ġ"):
    """Join runs of pieces that do not start with ``sep`` (reference tokenizer_utils.py:7-22)."""
    merged_tokens = []
    i = 0
    n = len(tokens)
    while i < n:
        cur = tokens[i]
        while i + 1 < n and not tokens[i + 1].startswith(sep):
            cur = cur + tokens[i + 1]
            i += 1
        merged_tokens.append(cur)
        i += 1
    return merged_tokens


def pretokenize_with_llama(tokenizer, vocab_bidict):
    """SentencePiece pieces merged into words (reference tokenizer_utils.py:24-31)."""
    inverse = vocab_bidict.inverse

    def pretokenize(input_str):
        pieces = [inverse[t] for t in tokenizer.encode(input_str)]
        return merge_tokens(pieces, sep=SPACE_TOKEN)

    return pretokenize


def pretokenize_raw(manual_mapping) -> callable:
    """Raw character pre-tokenizer (reference tokenizer_utils.py:33-50): first char gets the
    '▁' prefix, ' ' opens a word as '▁', characters in ``manual_mapping.inverse`` are replaced
    (``'\\n' -> '<0x0A>'``).  The GPU engine applies the same rules in-kernel."""
    inverse = manual_mapping.inverse

    def pretokenize(input_str):
        atoms = list(input_str)
        words = []
        start = 0
        for i, ch in enumerate(atoms):
            if i == 0:
                atoms[i] = SPACE_TOKEN + ch
            elif ch == " ":
                atoms[i] = SPACE_TOKEN
                words.append(atoms[start:i])
                start = i
            elif ch in inverse:
                atoms[i] = inverse[ch]
        words.append(atoms[start:])
        return words

    return pretokenize


def _device() -> int:
    return int(os.environ.get("LOCAL_RANK", "0"))


def batch_encoder(tokenizer):
    """``texts -> [tokenizer.encode(t) for t in texts]``, in one call of the Rust backend when the
    tokenizer is a ``transformers`` tokenizers-backed class whose ``encode`` is the library's own:
    that ``encode`` is ``_encode_plus`` over a one-text batch -- ``set_truncation_and_padding`` with
    the default strategies, ``encode_special_tokens = split_special_tokens``, then
    ``_tokenizer.encode_batch([text], add_special_tokens=True)`` -- so one ``encode_batch_fast``
    over every text returns the same ids per text (tests/test_llama_sp.py checks it on every
    fixture), with the backend's threads.  Any other tokenizer object: its ``encode``, per text."""
    try:
        from transformers.tokenization_utils_base import PreTrainedTokenizerBase
        from transformers.tokenization_utils_tokenizers import TokenizersBackend
        from transformers.utils import PaddingStrategy
        from transformers.tokenization_utils_base import TruncationStrategy
    except ImportError:
        TokenizersBackend = None
    if (TokenizersBackend is not None and isinstance(tokenizer, TokenizersBackend)
            and type(tokenizer).encode is PreTrainedTokenizerBase.encode
            and type(tokenizer)._encode_plus is TokenizersBackend._encode_plus
            and hasattr(tokenizer._tokenizer, "encode_batch_fast")):
        fast = [True]   # (the private calls below are pinned on transformers 5.x; any other signature: per text)

        def encode_batch(texts):
            if fast[0]:
                try:
                    pad, trunc, max_len, _ = tokenizer._get_padding_truncation_strategies(padding=False, truncation=None,
                                                                                          max_length=None)
                    if pad == PaddingStrategy.DO_NOT_PAD and trunc == TruncationStrategy.DO_NOT_TRUNCATE:
                        tokenizer.set_truncation_and_padding(padding_strategy=pad, truncation_strategy=trunc,
                                                             max_length=max_len, stride=0, pad_to_multiple_of=None,
                                                             padding_side=None)
                        if tokenizer._tokenizer.encode_special_tokens != tokenizer.split_special_tokens:
                            tokenizer._tokenizer.encode_special_tokens = tokenizer.split_special_tokens
                        return [e.ids for e in tokenizer._tokenizer.encode_batch_fast(list(texts), add_special_tokens=True)]
                except (TypeError, AttributeError):
                    fast[0] = False   # from now on the library's public encode, per text
            return [tokenizer.encode(t) for t in texts]
        return encode_batch
    return lambda texts: [tokenizer.encode(t) for t in texts]


def _batch_spans(engine, texts, text, offs, mode, cut=None, none=None, outcome=None) -> List[TokenSpans]:
    """One encode + spans call over a packed batch -> a ``TokenSpans`` per string.  ``none[i]``: string i
    has no words (an empty result, whatever its status); ``outcome(status) -> (status, none)``: the
    statuses that decide the strings' exceptions, and ``none``, once the engine's are known.  Raises what
    ``dp_tokenize.batch`` raises, string by string in order, and DptError when a string's ids do not tile
    it (span status 4: never expected)."""
    ids, id_off, st, _, tok_end, tok_word, sst = engine.encode_csr_spans(text, offs, mode=mode, cut_mask=cut)
    out = csr_token_spans(text, offs, ids, id_off, tok_end, tok_word)
    if outcome is not None:
        st, none = outcome(st)
        none = none.tolist()
    stl, sstl = st.tolist(), sst.tolist()
    for i, t in enumerate(texts):
        if none is not None and none[i]:
            out[i] = TokenSpans([], [], [], "")
            continue
        raise_for_status(stl[i], t)
        if sstl[i] != _dpt.STATUS_OK:
            raise DptError("token spans: the ids do not tile the string (status %d) of %r" % (sstl[i], t[:60]))
    return out


_DECODE_BATCH_DOC = """``decode_dp_tokenization.batch(list of id lists) -> List[str]``: every list decoded on the
GPU in one launch, the bytes read as UTF-8 with ``errors="replace"``.  This is %s own decode of the ids.  A
``transformers`` tokenizer's ``decode`` -- what ``decode_dp_tokenization`` itself calls -- may render special
tokens and spacing differently: on the recorded llama-mode cases 83 of 565 differ for the ``transformers``
tokenizer, none for the SentencePiece one."""

_ROUNDTRIP_DOC = """``dp_tokenize.batch_roundtrip(texts) -> List[Optional[int]]``: the encode exactly as ``batch`` (same
exceptions, in the same order), then ONE round-trip launch against the original texts -- the caller's
``decode_dp_tokenization(dp_tokenize(x)) == x`` (reference main_analyze_s2orc.py:84-87) for the batch.  Per
string None when the decode equals the text, else the first differing byte offset of its UTF-8."""


def _bos_id(tokenizer) -> Optional[int]:
    """The tokenizer's BOS id when it has one: its ``bos_token_id``, else the one id it puts in front of
    the empty string (the SentencePiece wrappers without that attribute)."""
    bos = getattr(tokenizer, "bos_token_id", None)
    if bos is None:
        try:
            e = list(tokenizer.encode(""))
        except Exception:
            return None
        bos = e[0] if len(e) == 1 else None
    return None if bos is None else int(bos)


def _decode_surface(make_detok, strip, encode_many):
    """The batch calls over one lazily built ``Detok`` (the table is built and uploaded at the first call):
    ``decode_batch(list of id lists) -> List[str]`` and ``batch_roundtrip(texts) -> List[Optional[int]]``."""
    box = []

    def detok():
        if not box:
            box.append(make_detok())
        return box[0]

    def decode_batch(id_lists) -> List[str]:
        id_lists = list(id_lists)
        ids, id_off = _pack_id_lists(id_lists)
        raw, out_off, st = detok().decode_csr(ids, id_off, strip_space=strip)
        bad = np.flatnonzero(st)
        if len(bad):
            raise DptError("decode: string %d has an id outside the vocabulary" % int(bad[0]))
        blob, o = raw.tobytes(), out_off.tolist()
        return [blob[o[s]:o[s + 1]].decode("utf-8", "replace") for s in range(len(id_lists))]

    def batch_roundtrip(texts) -> List[Optional[int]]:
        texts = list(texts)
        id_lists = encode_many(texts)   # the encode exactly as ``batch`` does it, with its exceptions
        ids, id_off = _pack_id_lists(id_lists)
        text, offs = pack_strings(texts)
        rt, fd = detok().roundtrip_csr(text, offs, ids, id_off, strip_space=strip)
        bad = np.flatnonzero((rt != _dpt.RT_EQUAL) & (rt != _dpt.RT_DIFFERS))
        if len(bad):
            raise DptError("round trip: string %d has an id outside the vocabulary (status %d)" % (int(bad[0]), int(rt[bad[0]])))
        return [None if v == _dpt.RT_EQUAL else d for v, d in zip(rt.tolist(), fd.tolist())]

    return decode_batch, batch_roundtrip


_MODEL_INPUTS_DOC = """``dp_tokenize.batch_model_inputs(texts, max_length=None, padding="longest", pad_to_multiple_of=None,
add_bos=False, add_eos=False, padding_side="right", truncation_side="right", labels=False, errors="raise") -> dict``:
the batch as model inputs on the GPU -- what the reference's llama_preprocessing_function (main_analyze_s2orc.py:
61-93) and the Trainer's collator build on the host.  The packed text goes up, dpt_encode_padded and dpt_collate
run back to back, and nothing comes back but the statuses (and, for ``padding="longest"``, the row length).
``input_ids`` / ``attention_mask`` (/ ``labels``, pad positions -100) are int64 ``[len(texts), row]`` tensors on the
engine's device, ``lengths`` int32 per string.  The row is the longest sequence capped by ``max_length``
(``padding="max_length"``: exactly ``max_length``), rounded up to ``pad_to_multiple_of``.  The pad id is the
tokenizer's ``pad_token_id``, else its ``eos_token_id``, else 0; ``add_bos`` / ``add_eos`` put its BOS / EOS id
around the kept ids (in llama mode the BOS piece ``tokenizer.encode`` adds is already a word of the text).
``errors="raise"``: what ``dp_tokenize.batch`` raises, for the first failed string in order; ``"mask"``: a
failed string's row is all pad with mask 0 and length 0, and ``status`` (int32 per string) is returned too."""


_PAIR_INPUTS_DOC = """``dp_tokenize.batch_pair_model_inputs(sources, targets, max_length=None, padding="longest",
pad_to_multiple_of=None, max_source=None, max_target=None, add_bos=False, sep_id=None, add_eos=False, labels=True,
mask_source=False, token_type_ids=False, trim="target", ignore_id=None, padding_side="right", truncation_side="right",
errors="raise") -> dict``: source + target rows as model inputs on the GPU -- what the reference's translation driver
builds with apply_tokenizer (main_biomed_translation.py:138-145) and ShortcutDataCollatorForSeq2Seq (:104-124).
``sources + targets`` go up as one packed batch, one dpt_encode_padded and one dpt_collate_pair run back to back (the
targets are the same buffers from string ``len(sources)`` on), and nothing comes back but the statuses (and, for
``padding="longest"``, the row length).  Row i is ``[bos] + source i + [sep] + target i + [eos]``; the defaults are the
reference collator's tensors: no specials, right padding to the longest pair, int64, ``labels`` equal to the padded
``input_ids`` (``ignore_id`` None: the pad id).  ``max_source`` / ``max_target`` cap a side's ids; a row longer than
``max_length`` loses ids of ``trim`` ("target" or "source") first.  ``mask_source``: the labels are ``ignore_id`` on the
source (pass e.g. ``ignore_id=-100``); ``token_type_ids``: 0 on the source, 1 on the target.  Also returned: ``lengths``
and ``b_start`` (the column of the target's first position), int32 per row.  ``errors="raise"``: what
``dp_tokenize.batch`` raises, for the first failed string in row order, a row's source before its target; ``"mask"``:
a row with a failed side is all pad, and ``status_source`` / ``status_target`` (int32 per row) are returned too.
ValueError when the two lists differ in length."""


_PACKED_INPUTS_DOC = """``dp_tokenize.batch_packed_inputs(texts, max_length, add_bos=False, add_eos=False, labels=False,
mask_first=False, truncation_side="right", errors="raise") -> dict``: the batch packed into rows of ``max_length``
tokens on the GPU -- consecutive strings share a row, in order, no sequence split (include/dpt.h dpt_pack_plan has the
rule).  The packed text goes up, dpt_encode_padded and the three packing calls run back to back, and nothing comes
back but the statuses and the number of rows.  ``input_ids`` / ``position_ids`` / ``segment_ids`` (/ ``labels``, pad
positions -100) are int64 ``[n_rows, max_length]`` tensors on the engine's device: the position of a token inside its own
sequence, and per row 1, 2, ... per sequence with 0 at pad (the attention mask is ``segment_ids != 0``; sequences of a
row must not attend to each other).  ``mask_first``: the labels are -100 on the first token of every sequence.  Also
returned: ``lengths``, ``str_row``, ``str_col`` (int32 per string; ``str_row`` -1: the string holds no token and is not
placed), ``row_first``, ``row_fill`` (int32 per row) and ``n_rows``.  A string longer than ``max_length`` is truncated as
in ``batch_model_inputs``; the pad id and ``add_bos`` / ``add_eos`` are that call's too.  ``errors="raise"``: what
``dp_tokenize.batch`` raises, for the first failed string in order; ``"mask"``: a failed string is not placed, and
``status`` (int32 per string) is returned too."""


def _special_ids(tokenizer):
    """(bos, eos, pad) ids of a tokenizer object: bos / eos None when it has none; pad is its ``pad_token_id``,
    else its ``eos_token_id``, else 0."""
    eos = getattr(tokenizer, "eos_token_id", None)
    pad = getattr(tokenizer, "pad_token_id", None)
    eos = None if eos is None else int(eos)
    return _bos_id(tokenizer), eos, int(pad) if pad is not None else eos if eos is not None else 0


def _model_inputs_surface(engine, tokenizer, pack_batch):
    """(``batch_model_inputs``, ``batch_pair_model_inputs``, ``batch_packed_inputs``) over one adapter's packing: ``pack_batch(texts) -> (text, offs, mode, cut, none,
    outcome)``, the buffers of its ``batch`` call with ``none`` / ``outcome`` as ``_batch_spans`` takes them."""

    def encode_padded(texts):
        """One dpt_encode_padded over the adapter's packing of ``texts`` -> (dev, ids, d_offs, st, counts, offs): the
        device tensors ``model_inputs`` takes (st and counts of len(texts) entries, the statuses fixed up as ``batch``
        sees them) and the host offsets."""
        import torch
        text, offs, mode, cut, none, outcome = pack_batch(texts)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n, b0 = len(offs) - 1, int(offs[0])
        n_bytes = int(offs[-1]) - b0
        dev = torch.device("cuda", engine.vocab.device)

        def up(a):   # the batch's bytes (at least one, so the tensor has an address)
            a = np.ascontiguousarray(a, dtype=np.uint8)[b0:b0 + n_bytes]
            if not n_bytes or not a.flags.writeable:   # (torch wraps writable arrays only)
                a = a.copy() if n_bytes else np.zeros(1, dtype=np.uint8)
            return torch.from_numpy(a).to(dev)

        with torch.cuda.device(dev):
            d_text, d_cut = up(text), (up(cut) if cut is not None else None)
            d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
            ids = torch.empty(max(n_bytes, 1), dtype=torch.int32, device=dev)
            counts = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
            st = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            if n:
                engine.encode_device_padded(d_text.data_ptr(), n_bytes, d_offs.data_ptr(), n, ids.data_ptr(), max(n_bytes, 1),
                                            counts.data_ptr(), st.data_ptr(), cut_ptr=d_cut.data_ptr() if d_cut is not None else 0,
                                            stream=torch.cuda.current_stream(dev).cuda_stream, mode=mode)
            st = st[:n]
            if outcome is not None:   # (the word-list packing: the statuses depend on the engine's, read back)
                fixed, none = outcome(st.cpu().numpy())
                st = torch.from_numpy(np.ascontiguousarray(fixed, dtype=np.int32)).to(dev)
            if none is not None and n:   # strings without words: nothing, whatever the engine made of them
                d_none = torch.from_numpy(np.ascontiguousarray(none, dtype=bool)).to(dev)
                st = st.masked_fill(d_none, _dpt.STATUS_OK)
                counts = counts[:n].masked_fill(d_none, 0)
        return dev, ids, d_offs, st, counts[:n].contiguous(), offs

    def checked_specials(errors, add_bos, add_eos):
        """the prelude of both calls: ``errors`` checked, and the tokenizer's (bos, eos, pad) ids with those asked for present"""
        if errors not in ("raise", "mask"):
            raise ValueError("errors must be 'raise' or 'mask'")
        bos, eos, pad = _special_ids(tokenizer)
        if (add_bos and bos is None) or (add_eos and eos is None):
            raise ValueError("the tokenizer has no %s id to add" % ("BOS" if add_bos and bos is None else "EOS"))
        return bos, eos, pad

    def batch_model_inputs(texts, max_length=None, padding="longest", pad_to_multiple_of=None, add_bos=False,
                           add_eos=False, padding_side="right", truncation_side="right", labels=False, errors="raise"):
        import torch
        from dptok.collate import model_inputs
        bos, eos, pad = checked_specials(errors, add_bos, add_eos)
        texts = list(texts)
        dev, ids, d_offs, st, counts, _ = encode_padded(texts)
        with torch.cuda.device(dev):
            out = model_inputs(ids, d_offs, st, counts, padding=padding, max_length=max_length,
                               pad_to_multiple_of=pad_to_multiple_of, labels=labels, pad_id=pad,
                               bos_id=bos if add_bos else None, eos_id=eos if add_eos else None,
                               padding_side=padding_side, truncation_side=truncation_side)
            if errors == "mask":
                out["status"] = st
                return out
            for i in np.flatnonzero(st.cpu().numpy()).tolist()[:1]:
                raise_for_status(int(st[i]), texts[i])
        return out

    def batch_pair_model_inputs(sources, targets, max_length=None, padding="longest", pad_to_multiple_of=None,
                                max_source=None, max_target=None, add_bos=False, sep_id=None, add_eos=False, labels=True,
                                mask_source=False, token_type_ids=False, trim="target", ignore_id=None,
                                padding_side="right", truncation_side="right", errors="raise"):
        import torch
        from dptok.collate import pair_model_inputs
        bos, eos, pad = checked_specials(errors, add_bos, add_eos)
        sources, targets = list(sources), list(targets)
        if len(sources) != len(targets):
            raise ValueError("%d sources for %d targets" % (len(sources), len(targets)))
        n = len(sources)
        dev, ids, d_offs, st, counts, offs = encode_padded(sources + targets)
        first_b = int(offs[n] - offs[0])   # side B: the same buffers from string n on (its ids start at str_off[n])
        with torch.cuda.device(dev):
            out = pair_model_inputs((ids, d_offs[:n + 1], st[:n], counts[:n]), (ids[first_b:], d_offs[n:], st[n:], counts[n:]),
                                    padding=padding, max_length=max_length, pad_to_multiple_of=pad_to_multiple_of,
                                    max_source=max_source, max_target=max_target, labels=labels, mask_source=mask_source,
                                    token_type_ids=token_type_ids, trim=trim, pad_id=pad, bos_id=bos if add_bos else None,
                                    sep_id=sep_id, eos_id=eos if add_eos else None,
                                    ignore_id=pad if ignore_id is None else ignore_id, padding_side=padding_side,
                                    truncation_side=truncation_side)
            if errors == "mask":
                out["status_source"], out["status_target"] = st[:n], st[n:]
                return out
            st_h = st.cpu().numpy()
            for i in np.flatnonzero(st_h[:n] | st_h[n:]).tolist()[:1]:   # sources before targets of the same row
                if st_h[i]:
                    raise_for_status(int(st_h[i]), sources[i])
                raise_for_status(int(st_h[n + i]), targets[i])
        return out

    def batch_packed_inputs(texts, max_length, add_bos=False, add_eos=False, labels=False, mask_first=False,
                            truncation_side="right", errors="raise"):
        import torch
        from dptok.packing import packed_inputs
        bos, eos, pad = checked_specials(errors, add_bos, add_eos)
        texts = list(texts)
        dev, ids, d_offs, st, counts, _ = encode_padded(texts)
        with torch.cuda.device(dev):
            out = packed_inputs(ids, d_offs, st, counts, max_length=max_length, labels=labels, mask_first=mask_first, pad_id=pad,
                                bos_id=bos if add_bos else None, eos_id=eos if add_eos else None,
                                truncation_side=truncation_side)
            if errors == "mask":
                out["status"] = st
                return out
            for i in np.flatnonzero(st.cpu().numpy()).tolist()[:1]:
                raise_for_status(int(st[i]), texts[i])
        return out

    batch_model_inputs.__doc__ = _MODEL_INPUTS_DOC
    batch_pair_model_inputs.__doc__ = _PAIR_INPUTS_DOC
    batch_packed_inputs.__doc__ = _PACKED_INPUTS_DOC
    return batch_model_inputs, batch_pair_model_inputs, batch_packed_inputs


def _finish_adapter(dp_tokenize, decode_dp_tokenization, engine, encode_many, spans_many, inputs_surface, decode_batch,
                    batch_roundtrip, whose, **extra):
    """Hang the batch calls, the engine and ``extra`` on the two closures of an adapter and return the pair;
    ``whose``: the decode that ``decode_batch`` is (for its docstring)."""
    decode_batch.__doc__ = _DECODE_BATCH_DOC % whose
    batch_roundtrip.__doc__ = _ROUNDTRIP_DOC
    decode_dp_tokenization.batch = decode_batch
    dp_tokenize.batch_roundtrip = batch_roundtrip
    dp_tokenize.batch = encode_many
    dp_tokenize.batch_spans = spans_many
    dp_tokenize.batch_model_inputs, dp_tokenize.batch_pair_model_inputs, dp_tokenize.batch_packed_inputs = inputs_surface
    dp_tokenize.engine = engine
    for name, value in extra.items():
        setattr(dp_tokenize, name, value)
    return dp_tokenize, decode_dp_tokenization


class PretokStats:
    """``dp_tokenize.pretok_stats``: of the last batch call, the strings the device rule certified and the
    strings sent through the host tokenizer.  Reads as the tuple (certified, sent_to_host).  ``default_off``: None
    when ``dp_tokenize.batch_default`` / ``batch_compare`` are on, else why construction left them off."""

    def __init__(self):
        self.certified = self.sent_to_host = 0
        self.default_off = None

    def set(self, certified: int, sent_to_host: int) -> None:
        self.certified, self.sent_to_host = int(certified), int(sent_to_host)

    def __iter__(self):
        return iter((self.certified, self.sent_to_host))

    def __eq__(self, other):
        return tuple(self) == tuple(other)

    def __repr__(self):
        return "PretokStats(certified=%d, sent_to_host=%d)" % tuple(self)


def _pretok_literals(tokenizer, t2i) -> List[str]:
    """The strings a tokenizer object may treat specially inside a text -- the device rule refuses a text
    that holds one: its ``all_special_tokens``, its added vocabulary, the pieces of its BOS / EOS / UNK / PAD
    ids, and every vocabulary piece that reads as a control symbol (``<...>`` other than a byte piece
    ``<0xNN>``; a SentencePiece processor wrapped without those attributes has its ``<unk>``, ``<s>``,
    ``</s>`` only there)."""
    inverse = {i: t for t, i in t2i.items()}
    out = [t for t in (getattr(tokenizer, "all_special_tokens", None) or []) if isinstance(t, str)]
    added = getattr(tokenizer, "get_added_vocab", None)
    if callable(added):
        out += list(added())
    ids = [_bos_id(tokenizer)] + [getattr(tokenizer, a, None) for a in ("eos_token_id", "unk_token_id", "pad_token_id")]
    out += [inverse[int(i)] for i in ids if i is not None and int(i) in inverse]
    out += [t for t in t2i if len(t) >= 3 and t[0] == "<" and t[-1] == ">" and not (len(t) == 6 and t.startswith("<0x"))]
    return [t for t in dict.fromkeys(out) if t]


def _device_split_paths(split, mode, engine, host_pack):
    """The batch paths of an adapter whose pre-tokenization runs on the device.  ``split(d_text, d_offs)`` -> device
    (text2, offs2 int64[n + 1], cut, pre_status): ``Pretok.presplit`` or ``ByteLevelSplit.split``;  ``host_pack(texts)``
    -> the host path's (text, offs, cut, cnt) for ``mode``, cnt[i] == 0: string i has no words.  The strings the
    device refuses (pre_status 6) go through ``host_pack`` as one sub-batch and are merged back by index.
    -> (presplit, encode_many, spans_many, pack_batch, stats): ``presplit`` for ``_probe_check``, the next three what
    the adapter hangs on its closure in place of the host path's, ``stats`` its ``pretok_stats``."""
    import torch
    from dptok._lib import PRETOK_NEEDS_HOST as NEEDS_HOST
    from dptok.engine import csr_lists

    dev = torch.device("cuda", _device())
    stats = PretokStats()

    def presplit(texts):
        """-> device (text2, offs2 int64[n + 1], cut, pre_status) and the refused strings' indices (host)."""
        text, offs = pack_strings(texts)
        with torch.cuda.device(dev):
            d_text = torch.from_numpy(text.copy()).to(dev)
            d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
            text2, offs2, cut, pre = split(d_text, d_offs)
        pre_h = pre.cpu().numpy()
        refused = np.flatnonzero(pre_h == NEEDS_HOST)
        stats.set(len(texts) - len(refused), len(refused))
        return text2, offs2, cut, refused

    def encode_csr_lists(texts):
        """Per string (ids, status), as the host path's one launch over ``host_pack(texts)`` gives them."""
        n = len(texts)
        if n == 0:
            stats.set(0, 0)
            return []
        text2, offs2, cut, refused = presplit(texts)
        n2 = int(text2.numel())
        with torch.cuda.device(dev):
            ids = torch.empty(max(n2, 1), dtype=torch.int32, device=dev)
            id_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            st = torch.empty(n, dtype=torch.int32, device=dev)
            engine.encode_device(text2.data_ptr(), n2, offs2.data_ptr(), n, ids.data_ptr(), max(n2, 1), id_off.data_ptr(),
                                 st.data_ptr(), cut_ptr=cut.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream,
                                 mode=mode)
            id_off_h = id_off.cpu().numpy().view(np.uint64)
            ids_h = ids[:int(id_off_h[-1])].cpu().numpy()
            st_h = st.cpu().numpy()
            none = (torch.diff(offs2) == 0).cpu().numpy()   # nothing to tokenize (and every refused string)
        out = csr_lists(ids_h, id_off_h, st_h, none=none, keep_failed=False)
        if len(refused):
            text, offs, cutm, cnt = host_pack([texts[i] for i in refused.tolist()])
            h_ids, h_off, h_st, _ = engine.encode_csr(text, offs, mode=mode, cut_mask=cutm)
            sub = csr_lists(h_ids, h_off, h_st, none=(np.asarray(cnt) == 0), keep_failed=False)
            for i, r in zip(refused.tolist(), sub):
                out[i] = r
        return out

    def pack_merged(texts):
        """``host_pack(texts)``'s arrays (text, offs, cut, words per string -- here 0 or 1 for the strings made on the
        device: only its being 0 is read) with every string the device takes made there."""
        n = len(texts)
        if n == 0:
            stats.set(0, 0)
            return host_pack(texts)
        text2, offs2, cut, refused = presplit(texts)
        t2, c2, o2 = text2.cpu().numpy(), cut.cpu().numpy(), offs2.cpu().numpy()
        lens = np.diff(o2)
        cnt = (lens > 0).astype(np.int64)
        if not len(refused):
            return np.append(t2, np.uint8(0)), o2.astype(np.uint64), np.append(c2, np.uint8(0)), cnt
        ht, ho, hc, hcnt = host_pack([texts[i] for i in refused.tolist()])
        ho = ho.astype(np.int64)
        lens[refused] = np.diff(ho)
        cnt[refused] = hcnt
        offs = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=offs[1:])
        text = np.zeros(int(offs[-1]) + 1, dtype=np.uint8)
        cutm = np.zeros(int(offs[-1]) + 1, dtype=np.uint8)
        # the device's strings keep their order among themselves, and so do the refused ones: two masked copies
        sid = np.repeat(np.arange(n), lens)
        from_host = np.zeros(n, dtype=bool)
        from_host[refused] = True
        m = from_host[sid]
        text[:-1][m], cutm[:-1][m] = ht[:int(ho[-1])], hc[:int(ho[-1])]
        text[:-1][~m], cutm[:-1][~m] = t2, c2
        return text, offs.astype(np.uint64), cutm, cnt

    def encode_many(texts: Sequence[str]) -> List[List[int]]:
        texts = list(texts)
        return _raise_and_collect(texts, encode_csr_lists(texts))

    def spans_many(texts: Sequence[str]) -> List[TokenSpans]:
        texts = list(texts)
        text, offs, cut, cnt = pack_merged(texts)
        return _batch_spans(engine, texts, text, offs, mode, cut, none=(cnt == 0).tolist())

    def pack_batch(texts):
        text, offs, cut, cnt = pack_merged(list(texts))
        return text, offs, mode, cut, cnt == 0, None

    return presplit, encode_many, spans_many, pack_batch, stats


def _probe_check(presplit, stats, probes, host_words, bit, skip_refused, not_for):
    """The self-check of a device rule at construction: every probe's words out of ``presplit`` (``bit``: the bits
    of the cut mask that open a word) against ``host_words(probe)``, the tokenizer's.  DptError on the first
    difference; a probe the rule refuses is left out when ``skip_refused`` (the rule certifies only some texts) and is
    a difference otherwise (the rule is exact)."""
    for probe, words in zip(probes, _presplit_words(presplit, probes, bit)):
        if (words is not None or not skip_refused) and words != host_words(probe):
            raise DptError("device_pretokenize: the device rule gives %r for the probe %r, the tokenizer %r: this %s"
                           % (words, probe, host_words(probe), not_for))
    stats.set(0, 0)


def _device_pretokenizer(tokenizer, t2i, engine, host, merge_words):
    """llama mode with the pre-tokenization on the device (dptok/pretok.py; the rule: include/dpt.h
    dpt_pretok_create) -> (encode_many, spans_many, pack_batch, stats): the strings the rule certifies never see the
    tokenizer object, the others (pre_status 6) go through ``host.pack`` as one sub-batch and are merged back
    by index.  Construction runs the probe list through both and raises DptError on the first certified probe
    whose words differ: the guard for tokenizers the rule was not pinned on."""
    from dptok.pretok import Pretok
    from dptok.pretok_probes import PROBES

    bos = _bos_id(tokenizer)
    inverse = {i: t for t, i in t2i.items()}
    if bos is not None and bos not in inverse:
        raise DptError("device_pretokenize: the BOS id %d has no piece" % bos)
    literals = _pretok_literals(tokenizer, t2i)
    pretok = Pretok(t2i, inverse[bos] if bos is not None else "", literals, _device())
    presplit, *paths, stats = _device_split_paths(pretok.presplit, "presplit", engine, host.pack)
    stats.split_atoms = lambda d_text, d_offs: pretok.presplit(d_text, d_offs, atoms=True)   # (_default_surface)
    stats.dp_form = (pretok.presplit, "presplit")
    _probe_check(presplit, stats, PROBES, merge_words, 0xFF, True,
                 "tokenizer is not one the rule holds for (a normalising model, other added-token behaviour)")
    return (*paths, stats)


def _default_surface(dp_tokenize, tokenizer, split_atoms, make_table, bpe_vocab, probes, empty_ids, host_only, stats,
                     dp_form, dp_pieces, default_pieces):
    """``dp_tokenize.batch_default`` and ``dp_tokenize.batch_compare``: the tokenizer's own ids made on the device
    (dptok/bpe.py; the rule: include/dpt.h dpt_bpe_encode) next to the shortest tokenization -- the comparison the
    reference drivers exist for (main_analyze_s2orc.py:269-297, main_biomed_translation.py:74-77).

    ``split_atoms(d_text, d_offs)`` -> the device ATOMS form (text2, offs2, cut, pre_status); ``make_table()`` -> the
    pair table's four arrays by the route the tokenizer object offers; ``bpe_vocab`` the ``Vocab`` whose ids are the
    tokenizer's; ``host_only(text)``: the text must go to the host tokenizer whatever the device rule says.
    ``dp_form`` = (split, mode): ``split(d_text, d_offs)`` -> the device form the DP runs on and its engine mode -- the
    same text as ``split_atoms``' with the words starting at the same bytes; ``dp_pieces`` / ``default_pieces``: id ->
    token string of the DP's and of the tokenizer's ids (``batch_compare(words=True)``).
    Construction runs ``probes`` through ``batch_default`` against ``tokenizer.encode``; when they disagree, when
    ``tokenizer.encode("")`` is not ``empty_ids`` or when the table cannot be built, both attributes stay off and
    ``stats.default_off`` says why (None: they are on)."""
    import torch
    from dptok.bpe import Bpe

    dev = torch.device("cuda", _device())
    stats.default_off = None

    def host_encode(text):
        return [int(i) for i in tokenizer.encode(text)]

    def device_default(texts, want_words):
        """Per string the default ids (None: the device does not take it) and, with want_words, their word indices."""
        ids_out: List[Optional[List[int]]] = [None] * len(texts)
        words_out: List[Optional[np.ndarray]] = [None] * len(texts)
        take = [i for i, t in enumerate(texts) if not host_only(t)]
        if not take:
            return ids_out, words_out
        text, offs = pack_strings([texts[i] for i in take])
        with torch.cuda.device(dev):
            text2, offs2, cut, pre = split_atoms(torch.from_numpy(text.copy()).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev))
            ids, counts, status, words = bpe.encode_atoms(bpe_vocab, text2, offs2, cut, tok_word=want_words)
            ids_h, cnt_h, st_h, pre_h, o = (x.cpu().numpy() for x in (ids, counts, status, pre, offs2))
            words_h = words.cpu().numpy() if want_words else None
        for k, i in enumerate(take):
            if pre_h[k] == 0 and st_h[k] == 0:
                a, c = int(o[k]), int(cnt_h[k])
                ids_out[i] = ids_h[a:a + c].tolist()
                if want_words:
                    words_out[i] = words_h[a:a + c]
        return ids_out, words_out

    def batch_default(texts: Sequence[str]) -> List[List[int]]:
        """``[tokenizer.encode(t) for t in texts]``: the strings the device rules certify are pre-tokenized and merged
        on the GPU (two pre-tokenization kernels and dpt_bpe_encode), the others go to the host tokenizer."""
        texts = list(texts)
        got, _ = device_default(texts, False)
        return [g if g is not None else host_encode(t) for g, t in zip(got, texts)]

    def device_words(texts):
        """Per string the words with fewer DP tokens than default tokens, found on the device (dptok/words.py): (their
        indices, their DP ids word by word, their default ids word by word), or None for a string the device does not
        take.  Both encodings, the spans and the comparison run back to back on the two device forms of the batch;
        only the per-string sizes, the selected words' records and their gathered ids come back."""
        from dptok import words as wcmp
        from dptok._lib import STATUS_INTERNAL
        out = [None] * len(texts)
        take = [i for i, t in enumerate(texts) if not host_only(t)]
        if not take:
            return out
        text, offs = pack_strings([texts[i] for i in take])
        n, engine = len(take), dp_tokenize.engine
        split_dp, dp_mode = dp_form
        with torch.cuda.device(dev):
            d_text, d_offs = torch.from_numpy(text.copy()).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev)
            text_b, offs_b, cut_b, pre_b = split_atoms(d_text, d_offs)
            text_a, offs_a, cut_a, pre_a = (text_b, offs_b, cut_b, pre_b) if split_dp == split_atoms else split_dp(d_text, d_offs)
            nb = int(text_a.numel())
            if nb != int(text_b.numel()):
                raise DptError("batch_compare: the two device forms of the batch differ in length")
            stream = torch.cuda.current_stream(dev).cuda_stream
            ids, tok_end, tok_word = (torch.empty(max(nb, 1), dtype=torch.int32, device=dev) for _ in range(3))
            id_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            st, sst = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
            text_ptr, cut_ptr = (text_a.data_ptr(), cut_a.data_ptr()) if nb else (ids.data_ptr(), ids.data_ptr())
            engine.encode_device(text_ptr, nb, offs_a.data_ptr(), n, ids.data_ptr(), max(nb, 1), id_off.data_ptr(), st.data_ptr(),
                                 cut_ptr=cut_ptr, stream=stream, mode=dp_mode)
            engine.spans_device(text_ptr, nb, offs_a.data_ptr(), n, ids.data_ptr(), id_off.data_ptr(), st.data_ptr(), tok_end.data_ptr(),
                                sst.data_ptr(), tok_word_ptr=tok_word.data_ptr(), cut_ptr=cut_ptr, stream=stream, mode=dp_mode)
            b_ids, b_cnt, b_st, b_word = bpe.encode_atoms(bpe_vocab, text_b, offs_b, cut_b, tok_word=True)
            # a refused string keeps its pre-tokenization status; one with nothing to tokenize has no words on either side
            nothing = torch.diff(offs_a) == 0
            st_a = torch.where(pre_a != 0, pre_a, torch.where(nothing, torch.zeros_like(sst), sst))
            st_b = torch.where(pre_b != 0, pre_b, b_st)
            r = wcmp.compare_device(wcmp.Side(id_off, tok_word, status=st_a, tok_end=tok_end),
                                    wcmp.Side(offs_b, b_word, counts=b_cnt, status=st_b), wcmp.WORDS_LESS)
            a_sel, a_off = wcmp.selected_ids(ids, id_off, None, r.sel_str, r.sel_a_first, r.sel_a_count)
            b_sel, b_off = wcmp.selected_ids(b_ids, offs_b, b_cnt, r.sel_str, r.sel_b_first, r.sel_b_count)
            status, sel_off, sel_word, a_sel, a_off, b_sel, b_off = (x.cpu().numpy() for x in (r.status, r.sel_off, r.sel_word, a_sel, a_off,
                                                                                                b_sel, b_off))
        if (status == STATUS_INTERNAL).any():
            k = int(np.flatnonzero(status == STATUS_INTERNAL)[0])
            raise DptError("batch_compare: the two tokenizations of %r do not number the same words" % texts[take[k]][:60])
        a_sel, b_sel, sel_word, so, ao, bo = a_sel.tolist(), b_sel.tolist(), sel_word.tolist(), sel_off.tolist(), a_off.tolist(), b_off.tolist()
        for k, i in enumerate(take):
            if status[k] == 0:
                q = range(so[k], so[k + 1])
                out[i] = (sel_word[so[k]:so[k + 1]], [a_sel[ao[d]:ao[d + 1]] for d in q], [b_sel[bo[d]:bo[d + 1]] for d in q])
        return out

    def batch_compare(texts: Sequence[str], words: bool = False, pack_length: Optional[int] = None) -> dict:
        """The shortest tokenization against the tokenizer's own, per string: ``dp_lengths`` and ``default_lengths``
        (int64 arrays: the ``len`` of ``dp_tokenize.batch`` and of ``tokenizer.encode``), ``improved`` (the mask
        dp < default), and ``dp_word_counts`` / ``default_word_counts``: per string the tokens in each word of its
        pre-tokenization (bincounts of the word index of every token; the default side's is None for a string that went
        to the host tokenizer).  The reference's per-word step re-encodes each word as a text of its own, which adds a
        BOS and a dummy prefix to both sides; here the words are compared in place, inside their string.

        ``words=True`` adds, per string, the words the shortest tokenization improves -- the reference's per-word step
        (main_analyze_s2orc.py:277-290) for the whole batch, found on the device by one streaming comparison of the two
        word-index streams: ``improved_word_ids`` (the words with fewer DP tokens than default tokens, ascending),
        ``improved_tokens`` (per improved word the DP's token strings) and ``worse_tokens`` (the default's, of the same
        words) -- the reference frame's two columns, ``[]`` for a string without an improved word and None for a string
        that went to the host tokenizer on either side.  Every other key holds what it holds without it.

        ``pack_length=L`` adds ``dp_rows`` and ``default_rows``: the rows of L tokens each side's lengths pack into, in
        order and without splitting a sequence (dptok/packing.py ``plan_lengths``; a sequence longer than L counts as L
        tokens, as truncated) -- what a shorter tokenization saves a training loop that packs its batches."""
        texts = list(texts)
        spans = dp_tokenize.batch_spans(texts)
        got, default_words = device_default(texts, True)
        default = [g if g is not None else host_encode(t) for g, t in zip(got, texts)]
        dp_len = np.array([len(s.ids) for s in spans], dtype=np.int64)
        df_len = np.array([len(d) for d in default], dtype=np.int64)
        dp_words = [np.bincount(np.asarray(s.word_ids, dtype=np.int64)) if s.word_ids else np.zeros(0, dtype=np.int64) for s in spans]
        df_words = [None if w is None else np.bincount(w.astype(np.int64)) if len(w) else np.zeros(0, dtype=np.int64) for w in default_words]
        out = {"dp_lengths": dp_len, "default_lengths": df_len, "improved": dp_len < df_len, "dp_word_counts": dp_words,
               "default_word_counts": df_words}
        if pack_length is not None:
            from dptok.packing import plan_lengths
            with torch.cuda.device(dev):
                for key, lens in (("dp_rows", dp_len), ("default_rows", df_len)):
                    out[key] = plan_lengths(torch.from_numpy(np.minimum(lens, int(pack_length))).to(dev), int(pack_length))["n_rows"]
        if words:
            found = device_words(texts)
            out["improved_word_ids"] = [None if f is None else f[0] for f in found]
            out["improved_tokens"] = [None if f is None else [[dp_pieces[i] for i in w] for w in f[1]] for f in found]
            out["worse_tokens"] = [None if f is None else [[default_pieces[i] for i in w] for w in f[2]] for f in found]
        return out

    try:
        bpe = Bpe(*make_table(), device=_device())
        if host_encode("") != list(empty_ids):
            raise ValueError("tokenizer.encode('') is %r, the rule gives %r" % (host_encode(""), list(empty_ids)))
        for probe, got in zip(probes, batch_default(probes)):
            if got != host_encode(probe):
                raise ValueError("the device rule gives %r for the probe %r, the tokenizer %r" % (got, probe, host_encode(probe)))
    except (ValueError, KeyError, DptError) as e:
        stats.default_off = "batch_default is off: %s" % e
        return
    dp_tokenize.batch_default, dp_tokenize.batch_compare = batch_default, batch_compare


def _presplit_words(presplit, texts, bit: int = 0xFF) -> List[Optional[List[str]]]:
    """The device rule's words per text (None where it refuses the text), read back from ``presplit``; ``bit``:
    the bits of the cut mask that open a word (ATOMS masks: 1)."""
    text2, offs2, cut, refused = presplit(list(texts))
    t2, c2, o2 = text2.cpu().numpy().tobytes(), cut.cpu().numpy(), offs2.cpu().numpy().tolist()
    no = set(refused.tolist())
    out: List[Optional[List[str]]] = []
    for s in range(len(o2) - 1):
        if s in no:
            out.append(None)
            continue
        starts = (np.flatnonzero(c2[o2[s]:o2[s + 1]] & bit) + o2[s]).tolist() + [o2[s + 1]]
        out.append([t2[a:b].decode("utf-8", "replace") for a, b in zip(starts, starts[1:])])
    return out


def dp_tokenize_llama(llama_tokenizer, pretokenize_option="llama", device_pretokenize=False):
    t2i: Dict[str, int] = dict(llama_tokenizer.get_vocab())
    vocab_bidict = _InverseDict(t2i)
    engine = Encoder(Vocab(t2i, _device()))
    manual_mapping = _InverseDict({"<0x0A>": "\n"})
    if manual_mapping.inverse != {"\n": "<0x0A>"}:  # the raw kernel hard-codes this mapping
        raise AssertionError("unexpected manual mapping")

    if pretokenize_option == "raw":
        def encode_many(texts: Sequence[str]) -> List[List[int]]:
            return _raise_and_collect(texts, engine.encode_strs(list(texts)))

        def spans_many(texts: Sequence[str]) -> List[TokenSpans]:
            texts = list(texts)
            return _batch_spans(engine, texts, *pack_strings(texts), "raw")

        def pack_batch(texts):
            return (*pack_strings(texts), "raw", None, None, None)
    elif pretokenize_option == "llama":
        pretokenize = pretokenize_with_llama(llama_tokenizer, vocab_bidict)
        pieces = PieceTable(t2i)
        encode_ids = batch_encoder(llama_tokenizer)
        host = shared_pool(llama_tokenizer, pieces, encode_ids)   # worker processes for large batches (one per tokenizer)

        def encode_many(texts: Sequence[str]) -> List[List[int]]:
            # SentencePiece runs on the host (third-party); the pieces -> words merge is array
            # gathers over the whole batch (PieceTable), and the DP of every word of every text is
            # ONE pre-split launch
            texts = list(texts)
            if pieces.ok and not pieces.empty_piece:
                res = engine.encode_packed_presplit(*host.pack(texts))
            else:
                res = engine.encode_presplit([pretokenize(t) for t in texts])
            return _raise_and_collect(texts, res)

        def spans_many(texts: Sequence[str]) -> List[TokenSpans]:
            # the same two packings as encode_many; ``text`` is the pieces' concatenation
            texts = list(texts)
            if pieces.ok and not pieces.empty_piece:
                text, offs, cut, cnt = host.pack(texts)
                return _batch_spans(engine, texts, text, offs, "presplit", cut, none=(cnt == 0).tolist())
            text, offs, cut, n_words, cut_at = pack_presplit_words([pretokenize(t) for t in texts])
            # (as Encoder.encode_presplit: a string is cut at its first empty word -> IndexError)
            return _batch_spans(engine, texts, text, offs, "presplit", cut,
                                outcome=lambda st: presplit_outcome(st, n_words, cut_at))

        def pack_batch(texts):
            # the same two packings again
            if pieces.ok and not pieces.empty_piece:
                text, offs, cut, cnt = host.pack(texts)
                return text, offs, "presplit", cut, cnt == 0, None
            text, offs, cut, n_words, cut_at = pack_presplit_words([pretokenize(t) for t in texts])
            return text, offs, "presplit", cut, None, lambda st: presplit_outcome(st, n_words, cut_at)

        pretok_stats = None
        if device_pretokenize:
            # the words come from the device rule wherever it certifies the text; everything downstream is the same
            if not (pieces.ok and not pieces.empty_piece):
                raise DptError("device_pretokenize needs a vocabulary with dense ids and no empty piece")
            encode_many, spans_many, pack_batch, pretok_stats = _device_pretokenizer(llama_tokenizer, t2i, engine, host, pretokenize)
    else:
        def encode_many(texts):
            raise NameError("name 'pretokenize_func' is not defined")
        spans_many = pack_batch = encode_many

    if pretokenize_option == "raw":
        def dp_tokenize(input_str) -> List[int]:
            ids, st = engine.encode_one(input_str)   # (the per-string call: one zero-copy launch)
            raise_for_status(st, input_str)
            return ids
    else:
        def dp_tokenize(input_str) -> List[int]:
            return encode_many([input_str])[0]

    def decode_dp_tokenization(encoding: List[int]):
        # reference tokenizer_utils.py:82-84: drop the 4-character "<s> " prefix
        return llama_tokenizer.decode(encoding)[4:]

    # SentencePiece's own decode for a batch in one launch: BOS decodes to nothing, the dummy-prefix space
    # is dropped.  The round trip compares with the ORIGINAL text in both modes.
    decode_batch, batch_roundtrip = _decode_surface(
        lambda: Detok(t2i, "sp", [b for b in [_bos_id(llama_tokenizer)] if b is not None], _device()), True, encode_many)
    pair = _finish_adapter(dp_tokenize, decode_dp_tokenization, engine, encode_many, spans_many,
                           _model_inputs_surface(engine, llama_tokenizer, pack_batch), decode_batch, batch_roundtrip,
                           "SentencePiece's", **({"host_pool": host} if pretokenize_option == "llama" else {}),
                           **({"pretok_stats": pretok_stats} if pretokenize_option == "llama" and device_pretokenize else {}))
    if pretokenize_option == "llama" and device_pretokenize:
        # the tokenizer's own ids on the device as well: dp_tokenize.batch_default / batch_compare
        from dptok.pretok_probes import PROBES
        bos = _bos_id(llama_tokenizer)
        _default_surface(dp_tokenize, llama_tokenizer, pretok_stats.split_atoms, lambda: _llama_pairs(llama_tokenizer, t2i),
                         engine.vocab, PROBES, [] if bos is None else [bos], lambda t: False, pretok_stats,
                         pretok_stats.dp_form, vocab_bidict.inverse, vocab_bidict.inverse)
    return pair


def _llama_pairs(tokenizer, t2i):
    """The pair table of a Llama-style tokenizer object by the route it offers: the ``merges`` of its
    ``backend_tokenizer``, else the scores of its SentencePiece processor (``sp_model``; ``sp`` on a bare wrapper)."""
    from dptok.bpe import pairs_from_scores, pairs_from_tokenizer_json
    backend = getattr(tokenizer, "backend_tokenizer", None)
    if backend is not None:
        return pairs_from_tokenizer_json(backend.to_str())
    sp = getattr(tokenizer, "sp_model", None) or getattr(tokenizer, "sp", None)
    if sp is None or not hasattr(sp, "get_score"):
        raise ValueError("the tokenizer object offers neither backend_tokenizer merges nor sp_model scores")
    n = sp.get_piece_size()
    exclude = [i for i in range(n) if sp.is_control(i) or sp.is_unknown(i) or sp.is_unused(i) or sp.is_byte(i)]
    pieces = {sp.id_to_piece(i): i for i in range(n)}
    if any(t2i.get(p) != i for p, i in pieces.items()):
        raise ValueError("the SentencePiece model's ids are not get_vocab()'s")
    return pairs_from_scores(pieces, {p: sp.get_score(i) for p, i in pieces.items()}, exclude)


BLOOM_TOKENIZER_JSON = ("{}/models--bigscience--bloom-3b/snapshots/"
                        "52bc5b43010b4844513826b8be3f78c7344c37d7/tokenizer.json")


BLOOM_SPLIT_PATTERN = " ?[^(\\s|[.,!?…。，、।۔،])]+"


def _device_bytelevel(tokenizer, vocab_to_index, engine, host_pack, pretokenize):
    """The BLOOM adapter with its pre-tokenization on the device (dptok/bytelevel.py; the rule: include/dpt.h
    dpt_bytelevel_create) -> (encode_many, spans_many, pack_batch, stats).  The rule is exact for one pre-tokenizer and
    one alphabet, so construction checks both: the tokenizer's pre-tokenizer must be Sequence[Split(Regex(
    BLOOM_SPLIT_PATTERN), isolated), ByteLevel(add_prefix_space=False, use_regex=False)], every character of the
    byte alphabet must be a vocabulary entry that ``convert_ids_to_tokens`` gives back unchanged, and the probe list
    must come out of the device rule as out of ``pre_tokenize_str``.  DptError names the first difference."""
    import json
    from dptok.bytelevel import BLOOM_SEPARATORS, ByteLevelSplit, bytes_to_unicode
    from dptok.bytelevel_probes import PROBES

    try:
        pre = json.loads(tokenizer._tokenizer.to_str()).get("pre_tokenizer")
    except Exception as e:   # noqa: BLE001
        raise DptError("device_pretokenize: the tokenizer's pre-tokenizer cannot be read (%s)" % e)
    steps = pre.get("pretokenizers") if isinstance(pre, dict) and pre.get("type") == "Sequence" else None
    if not (isinstance(steps, list) and len(steps) == 2 and all(isinstance(x, dict) for x in steps)):
        raise DptError("device_pretokenize: the pre-tokenizer is not Sequence[Split, ByteLevel]: %r" % (pre,))
    split, level = steps
    for what, got, want in (("first step", split.get("type"), "Split"), ("Split pattern", split.get("pattern"), {"Regex": BLOOM_SPLIT_PATTERN}),
                            ("Split behavior", split.get("behavior"), "Isolated"), ("Split invert", bool(split.get("invert")), False),
                            ("second step", level.get("type"), "ByteLevel"),
                            ("ByteLevel add_prefix_space", bool(level.get("add_prefix_space")), False),
                            ("ByteLevel use_regex", bool(level.get("use_regex")), False)):
        if got != want:
            raise DptError("device_pretokenize: the pre-tokenizer's %s is %r, the device rule needs %r" % (what, got, want))
    alphabet = bytes_to_unicode()
    for b in range(256):
        if alphabet[b] not in vocab_to_index:
            raise DptError("device_pretokenize: the byte alphabet's %r (byte 0x%02X) is not in the vocabulary" % (alphabet[b], b))
    back = tokenizer.convert_ids_to_tokens([vocab_to_index[alphabet[b]] for b in range(256)])
    for b in range(256):
        if back[b] != alphabet[b]:
            raise DptError("device_pretokenize: convert_ids_to_tokens gives %r for the byte alphabet's %r (byte 0x%02X)"
                           % (back[b], alphabet[b], b))
    splitter = ByteLevelSplit(BLOOM_SEPARATORS, _device())
    presplit, *paths, stats = _device_split_paths(splitter.split, "atoms", engine, host_pack)
    stats.split_atoms = splitter.split   # (_default_surface)
    stats.dp_form = (splitter.split, "atoms")
    _probe_check(presplit, stats, PROBES, pretokenize, 1, False, "pre-tokenizer is not the one the rule holds for")
    return (*paths, stats)


def dp_tokenize_bloom(bloom_tokenizer, HF_CACHE_DIR, device_pretokenize=False):
    """BLOOM byte-level adapter (reference tokenizer_utils.py:98-181).

    * the vocabulary is ``tokenizer.json``'s ``model.vocab`` with ids = its **enumeration
      order** (reference :104-108, ``{token: index for index, token in enumerate(vocab)}``);
    * words come from the tokenizer's own pre-tokenizer (``pre_tokenize_str``, :160-162);
    * a word's atoms are ``convert_ids_to_tokens([vocab_to_index[c] for c in word])`` (:155-157;
      a character outside the vocabulary raises KeyError there, as in the reference);
    * the DP + longest-token selection + ids run on the GPU in atoms mode (one launch per
      call; ``dp_tokenize.batch`` for many strings), ids = enumeration-order indices (:174-177).
    The reference's ``merges`` -> ``token_to_source_merge`` map (:113-116) feeds only the unused
    ``unwind_to_base_tokenization``; merges are parsed here in either tokenizer.json form
    ("a b" strings or [a, b] pairs) and otherwise unused.

    ``device_pretokenize=True``: the words and atoms are made on the GPU as well (dptok/bytelevel.py; the rule:
    include/dpt.h dpt_bytelevel_create) -- text up, two kernels, the atoms-mode encode, ids back; the tokenizer object
    is asked only at construction (``_device_bytelevel``: DptError unless its pre-tokenizer and alphabet are the ones
    the rule is exact for) and for text that is not well-formed UTF-8, which goes through the host path as one
    sub-batch.  Same ids and exceptions; ``dp_tokenize.pretok_stats`` reads as (made on the device, sent to the host)
    of the last call.  The default leaves the host path untouched.
    """
    import json

    with open(BLOOM_TOKENIZER_JSON.format(HF_CACHE_DIR), "r") as f:
        tokenizer_json = json.load(f)
    merges = tokenizer_json["model"]["merges"]
    vocab_to_index = _InverseDict({token: index for index, token in enumerate(tokenizer_json["model"]["vocab"])})
    token_to_source_merge = {}
    for merge in merges:
        a, b = merge.split() if isinstance(merge, str) else merge
        token_to_source_merge[a + b] = (a, b)
    engine = Encoder(Vocab(dict(vocab_to_index), _device()))

    def pretokenize(input_str):
        pretokenized = bloom_tokenizer._tokenizer.pre_tokenizer.pre_tokenize_str(input_str)
        return [block[0] for block in pretokenized]

    def atoms_of(word):
        token_inds = [vocab_to_index[c] for c in word]   # KeyError for characters outside the vocab
        return bloom_tokenizer.convert_ids_to_tokens(token_inds)

    def encode_many(texts: Sequence[str]) -> List[List[int]]:
        batch = [[atoms_of(w) for w in pretokenize(t)] for t in texts]
        return _raise_and_collect(texts, engine.encode_word_atoms(batch))

    def spans_many(texts: Sequence[str]) -> List[TokenSpans]:
        # ``text`` is the atoms' concatenation (the byte-level alphabet's characters, one per input byte)
        texts = list(texts)
        batch = [[atoms_of(w) for w in pretokenize(t)] for t in texts]
        text, offs, cut = pack_word_atoms(batch)
        return _batch_spans(engine, texts, text, offs, "atoms", cut, none=[not words for words in batch])

    def pack_batch(texts):
        batch = [[atoms_of(w) for w in pretokenize(t)] for t in texts]
        text, offs, cut = pack_word_atoms(batch)
        return text, offs, "atoms", cut, [not words for words in batch], None

    pretok_stats = None
    if device_pretokenize:
        def host_pack(texts):
            batch = [[atoms_of(w) for w in pretokenize(t)] for t in texts]
            return (*pack_word_atoms(batch), np.fromiter((len(words) for words in batch), dtype=np.int64, count=len(batch)))

        encode_many, spans_many, pack_batch, pretok_stats = _device_bytelevel(bloom_tokenizer, vocab_to_index, engine, host_pack,
                                                                             pretokenize)

    def dp_tokenize(input_str) -> List[int]:
        return encode_many([input_str])[0]

    def decode_dp_tokenization(encoding: List[int]):
        return bloom_tokenizer.decode(encoding)   # reference :179-181

    # ByteLevel's own decode (the alphabet back to bytes, nothing stripped); the round trip compares with
    # the UTF-8 of the input
    decode_batch, batch_roundtrip = _decode_surface(lambda: Detok(dict(vocab_to_index), "bytelevel", (), _device()), False,
                                                    encode_many)
    pair = _finish_adapter(dp_tokenize, decode_dp_tokenization, engine, encode_many, spans_many,
                           _model_inputs_surface(engine, bloom_tokenizer, pack_batch), decode_batch, batch_roundtrip,
                           "ByteLevel's", vocab_to_index=vocab_to_index,
                           **({"pretok_stats": pretok_stats} if device_pretokenize else {}))
    if device_pretokenize:
        # the tokenizer's own ids on the device as well: dp_tokenize.batch_default / batch_compare.  ``encode`` matches
        # the added-token literals before the model does and pre_tokenize_str does not: such a text goes to the host
        from dptok.bpe import pairs_from_merges
        from dptok.bytelevel_probes import PROBES
        model = tokenizer_json["model"]
        real = model["vocab"]
        literals = [t for t in dict.fromkeys(list(getattr(bloom_tokenizer, "all_special_tokens", None) or [])
                                             + list(bloom_tokenizer.get_added_vocab())) if t]

        def make_table():
            if json.loads(bloom_tokenizer._tokenizer.to_str()).get("normalizer") is not None:
                raise ValueError("the tokenizer has a normalizer")
            return pairs_from_merges(real, merges, model)

        same_ids = all(real[t] == i for i, t in enumerate(real))
        _default_surface(dp_tokenize, bloom_tokenizer, pretok_stats.split_atoms, make_table,
                         engine.vocab if same_ids else Vocab(dict(real), _device()), PROBES, [],
                         lambda t: any(x in t for x in literals), pretok_stats, pretok_stats.dp_form, vocab_to_index.inverse,
                         vocab_to_index.inverse if same_ids else {i: t for t, i in real.items()})
    return pair
