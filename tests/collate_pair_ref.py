"""The dpt_collate_pair rule (include/dpt.h) as plain Python over lists -- the model the tests compare the kernel
with.  Written from the rule's text, not from the kernel."""
from collate_ref import wrap

BOS, EOS, PAD_LEFT, TRUNC_LEFT, I64, SEP, MASK_A, TRIM_A_FIRST = 1, 2, 4, 8, 16, 32, 64, 128


def n_special(flags):
    return bool(flags & BOS) + bool(flags & SEP) + bool(flags & EOS)


def kept(nA, nB, max_a, max_b, room, a_first=False):
    """-> (kA, kB): the tokens each side keeps, by the header's caps / over / dA / dB arithmetic."""
    cA = min(nA, max_a) if max_a else nA
    cB = min(nB, max_b) if max_b else nB
    over = max(0, cA + cB - room)
    if a_first:
        dA = min(over, cA)
        dB = over - dA
    else:
        dB = min(over, cB)
        dA = over - dB
    return cA - dA, cB - dB


def _side_tokens(side, s):
    """(the flat ids, the index of string s's first token, its token count) of side = (ids, off, counts, status)"""
    ids, off, counts = side[0], side[1], side[2]
    n = off[s + 1] - off[s] if counts is None else counts[s]
    return ids, off[s] - off[0], n


def collate_pair_ref(a, b, *, row_len, pad_id=0, bos_id=0, sep_id=0, eos_id=0, ignore_id=-100, max_a=0, max_b=0, flags=0):
    """-> (input_ids, attention_mask, labels, token_type_ids, lengths, b_start): four lists of n_str rows of
    ``row_len`` ints and two lists of n_str ints.  ``a`` / ``b``: (ids, off, counts, status) as lists, each as
    collate_ref takes them (``counts`` None: n = off[s+1] - off[s]; ``status`` None: all 0)."""
    L = row_len
    n_str = len(a[1]) - 1
    assert len(b[1]) - 1 == n_str
    nsp = n_special(flags)
    if L == 0 or L < nsp:
        raise ValueError("row_len")
    room = L - nsp
    pad, ign = wrap(pad_id), wrap(ignore_id)
    rows, masks, labs, types, lengths, b_start = [], [], [], [], [], []
    for s in range(n_str):
        if (a[3] is not None and a[3][s] != 0) or (b[3] is not None and b[3][s] != 0):
            rows.append([pad] * L)
            masks.append([0] * L)
            labs.append([ign] * L)
            types.append([0] * L)
            lengths.append(0)
            b_start.append(0)
            continue
        idsA, firstA, nA = _side_tokens(a, s)
        idsB, firstB, nB = _side_tokens(b, s)
        kA, kB = kept(nA, nB, max_a, max_b, room, bool(flags & TRIM_A_FIRST))
        skipA = nA - kA if flags & TRUNC_LEFT else 0
        skipB = nB - kB if flags & TRUNC_LEFT else 0
        head = ([wrap(bos_id)] if flags & BOS else []) + [wrap(idsA[firstA + skipA + k]) for k in range(kA)] \
            + ([wrap(sep_id)] if flags & SEP else [])
        tail = [wrap(idsB[firstB + skipB + k]) for k in range(kB)] + ([wrap(eos_id)] if flags & EOS else [])
        seq = head + tail
        ln = len(seq)
        assert ln == kA + kB + nsp <= L
        lab = ([ign] * len(head) if flags & MASK_A else head) + tail
        typ = [0] * len(head) + [1] * len(tail)
        fill = L - ln
        if flags & PAD_LEFT:
            rows.append([pad] * fill + seq)
            masks.append([0] * fill + [1] * ln)
            labs.append([ign] * fill + lab)
            types.append([0] * fill + typ)
            b_start.append(fill + len(head))
        else:
            rows.append(seq + [pad] * fill)
            masks.append([1] * ln + [0] * fill)
            labs.append(lab + [ign] * fill)
            types.append(typ + [0] * fill)
            b_start.append(len(head))
        lengths.append(ln)
    return rows, masks, labs, types, lengths, b_start
