"""The dpt_collate rule (include/dpt.h) as plain Python over lists -- the model the tests compare the kernel
with.  Written from the rule's text, not from the kernel."""
BOS, EOS, PAD_LEFT, TRUNC_LEFT, I64 = 1, 2, 4, 8, 16


def wrap(v):
    """``v`` as the int32 the engine holds: what an int32 element stores and an int64 element sign-extends."""
    v = int(v) & 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def collate_ref(ids, off, counts=None, status=None, *, row_len, pad_id=0, bos_id=0, eos_id=0, ignore_id=-100, flags=0):
    """-> (input_ids, attention_mask, labels, lengths): three lists of n_str rows of ``row_len`` ints and one
    list of n_str ints.  ``ids`` is the flat id list that ``off[0]`` corresponds to (token k of string s is
    ids[off[s] - off[0] + k]); ``counts`` None: n = off[s+1] - off[s], else counts[s]; ``status`` None: all 0."""
    L = row_len
    n_str = len(off) - 1
    n_special = (1 if flags & BOS else 0) + (1 if flags & EOS else 0)
    if L == 0 or L < n_special:
        raise ValueError("row_len")
    pad, ign = wrap(pad_id), wrap(ignore_id)
    rows, masks, labs, lengths = [], [], [], []
    for s in range(n_str):
        if status is not None and status[s] != 0:
            rows.append([pad] * L)
            masks.append([0] * L)
            labs.append([ign] * L)
            lengths.append(0)
            continue
        n = off[s + 1] - off[s] if counts is None else counts[s]
        first = off[s] - off[0]
        keep = min(n, L - n_special)
        skip = n - keep if flags & TRUNC_LEFT else 0
        seq = []
        if flags & BOS:
            seq.append(wrap(bos_id))
        for k in range(keep):
            seq.append(wrap(ids[first + skip + k]))
        if flags & EOS:
            seq.append(wrap(eos_id))
        ln = len(seq)
        fill = L - ln
        if flags & PAD_LEFT:
            rows.append([pad] * fill + seq)
            masks.append([0] * fill + [1] * ln)
            labs.append([ign] * fill + seq)
        else:
            rows.append(seq + [pad] * fill)
            masks.append([1] * ln + [0] * fill)
            labs.append(seq + [ign] * fill)
        lengths.append(ln)
    return rows, masks, labs, lengths
