"""What the GPU tests of the two device splitters share (test_gpu_pretok.py, test_gpu_bytelevel.py): the guarded
sizes + write run of an object with ``sizes_device`` / ``write_device``, and its comparison, byte for byte, with a
plain-Python reference."""
import numpy as np

G = 67   # canary bytes on each side of an output (odd: the outputs start at odd addresses)


def _run(split, strings, pad=3, off0=1_000_003, out0=77):
    """sizes + write over ``strings`` -> (pre_status, out_len, text2 bytes, cut bytes).  The text sits at an odd
    address between continuation bytes (a load beyond a string's end would complete a truncated character),
    str_off and out_off start at off0 / out0, and every output lies between canaries that must survive."""
    return run_packed(split, b"".join(strings), np.array([len(s) for s in strings], dtype=np.int64), pad, off0, out0)


def run_packed(split, raw, lens, pad=3, off0=1_000_003, out0=77):
    """``_run`` over the strings of ``lens`` bytes each that ``raw`` holds back to back (batches too large for a
    list of strings)."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(lens)
    blob = np.frombuffer(b"\xbf" * pad + raw + b"\x80" * 8, dtype=np.uint8).copy()
    offs = np.full(n + 1, off0, dtype=np.int64)
    offs[1:] += np.cumsum(lens, dtype=np.int64)
    assert int(offs[-1]) - off0 == len(raw)
    d_blob, d_offs = torch.from_numpy(blob).to(dev), torch.from_numpy(offs).to(dev)

    def guarded(nbytes):
        return torch.full((G + nbytes + G,), 0xAA, dtype=torch.uint8, device=dev)

    def inner(buf, nbytes):
        got = buf.cpu().numpy()
        assert (got[:G] == 0xAA).all() and (got[G + nbytes:] == 0xAA).all(), "a store outside the output"
        return got[G:G + nbytes]

    b_len, b_st = guarded(8 * n + 5)[5:], guarded(4 * n + 1)[1:]      # (8- and 4-byte aligned behind the canary)
    assert (b_len.data_ptr() + G) % 8 == 0 and (b_st.data_ptr() + G) % 4 == 0
    split.sizes_device(d_blob.data_ptr() + pad, d_offs.data_ptr(), n, b_len.data_ptr() + G, b_st.data_ptr() + G)
    torch.cuda.synchronize()
    out_len = inner(b_len, 8 * n).copy().view(np.uint64)
    pre = inner(b_st, 4 * n).copy().view(np.int32)
    out_off = np.full(n + 1, out0, dtype=np.int64)
    out_off[1:] += np.cumsum(out_len.astype(np.int64))
    total = int(out_off[-1]) - out0
    d_out_off = torch.from_numpy(out_off).to(dev)
    b_text, b_cut = guarded(total), guarded(total)
    assert (b_text.data_ptr() + G) % 2 == 1
    split.write_device(d_blob.data_ptr() + pad, d_offs.data_ptr(), n, b_st.data_ptr() + G, b_text.data_ptr() + G,
                       d_out_off.data_ptr(), b_cut.data_ptr() + G)
    torch.cuda.synchronize()
    inner(b_len, 8 * n), inner(b_st, 4 * n)
    return pre, out_len, inner(b_text, total).tobytes(), inner(b_cut, total).tobytes()


def check(split, ref, strings, **kw):
    """``_run(split, strings, **kw)`` is ``ref(strings)`` -- (pre_status, out_len, text2, cut) -- or an AssertionError
    that names the first strings that differ; returns the reference's."""
    want = ref(strings)
    got = _run(split, strings, **kw)
    bad = np.flatnonzero(got[0] != want[0])
    assert not len(bad), ("pre_status", [(int(i), strings[i][:80], int(got[0][i]), int(want[0][i])) for i in bad[:5]])
    bad = np.flatnonzero(got[1] != want[1])
    assert not len(bad), ("out_len", [(int(i), strings[i][:80], int(got[1][i]), int(want[1][i])) for i in bad[:5]])
    for what, g, w in (("text", got[2], want[2]), ("cut", got[3], want[3])):
        if g != w:
            k = next(i for i in range(len(w)) if g[i] != w[i])
            s = int(np.searchsorted(np.cumsum(want[1].astype(np.int64)), k, side="right"))
            raise AssertionError((what, "string", s, strings[s][:80], "byte", k, g[max(k - 8, 0):k + 8], w[max(k - 8, 0):k + 8]))
    return want
