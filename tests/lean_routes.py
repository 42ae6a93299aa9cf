"""TEST INFRASTRUCTURE: one raw call on a first-pass route chosen by the test ("the lean pass and the
hint").  A plain raw call of a 16-lane vocabulary runs the lean kernel plus the list-fed general kernel, or the general
RAW kernel alone, depending on the context's hint word -- so on the calls the context has seen.  Here a *fresh*
``Encoder`` is the reset:

* the lean route: a fresh context, its words (0, 0, 0, 0) before the call; after it no probe and no skipped call, i.e.
  the lean pair was launched;
* the general route: a second fresh context with ``debug_no_lean(True)``.

Both go through the same entry -- device CSR (``encode_device``), device padded (``encode_device_padded``) or host
(``encode_csr``) -- and must agree with each other and with the C oracle, exactly.  ``device_call`` / ``both_routes``
are the one-context helpers tests/test_gpu_lean_pass.py has always used (the route there is the context's history)."""
import numpy as np

import lean_ref

N_BINS = 64
ENTRIES = ("device", "padded", "host")


def device_call(enc, text, offs):
    """dpt_encode with a DPT_HIST_OVERWRITE histogram -> (ids, id_off, status, capped, hist)"""
    import torch
    n = len(offs) - 1
    cap = max(len(text), 1)
    dt = torch.from_numpy(np.array(text) if len(text) else np.zeros(1, np.uint8)).cuda()
    do = torch.from_numpy(offs.astype(np.uint64).view(np.int64)).cuda()
    ids = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
    id_off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    capped = torch.empty(n, dtype=torch.int32, device="cuda")
    hist = torch.full((N_BINS + 8,), -3, dtype=torch.int64, device="cuda")
    enc.set_histogram(hist.data_ptr(), N_BINS, overwrite=True)
    enc.encode_device(dt.data_ptr(), len(text), do.data_ptr(), n, ids.data_ptr(), cap, id_off.data_ptr(), st.data_ptr(),
                      capped_ptr=capped.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    off_h = id_off.cpu().numpy().view(np.uint64)
    return ids[: int(off_h[-1])].cpu().numpy(), off_h, st.cpu().numpy(), capped.cpu().numpy(), hist.cpu().numpy()


def padded_call(enc, text, offs):
    """dpt_encode_padded -> (the ids of every string, read at its byte offset and joined in order, id_off built from
    the counts, status, capped): the CSR view of what the call left at the byte offsets"""
    import torch
    n = len(offs) - 1
    cap = max(len(text), 1)
    dt = torch.from_numpy(np.array(text) if len(text) else np.zeros(1, np.uint8)).cuda()
    do = torch.from_numpy(offs.astype(np.uint64).view(np.int64)).cuda()
    ids = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), 7, dtype=torch.int64, device="cuda")
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    capped = torch.empty(n, dtype=torch.int32, device="cuda")
    enc.encode_device_padded(dt.data_ptr(), len(text), do.data_ptr(), n, ids.data_ptr(), cap, cnt.data_ptr(), st.data_ptr(),
                             capped_ptr=capped.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cnt_h = cnt.cpu().numpy().astype(np.int64)
    ids_h = ids.cpu().numpy()
    o = offs.astype(np.int64) - int(offs[0])
    assert np.all(cnt_h >= 0) and np.all(cnt_h <= np.diff(o)), "a count outside its string's bytes"
    id_off = np.zeros(n + 1, dtype=np.uint64)
    id_off[1:] = np.cumsum(cnt_h)
    # element k of string s: ids[o[s] + k]
    src = np.repeat(o[:-1] - id_off[:-1].astype(np.int64), cnt_h) + np.arange(int(id_off[-1]), dtype=np.int64)
    return ids_h[src], id_off, st.cpu().numpy(), capped.cpu().numpy()


def host_call(enc, text, offs):
    """dpt_encode_host -> (ids, id_off, status, capped)"""
    return enc.encode_csr(np.ascontiguousarray(text), offs)


CALLS = {"device": device_call, "padded": padded_call, "host": host_call}


def both_routes(enc, orc, text, offs):
    """lean on, lean off (the launch knob), both against the oracle; returns the oracle's (ids, off, status, capped)"""
    lean = device_call(enc, text, offs)
    enc.debug_no_lean(True)
    try:
        plain = device_call(enc, text, offs)
    finally:
        enc.debug_no_lean(False)
    ref = orc.encode_csr(text, offs)
    _compare(lean, plain, ref)
    return ref


def _compare(lean, plain, ref):
    for k, (x, y) in enumerate(zip(lean, plain)):
        assert np.array_equal(x, y), ("lean route differs from the general kernel alone", k)
    for k in range(4):   # ids, offsets, status, capped
        assert np.array_equal(lean[k], ref[k]), (k, np.nonzero(np.asarray(lean[k][:len(ref[k])]) != ref[k][:len(lean[k])])[0][:10])
    counts = np.diff(ref[1].astype(np.int64))
    if len(lean) > 4:   # the device CSR entry's histogram
        assert lean[4][N_BINS] == counts.sum() and lean[4][N_BINS + 1] == len(counts)
    # the ids tile [0, n_tok): every string once
    assert int(ref[1][-1]) == len(lean[0]) and np.all(np.diff(lean[1].astype(np.int64)) >= 0)


def lean_call(vocab, entry, text, offs):
    """The call on the lean route: a fresh context, asserted untouched before and to have launched the lean pair after.
    -> (the entry's outputs, debug_lean_words())"""
    from dptok import Encoder
    enc = Encoder(vocab)
    assert enc.debug_lean_words() == (0, 0, 0, 0)
    got = CALLS[entry](enc, text, offs)
    words = enc.debug_lean_words()
    assert words[2] == 0 and words[3] == 0, ("the lean pair was not launched", words)
    return got, words


def general_call(vocab, entry, text, offs):
    """The call on the general RAW kernel alone: a second fresh context with the lean launch switched off."""
    from dptok import Encoder
    enc = Encoder(vocab)
    enc.debug_no_lean(True)
    got = CALLS[entry](enc, text, offs)
    assert enc.debug_lean_words() == (0, 0, 0, 0), "a lean kernel ran on the general route"
    return got


def pinned_routes(vocab, orc, text, offs, entry="device", want=None, exact=False):
    """Both routes through ``entry`` on contexts of their own: identical outputs, equal to the oracle's.

    ``want``: how many strings the model (lean_ref.predicted_deferred) says the lean kernel defers; None: the count is
    not checked.  The lean waves stop claiming once the hint is off, so: hint still on after the call -> exactly
    ``want`` deferred; hint off -> at least one and at most ``want``.  ``exact``: the call was built to hold at most
    five such strings -- no wave can reach the six deferrals of its own that turn the hint off -- so the hint must
    still be on and the count exact.
    -> (the oracle's (ids, off, status, capped), the lean route's words)"""
    lean, words = lean_call(vocab, entry, text, offs)
    plain = general_call(vocab, entry, text, offs)
    ref = orc.encode_csr(text, offs)
    _compare(lean, plain, ref)
    off, n_def = words[0], words[1]
    if exact:
        assert want is not None and want <= 5
        assert off == 0 and n_def == want, (words, want)
    elif want is not None:
        if off == 0:
            assert n_def == want, (words, want)
        else:
            assert 0 < n_def <= want, (words, want)
    return ref, words


def model_sets(t2i):
    """(no_token_bytes, first_no_token_bytes) of a vocabulary"""
    return lean_ref.no_token_bytes(t2i), lean_ref.first_no_token_bytes(t2i)


def want_deferred(t2i, text, offs):
    """the model's count of deferred strings for a packed corpus"""
    nt, fnt = model_sets(t2i)
    return len(lean_ref.predicted_deferred(lean_ref.split_blob(text, offs), nt, fnt))
