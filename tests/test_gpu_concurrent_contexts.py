"""Several contexts on several streams sharing one dpt_vocab (include/dpt.h: "a dpt_vocab is immutable
after creation and may be shared by threads and streams; a dpt_ctx must be used by one stream at a
time"): four workloads issued back to back on four side streams, five rounds, one synchronisation at
the end, every round bit-exact against the C oracle.  bench.py's batches-in-flight loop relies on it."""
import numpy as np
import pytest

import matrix_corpus as mc

pytestmark = pytest.mark.gpu

ROUNDS = 5


def _ragged(n=20000, seed=77):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 65, n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    text = rng.integers(0x20, 0x7F, int(offs[-1])).astype(np.uint8)
    return text, offs, None


@pytest.fixture(scope="module")
def workloads():
    """The four (form, text, offsets, cut mask) inputs: they differ in size, mode and passes."""
    return [("raw",) + _ragged()] + [(f,) + mc.form(f) for f in mc.FORMS]


@pytest.fixture(scope="module")
def oracle_results(workloads):
    from oracle import oracle
    cache = {}

    def get(vocab, k):
        if (vocab, k) not in cache:
            f, text, offs, cut = workloads[k]
            cache[(vocab, k)] = oracle.OracleVocab(mc.vocabularies()[vocab]).encode_csr(
                text, offs, mode=mc.oracle_mode(f), cut_mask=cut)
        return cache[(vocab, k)]
    return get


@pytest.fixture(scope="module")
def device_vocabs():
    from dptok import Vocab
    return {name: Vocab(mc.vocabularies()[name], 0) for name in ("base", "long+40000")}


def _run(vocab_names, vocabs, workloads, oracle_results):
    """Context k (vocabulary vocab_names[k], workload k) on stream k."""
    torch = pytest.importorskip("torch")
    from dptok import Encoder
    encs = [Encoder(vocabs[name]) for name in vocab_names]
    streams = [torch.cuda.Stream() for _ in vocab_names]
    assert len({s.cuda_stream for s in streams} | {0}) == len(streams) + 1
    dev, outs = [], []
    for k, (f, text, offs, cut) in enumerate(workloads):
        n, nb = len(offs) - 1, int(offs[-1])
        dev.append((torch.from_numpy(text).cuda(), torch.from_numpy(offs.view(np.int64)).cuda(),
                    None if cut is None else torch.from_numpy(cut).cuda()))
        outs.append([(torch.full((nb,), -7, dtype=torch.int32, device="cuda"),
                      torch.full((n + 1,), -7, dtype=torch.int64, device="cuda"),
                      torch.full((n,), -7, dtype=torch.int32, device="cuda")) for _ in range(ROUNDS)])
        encs[k].reserve(nb, n)   # no allocation, so no implicit synchronisation, inside the rounds
    torch.cuda.synchronize()
    for r in range(ROUNDS):
        for k, (f, text, offs, cut) in enumerate(workloads):
            dt, do, dc = dev[k]
            ids, io, st = outs[k][r]
            encs[k].encode_device(dt.data_ptr(), int(offs[-1]), do.data_ptr(), len(offs) - 1, ids.data_ptr(), len(ids),
                                  io.data_ptr(), st.data_ptr(), cut_ptr=0 if dc is None else dc.data_ptr(),
                                  stream=streams[k].cuda_stream, mode=f)
    torch.cuda.synchronize()
    for k in range(len(workloads)):
        rids, roff, rst, _ = oracle_results(vocab_names[k], k)
        for r in range(ROUNDS):
            ids, io, st = (t.cpu().numpy() for t in outs[k][r])
            assert np.array_equal(st, rst), (k, r, np.nonzero(st != rst)[0][:10])
            assert np.array_equal(io.view(np.uint64), roff), (k, r)
            assert np.array_equal(ids[: int(roff[-1])], rids), (k, r)


def test_four_contexts_four_streams_one_vocab(device_vocabs, workloads, oracle_results):
    _run(["base"] * 4, device_vocabs, workloads, oracle_results)


def test_two_vocabularies_in_flight(device_vocabs, workloads, oracle_results):
    """A 16-lane (int16 staging) and a 64-lane (int32 staging) vocabulary alive at once: their kernels are in
    flight together, and launch_encode's per-device caches serve both."""
    _run(["base", "long+40000", "long+40000", "base"], device_vocabs, workloads, oracle_results)
