"""The tensor checks of ``model_inputs`` and ``pair_model_inputs`` that run before any device work: host tensors
suffice, the library is never called."""
import pytest


@pytest.mark.parametrize("short", ["counts", "status"])
def test_status_and_counts_need_n_str_entries(short):
    """a ``counts`` or ``status`` tensor one entry short of n_str is an error of both calls, not a read past its end"""
    import torch
    from dptok import collate
    n = 5
    ids = torch.zeros(4 * n, dtype=torch.int32)
    off = torch.arange(0, 4 * (n + 1), 4, dtype=torch.int64)
    status, counts = torch.zeros(n, dtype=torch.int32), torch.full((n,), 3, dtype=torch.int64)
    good = (ids, off, status, counts)
    bad = (ids, off, status[:-1], counts) if short == "status" else (ids, off, status, counts[:-1])
    with pytest.raises(ValueError, match="status / counts need n_str entries"):
        collate.model_inputs(*bad, padding="max_length", max_length=8)
    with pytest.raises(ValueError, match="status / counts need n_str entries"):
        collate.model_inputs(*bad)
    for a, b in ((bad, good), (good, bad)):
        with pytest.raises(ValueError, match="status / counts need n_str entries"):
            collate.pair_model_inputs(a, b, padding="max_length", max_length=8)
