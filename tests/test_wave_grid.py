"""The grid of the one-wave-per-string kernels (csrc/dpt_internal.h wave_per_string_blocks, through
include/dpt.h dpt_debug_wave_grid) and its test-only cap DPT_WAVE_GRID_BLOCKS: no GPU needed.  The GPU tests of
tests/test_gpu_wave_stride.py ask the same call for the grid their launches get."""
import pytest

KNOB = "DPT_WAVE_GRID_BLOCKS"
SIZES = [1, 4, 5, 4 << 20, (4 << 20) + 1, (1 << 31) - 1]


def _default(n, waves=4):
    return min(-(-n // waves), 1 << 20)


@pytest.mark.parametrize("n", SIZES)
def test_default_grid(n, monkeypatch):
    from dptok import _lib
    monkeypatch.delenv(KNOB, raising=False)
    assert _lib.wave_grid(n, 4) == _default(n)


@pytest.mark.parametrize("cap", [1, 3, 2000000])
@pytest.mark.parametrize("n", SIZES)
def test_capped_grid(n, cap, monkeypatch):
    from dptok import _lib
    monkeypatch.setenv(KNOB, str(cap))
    assert _lib.wave_grid(n, 4) == min(_default(n), cap)


@pytest.mark.parametrize("value", ["", "0", "-2", "abc"])
@pytest.mark.parametrize("n", SIZES)
def test_values_that_are_no_cap(n, value, monkeypatch):
    from dptok import _lib
    monkeypatch.setenv(KNOB, value)
    assert _lib.wave_grid(n, 4) == _default(n)


def test_read_on_every_call_and_other_block_sizes(monkeypatch):
    from dptok import DptError, _lib
    monkeypatch.setenv(KNOB, "3")
    assert _lib.wave_grid(100, 4) == 3
    monkeypatch.setenv(KNOB, "7")
    assert _lib.wave_grid(100, 4) == 7 and _lib.wave_grid(100, 16) == 7 and _lib.wave_grid(100, 32) == 4
    monkeypatch.delenv(KNOB)
    assert _lib.wave_grid(100, 4) == 25 and _lib.wave_grid(0, 4) == 0
    with pytest.raises(DptError):
        _lib.wave_grid(100, 0)
