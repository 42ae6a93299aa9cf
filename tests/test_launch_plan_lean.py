"""The lean route in the encode launch plan (plan_encode, through the test-only dpt_debug_launch_plan_lean: 1 when
the lean kernel and the list-fed general kernel run in the first pass's place).  Plain raw calls of 16-lane
vocabularies take it; nothing else does; the rest of the plan (dpt_debug_launch_plan, the entry
tests/test_launch_plan.py uses) is what it is without it.  No GPU."""
import ctypes
import itertools

import pytest

RAW, PRESPLIT, ATOMS = 0, 1, 2
UNCAPPED, LEN_ONLY = 0x10, 0x20
ROWS16, ROWS64 = 1, 2
GENERIC_RAW, NO_SOLO_WAVE, NO_LEAN = 2, 4, 16
N_INTS = 20


@pytest.fixture(scope="module")
def plan():
    from dptok import _lib
    L = _lib.lib()

    def call(variant=ROWS16, mode=RAW, st16=True, edges=False, solo=False, padded=False, n_str=1000, knobs=0):
        """(the plan's twenty ints, lean)"""
        out = (ctypes.c_int * N_INTS)()
        lean = ctypes.c_int(-9)
        assert L.dpt_debug_launch_plan(variant, mode, st16, edges, solo, padded, 0, 0, n_str, 0, 258, knobs, out) == 0
        assert L.dpt_debug_launch_plan_lean(variant, mode, st16, edges, solo, padded, n_str, knobs, ctypes.byref(lean)) == 0
        return list(out), lean.value
    return call


@pytest.mark.parametrize("st16", [True, False])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n_str", [2, 1000, 256 * 2048 + 1])
def test_plain_raw_calls_take_the_lean_route(plan, st16, padded, n_str):
    st16 = st16 and not padded   # (dpt_encode_padded: the ids go to the caller's int32 array whatever the vocabulary)
    got, lean = plan(st16=st16, padded=padded, n_str=n_str)
    sw = 1 if st16 else 2
    # the general kernel is still the plan's first pass (the lean pair stands in its place at launch)
    assert got[0:6] == [16, 0, sw, 1, 0, -1] and lean == 1
    assert got[6] == 0 and got[13] == 0   # no 512-byte pass; the 2048-byte pass reads the first list
    # the knob: the same plan without the lean launch
    off, lean_off = plan(st16=st16, padded=padded, n_str=n_str, knobs=NO_LEAN)
    assert off == got and lean_off == 0


def test_the_other_calls_do_not(plan):
    for kw in (dict(edges=True), dict(mode=RAW | UNCAPPED), dict(mode=RAW | LEN_ONLY), dict(mode=PRESPLIT), dict(mode=ATOMS),
               dict(variant=ROWS64), dict(variant=ROWS64, mode=ATOMS), dict(knobs=GENERIC_RAW), dict(n_str=0),
               dict(solo=True, n_str=1), dict(solo=True, n_str=1, knobs=NO_SOLO_WAVE)):
        assert plan(**kw)[1] == 0, kw
    # (the solo flag means nothing for more than one string)
    assert plan(solo=True, n_str=2)[1] == 1


def test_the_lean_route_keeps_the_plan_of_the_workspace(plan):
    """the deferred strings' list is the third retry list, which no other pass of a raw call reads (big_list stays the
    first), and no 512-byte pass appears: nothing in the plan asks for workspace the call did not have
    (tests/test_gpu_lean_pass.py::test_workspace_bytes_with_and_without_lean measures the bytes)"""
    for st16, n_str in itertools.product((True, False), (2, 4096, 1_000_000)):
        got, lean = plan(st16=st16, n_str=n_str)
        assert lean == 1 and got[6] == 0 and got[13] == 0 and got[10] == 1
