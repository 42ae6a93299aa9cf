"""The encode launch plan (plan_encode in csrc/dpt_kernels.hip, through the test-only dpt_debug_launch_plan):
which instantiation every cell of the dispatch matrix launches -- the table of DESIGN.md 2, held here
explicitly -- the branches behind the A/B knobs, and the tail of the launch chain.  No GPU: the plan is
a pure function of the call's properties.  tests/test_gpu_dispatch_matrix.py proves the same cells exact."""
import ctypes
import itertools

import pytest

RAW, PRESPLIT, ATOMS = 0, 1, 2
UNCAPPED, LEN_ONLY = 0x10, 0x20
ROWS16, ROWS64 = 1, 2
GENERIC_PS, GENERIC_RAW, NO_SOLO_WAVE, NO_MID = 1, 2, 4, 8
FORMS = {"raw": RAW, "presplit": PRESPLIT, "atoms": ATOMS}
# tails
EMPTY, SOLO, RESET, SCAN, FOLD, ONE_BATCH = range(6)
# who zeroes an overwritten histogram
NOBODY, BIG_PASS, SCAN_KERNEL, MEMSET = range(4)
FIN_BATCH, FIN_FOLD_MAX, FIN_MAX_BINS = 256, 2048, 1024


@pytest.fixture(scope="module")
def plan():
    from dptok import _lib
    L = _lib.lib()

    def call(variant=ROWS16, mode=RAW, st16=True, edges=False, solo=False, padded=False, no_fallback=False,
             profiled=False, n_str=1000, hist=0, bins=258, knobs=0, rc=0):
        out = (ctypes.c_int * 20)()
        got = L.dpt_debug_launch_plan(variant, mode, st16, edges, solo, padded, no_fallback, profiled, n_str, hist, bins,
                                      knobs, out)
        assert got == rc, (got, list(out))
        v = list(out)
        return {"first": tuple(v[0:6]), "mid": tuple(v[7:10]) if v[6] else None,
                "fallback": tuple(v[11:13]) if v[10] else None, "big_list": v[13], "tail": v[14], "fin_width": v[15],
                "hist": tuple(v[16:20])}
    return call


# ---- the table of DESIGN.md 2.  First pass: (lanes, WIDE, SW, RAW, SOLO, MC); SW stands for the staged id
# width of the cell (1 = int16, 2 = int32).  "ids": the host, device and padded entries; "dp": LEN_ONLY.
SW = "SW"
FIRST = {
    (16, "raw", "ids"): (16, False, SW, True, False, -1),
    (16, "presplit", "ids"): (16, False, SW, False, False, PRESPLIT),
    (16, "atoms", "ids"): (16, True, SW, False, False, ATOMS),
    (16, "raw", "dp"): (16, False, SW, False, False, -1),
    (16, "presplit", "dp"): (16, False, SW, False, False, -1),
    (16, "atoms", "dp"): (16, True, SW, False, False, -1),
    (64, "raw", "ids"): (64, False, 0, True, False, -1),
    (64, "presplit", "ids"): (64, False, 0, False, False, -1),
    (64, "atoms", "ids"): (64, True, 0, False, False, ATOMS),
    (64, "raw", "dp"): (64, False, 0, False, False, -1),
    (64, "presplit", "dp"): (64, False, 0, False, False, -1),
    (64, "atoms", "dp"): (64, True, 0, False, False, -1),
}
SOLO_FIRST = {"raw": (16, False, 2, True, True, -1), "presplit": (16, False, 2, False, True, -1)}
# the 512-byte pass, 16-lane non-raw calls only: (SW, WIDE, MC)
MID = {
    ("presplit", "ids"): (SW, False, PRESPLIT),
    ("atoms", "ids"): (SW, True, ATOMS),
    ("presplit", "dp"): (SW, False, -1),
    ("atoms", "dp"): (SW, True, -1),
}
# the 2048-byte + unbounded launch: (WIDE, RAW)
FALLBACK = {"raw": (False, True), "presplit": (False, False), "atoms": (True, False)}
# every first-pass instantiation the library holds (16), by the rows above and both staging widths
ALL_FIRST = ({tuple(w if x is SW else x for x in t) for t in FIRST.values() for w in (1, 2)} | set(SOLO_FIRST.values()))
ALL_MID = {tuple(w if x is SW else x for x in t) for t in MID.values() for w in (1, 2)}

CELLS = [(lanes, form, st16, entry) for lanes in (16, 64) for form in FORMS for st16 in (True, False)
         for entry in ("host", "device", "padded", "dp")]


def _sub(t, sw):
    return tuple(sw if x is SW else x for x in t)


def _cell_key(lanes, form, st16, entry):
    """the call properties of a dispatch-matrix cell, the staged width its kernels take, and its table column"""
    # (dpt_encode_padded: the ids go straight to the caller's int32 array whatever the vocabulary)
    st16 = st16 and entry != "padded"
    kw = dict(variant=ROWS16 if lanes == 16 else ROWS64, mode=FORMS[form] | (LEN_ONLY if entry == "dp" else 0),
              st16=st16, padded=entry == "padded")
    return kw, (1 if st16 else 2), ("dp" if entry == "dp" else "ids")


def test_table_sizes():
    assert len(ALL_FIRST) == 16 and len(ALL_MID) == 8 and len(set(FALLBACK.values())) == 3


@pytest.mark.parametrize("lanes,form,st16,entry", CELLS)
def test_matrix_cell(plan, lanes, form, st16, entry):
    kw, sw, col = _cell_key(lanes, form, st16, entry)
    got = plan(**kw)
    assert got["first"] == _sub(FIRST[(lanes, form, col)], sw)
    if lanes == 16 and form != "raw":
        assert got["mid"] == _sub(MID[(form, col)], sw) and got["big_list"] == 2
    else:
        assert got["mid"] is None and got["big_list"] == 0
    assert got["fallback"] == FALLBACK[form]
    assert got["tail"] == (RESET if entry == "padded" else FOLD)   # (1000 strings: four batches)
    assert got["fin_width"] == (0 if entry == "padded" else 16 if st16 else 32)
    # edges or the uncapped DP make a call as little "plain" as LEN_ONLY does
    for other in (dict(edges=True), dict(mode=FORMS[form] | UNCAPPED)):
        g2 = plan(**{**kw, **other})
        assert (g2["first"], g2["mid"]) == (_sub(FIRST[(lanes, form, "dp")], sw),
                                            _sub(MID[(form, "dp")], sw) if got["mid"] else None)


@pytest.mark.parametrize("form", ["raw", "presplit"])
@pytest.mark.parametrize("st16", [True, False])
def test_one_string_solo_cells(plan, form, st16):
    got = plan(mode=FORMS[form], st16=st16, solo=True, no_fallback=True, n_str=1)
    assert got == {"first": SOLO_FIRST[form], "mid": None, "fallback": None, "big_list": 0, "tail": SOLO, "fin_width": 0,
                   "hist": (0, 0, 0, 0)}
    # the solo flag means nothing for more than one string, a padded call or (the wave's lanes) ATOMS
    assert plan(mode=FORMS[form], st16=st16, solo=True, n_str=2)["first"] == _sub(FIRST[(16, form, "ids")], 1 if st16 else 2)
    assert plan(mode=FORMS[form], st16=False, solo=True, padded=True, n_str=1)["tail"] == RESET
    atoms = plan(mode=ATOMS, st16=st16, solo=True, no_fallback=True, n_str=1)
    assert atoms["first"] == (16, True, 2, False, False, ATOMS) and atoms["tail"] == SOLO
    # 64-lane vocabularies have no one-string kernel: the lone wave of the usual one
    assert plan(variant=ROWS64, mode=FORMS[form], st16=st16, solo=True, n_str=1)["first"] == FIRST[(64, form, "ids")]


def test_fallback_launch_skipped_only_when_nothing_needs_it(plan):
    for form in FORMS:
        for no_fb, profiled, hist in itertools.product((False, True), (False, True), (0, 1, 2)):
            got = plan(mode=FORMS[form], no_fallback=no_fb, profiled=profiled, hist=hist, n_str=1000)
            hist_zero = hist == 2   # (1000 strings fold: the 2048-byte pass zeroes an overwritten histogram)
            assert got["hist"][2] == (BIG_PASS if hist_zero else NOBODY)
            assert got["fallback"] == (None if no_fb and not profiled and not hist_zero else FALLBACK[form])
            # the 512-byte pass does not look at no_fallback
            assert (got["mid"] is not None) == (form != "raw")


@pytest.mark.parametrize("lanes,form,st16,entry", [c for c in CELLS if c[3] != "dp"])
def test_knob_generic_ps_takes_the_dp_cells_instantiations(plan, lanes, form, st16, entry):
    kw, sw, _ = _cell_key(lanes, form, st16, entry)
    got = plan(knobs=GENERIC_PS, **kw)
    if form == "raw":   # (not a PRESPLIT / ATOMS call)
        assert got == plan(**kw)
        return
    assert got["first"] == _sub(FIRST[(lanes, form, "dp")], sw)
    assert got["mid"] == (_sub(MID[(form, "dp")], sw) if lanes == 16 else None)


@pytest.mark.parametrize("st16", [True, False])
def test_knob_generic_raw(plan, st16):
    sw = 1 if st16 else 2
    assert plan(mode=RAW, st16=st16, knobs=GENERIC_RAW)["first"] == (16, False, sw, False, False, -1)
    for other in (dict(mode=PRESPLIT), dict(mode=ATOMS), dict(variant=ROWS64)):   # 16-lane RAW calls only
        assert plan(st16=st16, knobs=GENERIC_RAW, **other) == plan(st16=st16, **other)


def test_knob_no_solo_wave_takes_the_four_string_kernels(plan):
    for st16 in (True, False):   # (a solo call stages nothing: int32 width)
        raw = plan(mode=RAW, st16=st16, solo=True, no_fallback=True, n_str=1, knobs=NO_SOLO_WAVE)
        ps = plan(mode=PRESPLIT, st16=st16, solo=True, no_fallback=True, n_str=1, knobs=NO_SOLO_WAVE)
        assert raw["first"] == (16, False, 2, True, False, -1) and ps["first"] == (16, False, 2, False, False, PRESPLIT)
        assert raw["tail"] == ps["tail"] == SOLO and raw["fallback"] is ps["fallback"] is None


@pytest.mark.parametrize("lanes,form,st16,entry", CELLS)
def test_knob_no_mid(plan, lanes, form, st16, entry):
    kw, _, _ = _cell_key(lanes, form, st16, entry)
    got, base = plan(knobs=NO_MID, **kw), plan(**kw)
    assert got["mid"] is None and got["big_list"] == 0
    assert {k: v for k, v in got.items() if k not in ("mid", "big_list")} == \
           {k: v for k, v in base.items() if k not in ("mid", "big_list")}


# ---- the tail.  Batches of 256 strings: one -> the finish pass alone; 2..2048 -> it folds the batch sums;
# more -> the scan kernel first.
TAIL_OF = {1: ONE_BATCH, 256: ONE_BATCH, 257: FOLD, 256 * 2048: FOLD, 256 * 2048 + 1: SCAN}
# (tail, histogram: 1 add / 2 overwrite, bins) -> (folded into the finish pass, stored by it, zeroed by, separate pass)
HIST = {
    (ONE_BATCH, 1, 1): (0, 0, NOBODY, 1), (ONE_BATCH, 1, 258): (1, 0, NOBODY, 0), (ONE_BATCH, 1, 1025): (0, 0, NOBODY, 1),
    (ONE_BATCH, 2, 1): (0, 0, MEMSET, 1), (ONE_BATCH, 2, 258): (1, 1, NOBODY, 0), (ONE_BATCH, 2, 1025): (0, 0, MEMSET, 1),
    (FOLD, 1, 1): (0, 0, NOBODY, 1), (FOLD, 1, 258): (1, 0, NOBODY, 0), (FOLD, 1, 1025): (0, 0, NOBODY, 1),
    (FOLD, 2, 1): (0, 0, MEMSET, 1), (FOLD, 2, 258): (1, 0, BIG_PASS, 0), (FOLD, 2, 1025): (0, 0, MEMSET, 1),
    (SCAN, 1, 1): (0, 0, NOBODY, 1), (SCAN, 1, 258): (1, 0, NOBODY, 0), (SCAN, 1, 1025): (0, 0, NOBODY, 1),
    (SCAN, 2, 1): (0, 0, MEMSET, 1), (SCAN, 2, 258): (1, 0, SCAN_KERNEL, 0), (SCAN, 2, 1025): (0, 0, MEMSET, 1),
}


@pytest.mark.parametrize("n_str", [0] + sorted(TAIL_OF))
@pytest.mark.parametrize("padded", [False, True])
def test_tail(plan, n_str, padded):
    assert FIN_BATCH * FIN_FOLD_MAX in TAIL_OF and FIN_MAX_BINS + 1 == 1025
    for hist, bins, st16 in itertools.product((0, 1, 2), (1, 258, 1025), (True, False)):
        got = plan(mode=PRESPLIT, st16=st16, padded=padded, n_str=n_str, hist=hist, bins=bins)
        if n_str == 0:   # no kernel: memsets (id_off[0], the histogram of no strings when it replaces the old one)
            assert got["tail"] == EMPTY and got["hist"] == (0, 0, MEMSET if hist == 2 else NOBODY, 0)
            assert got["mid"] is None and got["fallback"] is None
        elif padded:     # the ids are in place: reset_kernel, and no histogram
            assert (got["tail"], got["fin_width"], got["hist"]) == (RESET, 0, (0, 0, 0, 0))
        else:
            tail = TAIL_OF[n_str]
            assert got["tail"] == tail and got["fin_width"] == (16 if st16 else 32)
            assert got["hist"] == (HIST[(tail, hist, bins)] if hist else (0, 0, 0, 0))


def test_every_plan_names_an_instantiated_kernel_and_none_is_dead(plan):
    first, mid, fb = set(), set(), set()
    keys = itertools.product((ROWS16, ROWS64), (RAW, PRESPLIT, ATOMS), (0, UNCAPPED, LEN_ONLY), *[(False, True)] * 6,
                             (1, 257), (0, 2))
    for variant, mode, flags, st16, edges, solo, padded, no_fb, profiled, n_str, hist in keys:
        for knobs in range(16):
            got = plan(variant=variant, mode=mode | flags, st16=st16, edges=edges, solo=solo, padded=padded,
                       no_fallback=no_fb, profiled=profiled, n_str=n_str, hist=hist, knobs=knobs)   # (asserts rc == 0)
            assert got["first"] in ALL_FIRST and got["mid"] in ALL_MID | {None}
            if knobs == 0:
                first.add(got["first"]), mid.add(got["mid"]), fb.add(got["fallback"])
    assert first == ALL_FIRST
    assert mid == ALL_MID | {None} and fb == set(FALLBACK.values()) | {None}
