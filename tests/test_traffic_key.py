"""The key of the traffic record (tools/pmc_traffic.py: bench.py reports profiles/pmc_traffic.json only when
source_hash() matches it) covers the whole dpt_kernels.hip translation unit: every file under csrc/ the unit
reaches by quoted #include is in SRC, and a change to any one of them changes the key.  CPU only."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dp-tokenization_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pmc_traffic  # noqa: E402


def read_src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def unit_files(top="dpt_kernels.hip"):
    """top and every file under csrc/ it includes by `#include "..."`, transitively, in include order."""
    seen = []

    def visit(name):
        if name in seen:
            return
        seen.append(name)
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', read_src(name), flags=re.M):
            path = os.path.normpath(os.path.join(CSRC, os.path.dirname(name), inc))
            if os.path.dirname(path) == CSRC and os.path.exists(path):   # (include/dpt.h is the public ABI, not csrc/)
                visit(os.path.basename(path))

    visit(top)
    return seen


def test_key_lists_the_whole_kernel_unit():
    unit = unit_files()
    assert "dpt_tok_lds.h" in unit and "dpt_lean_hint.h" in unit   # the walk follows nested includes
    missing = [f for f in unit if f not in pmc_traffic.SRC]
    assert not missing, "files of the dpt_kernels.hip unit missing from pmc_traffic.SRC: %s" % missing
    assert len(set(pmc_traffic.SRC)) == len(pmc_traffic.SRC)
    for f in pmc_traffic.SRC:
        assert os.path.exists(os.path.join(CSRC, f)), f


def test_build_sed_reaches_the_unit():
    """tools/build_sed.sh names the unit's text by patterns: every file of the unit matches one, except the interface
    headers the unit shares with the host code (dpt_internal.h and what it includes)."""
    import fnmatch
    with open(os.path.join(ROOT, "tools", "build_sed.sh")) as fh:
        patterns = re.findall(r"dp-tokenization_amd/csrc/(dpt_[\w*.]+)", fh.read())
    shared = unit_files("dpt_internal.h")
    missed = [f for f in unit_files() if f not in shared and not any(fnmatch.fnmatch(f, p) for p in patterns)]
    assert patterns and not missed, "files of the unit that build_sed.sh does not edit: %s" % missed


def test_key_changes_with_every_file():
    texts = {f: read_src(f) for f in pmc_traffic.SRC}
    base = pmc_traffic.source_hash(read=texts.__getitem__)
    assert base == pmc_traffic.source_hash()
    keys = {base}
    for f in pmc_traffic.SRC:
        key = pmc_traffic.source_hash(read=lambda g, f=f: texts[g] + "\nint altered;\n" if g == f else texts[g])
        assert key not in keys, "altering %s gives a key already seen" % f
        keys.add(key)
    # comments and whitespace are not part of the key
    assert pmc_traffic.source_hash(read=lambda g: texts[g] + "\n   // a comment\n") == base
