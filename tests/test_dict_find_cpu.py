"""CPU: the term lookup's wiring and its arithmetic.  ii2_term_bounds answers one probe against one host dictionary by the
functions the kernel of ii2_dict_find runs (csrc/term_device.h) - the 8-byte keys, the comparison, the bisection and the
prefix rule - so every case of tests/dict_cases.py is pinned here without a GPU; tests/test_gpu_dict_find.py runs the same
table through the kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from tests import dict_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "inverted_index_2_amd", "csrc")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _lib_or_build():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def term_bounds(lib, terms, probe, prefix):
    blob, off = dict_cases.flat(terms)
    blob = np.frombuffer(blob, np.uint8)
    off = np.array(off, np.uint64)
    pr = np.frombuffer(probe + b"\0", np.uint8)
    first, end = C.c_uint64(77), C.c_uint64(77)
    rc = lib.ii2_term_bounds(blob.ctypes.data, off.ctypes.data, len(terms), pr.ctypes.data, len(probe), prefix, C.byref(first), C.byref(end))
    assert rc == 0, rc
    return first.value, end.value


# ---- wiring ----
def test_header_declares_both_entry_points():
    header = re.sub(r"/\*.*?\*/", "", _read("include", "ii2.h"), flags=re.S)
    assert re.search(r"\bint\s+ii2_dict_find\s*\(\s*ii2_ctx\s*\*", header)
    assert re.search(r"\bint\s+ii2_term_bounds\s*\(\s*const\s+uint8_t\s*\*", header)


def test_binding_arity_matches_the_header():
    header = re.sub(r"/\*.*?\*/", "", _read("include", "ii2.h"), flags=re.S)
    for name in ("ii2_dict_find", "ii2_term_bounds"):
        args = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        assert len(args.split(",")) == len(_lib.PROTOTYPES[name][1]), name
    assert len(_lib.PROTOTYPES["ii2_dict_find"][1]) == 11 and len(_lib.PROTOTYPES["ii2_term_bounds"][1]) == 8


def test_export_map_and_library_carry_the_symbols():
    assert "ii2_*" in _read("inverted_index_2_amd", "csrc", "exports.map")
    lib = _lib_or_build()
    assert hasattr(lib, "ii2_dict_find") and hasattr(lib, "ii2_term_bounds")


def test_makefile_builds_the_kernel_and_tracks_the_header():
    mk = _read("inverted_index_2_amd", "csrc", "Makefile")
    assert "build/dict_find.o" in mk and "term_device.h" in mk
    assert os.path.exists(os.path.join(CSRC, "dict_find.hip"))


def test_go_binding_declares_the_call():
    go = _read("bindings", "go", "ii2.go")
    assert "ii2_dict_find" in go and "func (c *Ctx) DictFind(" in go


def test_host_mirror_has_the_resolve_switch():
    src = _read("inverted_index_2_amd", "host", "host_index.cpp")
    assert "int ii2h_set_resolve(" in src and "ii2_dict_find(" in src and "RESOLVE_MIN_PAIRS" in src
    assert "def set_resolve(" in _read("inverted_index_2_amd", "host.py")


def test_term_device_h_is_the_only_definition_of_the_comparison():
    defined = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".h", ".hip", ".cpp")):
            text = _read("inverted_index_2_amd", "csrc", f)
            for name in ("term_cmp", "term_bound", "term_in_prefix_run"):
                if re.search(r"\b(?:int|bool|uint32_t)\s+%s\s*\(" % name, text):
                    defined.setdefault(name, []).append(f)
            if f != "term_device.h":
                assert not re.search(r"\bstruct\s+TermRef\b", text), f
    assert defined == {"term_cmp": ["term_device.h"], "term_bound": ["term_device.h"], "term_in_prefix_run": ["term_device.h"]}
    for f in ("align.hip", "dict_find.hip"):
        assert '#include "term_device.h"' in _read("inverted_index_2_amd", "csrc", f), f


# ---- the table ----
def test_the_table_covers_the_seams():
    names = {c.name for c in dict_cases.CASES}
    assert len(names) == len(dict_cases.CASES)
    assert {len(c.dicts) for c in dict_cases.CASES} >= {1, 3, 64}
    assert any(len(d) >= 5000 for c in dict_cases.CASES for d in c.dicts)
    assert any(not d for c in dict_cases.CASES for d in c.dicts)
    lens = {len(t) for c in dict_cases.CASES for d in c.dicts for t in d}
    assert {0, 7, 8, 9} <= lens
    for c in dict_cases.CASES:
        assert len(c.probes) == len(c.flags) and set(c.flags) <= {0, 1}
        assert all(d == sorted(set(d)) for d in c.dicts)
        assert len(c.probes) * sum(len(d) for d in c.dicts) < 5_000_000       # seconds on the CPU


@pytest.mark.parametrize("case", dict_cases.CASES, ids=lambda c: c.name)
def test_term_bounds_equals_the_python_expectation(case):
    lib = _lib_or_build()
    for d in case.dicts[:8]:                      # (the k = 64 case repeats sizes: eight of its dictionaries carry them all)
        for p, f in zip(case.probes, case.flags):
            assert term_bounds(lib, d, p, f) == dict_cases.expected(d, p, f), (case.name, p, f)


def test_term_bounds_argument_errors():
    lib = _lib_or_build()
    blob = np.frombuffer(b"abc\0", np.uint8)
    off = np.array([0, 1, 3], np.uint64)
    first, end = C.c_uint64(5), C.c_uint64(6)
    ok = lambda *a: lib.ii2_term_bounds(*a)
    args = [blob.ctypes.data, off.ctypes.data, 2, blob.ctypes.data, 1, 0, C.byref(first), C.byref(end)]
    assert ok(*args) == 0 and (first.value, end.value) == (0, 1)

    def bad(i, v, code=-1):
        a = list(args)
        a[i] = v
        first.value, end.value = 5, 6
        assert ok(*a) == code, (i, v)
        if i not in (6, 7):
            assert (first.value, end.value) == (5, 6)          # nothing written

    bad(6, None)
    bad(7, None)
    bad(1, None)
    bad(0, None)                                   # bytes named by the offsets, none given
    bad(3, None)                                   # probe_len > 0 without a probe
    bad(5, 2)
    bad(5, -1)
    bad(2, 1 << 31, -5)
    late, down = np.array([1, 2, 3], np.uint64), np.array([0, 2, 1], np.uint64)
    bad(1, late.ctypes.data)                       # does not start at 0
    bad(1, down.ctypes.data)                       # descends
    # no terms: NULL arrays are fine, the answer is [0, 0)
    assert ok(None, None, 0, blob.ctypes.data, 1, 1, C.byref(first), C.byref(end)) == 0 and (first.value, end.value) == (0, 0)
    assert ok(None, None, 0, None, 0, 0, C.byref(first), C.byref(end)) == 0 and (first.value, end.value) == (0, 0)
