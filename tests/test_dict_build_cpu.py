"""CPU: the dictionary build's wiring and its arithmetic.  ii2_term_chunk and ii2_dict_build_plan are computed by the functions
the driver and the kernels of ii2_dict_build use (csrc/term_device.h, csrc/dict_build.hip), so the order the sort realises and
the passes it runs are pinned here for every case of tests/dict_build_cases.py without a GPU; tests/test_gpu_dict_build.py runs
the same table through the kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from tests import dict_build_cases as cases

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


def chunk(lib, term, c):
    buf = np.frombuffer(term + b"\0", np.uint8)
    key = C.c_uint64(0x77)
    assert lib.ii2_term_chunk(buf.ctypes.data, len(term), c, C.byref(key)) == 0
    return key.value


def plan(lib, terms):
    """(rc, pos_pass, len_pass, n_passes, min_len, max_len) of ii2_dict_build_plan"""
    blob, off = cases.flat(terms)
    pos, lp = np.full(256, 9, np.uint8), np.full(2, 9, np.uint8)
    n, lo, hi = C.c_uint32(99), C.c_uint32(99), C.c_uint32(99)
    rc = lib.ii2_dict_build_plan(blob.ctypes.data, off.ctypes.data, len(terms), pos.ctypes.data, lp.ctypes.data, C.byref(n), C.byref(lo), C.byref(hi))
    return rc, pos, lp, n.value, lo.value, hi.value


# ---- the order ----
@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_chunk_tuple_order_is_bytes_compare(case):
    """sorting by (chunk 0, ..., chunk C - 1, length) equals sorted()"""
    lib = _lib_or_build()
    uniq = sorted(set(case.terms))
    n_chunks = (max(len(t) for t in uniq) + 7) // 8
    got = sorted(uniq[::-1], key=lambda t: tuple(chunk(lib, t, c) for c in range(n_chunks)) + (len(t),))
    assert got == uniq


def test_chunk_values():
    lib = _lib_or_build()
    assert chunk(lib, b"", 0) == 0 and chunk(lib, b"a", 0) == 0x61 << 56 and chunk(lib, b"a", 1) == 0
    t = bytes(range(1, 12))
    assert chunk(lib, t, 0) == int.from_bytes(t[:8], "big") and chunk(lib, t, 1) == int.from_bytes(t[8:] + b"\0" * 5, "big") and chunk(lib, t, 2) == 0
    key = C.c_uint64(5)
    assert lib.ii2_term_chunk(None, 3, 0, C.byref(key)) == -1 and key.value == 5
    assert lib.ii2_term_chunk(None, 0, 0, C.byref(key)) == 0 and key.value == 0
    assert lib.ii2_term_chunk(np.frombuffer(b"ab", np.uint8).ctypes.data, 2, 0, None) == -1


# ---- the plan ----
@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_plan_equals_the_numpy_restatement(case):
    lib = _lib_or_build()
    rc, pos, lp, n, lo, hi = plan(lib, case.terms)
    w_pos, w_lp, w_n, w_lo, w_hi = cases.numpy_plan(case.terms)
    assert rc == 0
    assert pos.tolist() == w_pos.tolist() and lp.tolist() == w_lp.tolist() and (n, lo, hi) == (w_n, w_lo, w_hi)
    if "len_pass" in case.expect:
        assert lp.tolist() == case.expect["len_pass"]
    if "no_pass_before" in case.expect:
        assert not pos[: case.expect["no_pass_before"]].any() and pos[case.expect["no_pass_before"]:].any()
    if "n_passes" in case.expect:
        assert n == case.expect["n_passes"]


def test_plan_argument_errors():
    lib = _lib_or_build()
    assert plan(lib, cases.TOO_LONG)[0] == -5                 # a term of 257 bytes
    assert plan(lib, [b"z" * 256])[0] == 0
    rc, pos, lp, n, lo, hi = plan(lib, [])
    assert rc == 0 and not pos.any() and not lp.any() and (n, lo, hi) == (0, 0, 0)
    blob = np.frombuffer(b"abcd", np.uint8)
    pos, lp = np.zeros(256, np.uint8), np.zeros(2, np.uint8)
    n, lo, hi = C.c_uint32(), C.c_uint32(), C.c_uint32()
    outs = [pos.ctypes.data, lp.ctypes.data, C.byref(n), C.byref(lo), C.byref(hi)]
    good = np.array([0, 1, 4], np.uint64)
    assert lib.ii2_dict_build_plan(blob.ctypes.data, good.ctypes.data, 2, *outs) == 0
    for off in (np.array([1, 1, 4], np.uint64), np.array([0, 3, 1], np.uint64)):       # does not start at 0; descends
        assert lib.ii2_dict_build_plan(blob.ctypes.data, off.ctypes.data, 2, *outs) == -1
    assert lib.ii2_dict_build_plan(None, good.ctypes.data, 2, *outs) == -1
    assert lib.ii2_dict_build_plan(blob.ctypes.data, None, 2, *outs) == -1
    assert lib.ii2_dict_build_plan(blob.ctypes.data, good.ctypes.data, 1 << 31, *outs) == -5
    for i in range(5):
        o = list(outs)
        o[i] = None
        assert lib.ii2_dict_build_plan(blob.ctypes.data, good.ctypes.data, 2, *o) == -1
    assert lib.ii2_dict_build_plan(None, None, 0, *outs) == 0 and n.value == 0


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_lsd_simulation_driven_by_the_plan_sorts(case):
    """a stable least-significant-first sort that runs only the plan's passes - the length bytes, then the byte positions from
    the last to the first - leaves the terms in bytes.Compare order, equal terms adjacent in input order"""
    lib = _lib_or_build()
    rc, pos, lp, n, lo, hi = plan(lib, case.terms)
    assert rc == 0
    terms = case.terms
    order = list(range(len(terms)))
    ran = 0
    for b in range(2):
        if lp[b]:
            order.sort(key=lambda i: (len(terms[i]) >> (8 * b)) & 0xFF)         # (list.sort is stable)
            ran += 1
    for p in range(255, -1, -1):
        if pos[p]:
            order.sort(key=lambda i: terms[i][p] if p < len(terms[i]) else 0)
            ran += 1
    assert ran == n
    got = [terms[i] for i in order]
    assert got == sorted(terms)
    for a, b in zip(order, order[1:]):
        assert terms[a] != terms[b] or a < b


# ---- wiring ----
def _header():
    return re.sub(r"/\*.*?\*/", "", _read("include", "ii2.h"), flags=re.S)


NEW = {"ii2_dict_build": 8, "ii2_dict_info": 3, "ii2_dict_export": 4, "ii2_term_chunk": 4, "ii2_dict_build_plan": 8}


def test_header_declares_the_entry_points_and_the_limit():
    header = _header()
    symbols = set(re.findall(r"\b(ii2_[a-z0-9_]+)\s*\(", header))
    assert set(NEW) <= symbols
    assert re.search(r"#define\s+II2_DICT_BUILD_MAX_TERM\s+256u", header)
    assert "ii2_dict_build_stats" in header


def test_prototypes_and_the_stats_structure():
    header = _header()
    for name, arity in NEW.items():
        assert name in _lib.PROTOTYPES, name
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == arity, name
        declared = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        assert len(declared.split(",")) == arity, name
    assert [f[0] for f in _lib.DictBuildStats._fields_] == ["n_terms", "n_unique", "n_bytes", "min_len", "max_len", "n_passes", "pad"]
    assert C.sizeof(_lib.DictBuildStats) == 40


def test_makefile_object_and_exports():
    mk = _read("inverted_index_2_amd", "csrc", "Makefile")
    objs = next(line for line in mk.splitlines() if line.startswith("OBJS"))
    assert "build/dict_build.o" in objs.split()
    hdrs = next(line for line in mk.splitlines() if line.startswith("HDRS"))
    assert "radix_device.h" in hdrs.split()
    assert "ii2_*" in _read("inverted_index_2_amd", "csrc", "exports.map")
    lib = _lib_or_build()
    for name in NEW:
        assert hasattr(lib, name), name


def test_go_binding_declares_the_calls():
    go = _read("bindings", "go", "ii2.go")
    for c_name, go_name in (("ii2_dict_build", "DictBuild"), ("ii2_dict_info", "DictInfo"), ("ii2_dict_export", "DictExport")):
        assert "C.%s(" % c_name in go and re.search(r"func \([a-z]+ \*[A-Za-z]+\) %s\(" % go_name, go), go_name


def test_host_mirror_has_the_build_switch():
    src = _read("inverted_index_2_amd", "host", "host_index.cpp")
    assert "int ii2h_set_build(" in src and "ii2_dict_build(" in src and "ii2_dict_export(" in src and "void SetBuild(" in src
    assert "def set_build(" in _read("inverted_index_2_amd", "host.py")
    from inverted_index_2_amd import host
    if not os.path.exists(host.HOST_LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    C.CDLL(_lib.LIB_PATH)        # dependency first
    assert hasattr(C.CDLL(host.HOST_LIB_PATH), "ii2h_set_build")


def test_python_faces():
    from inverted_index_2_amd import Context, host
    from inverted_index_2_amd.engine import Dictionary
    assert callable(getattr(Context, "build_dictionary", None))
    assert callable(getattr(Dictionary, "export", None)) and callable(getattr(Dictionary, "info", None))
    assert callable(getattr(host.InvertedIndex, "set_build", None))


def test_both_sorts_share_the_pass_and_neither_waits_between_workgroups():
    db, sb, shared = (_read("inverted_index_2_amd", "csrc", f) for f in ("dict_build.hip", "seg_build.hip", "radix_device.h"))
    for src in (db, shared):
        assert "lookback.h" not in src and "ii2_lookback_launch" not in src
    for src in (db, sb):
        assert '#include "radix_device.h"' in src
        for part in ("sb_wave_rank(", "sb_tile_bases(", "sb_stage_slot(", "sb_hist_count("):
            assert part in src, part
        assert "__ballot(bit)" not in src              # the ranking loop lives in the shared header alone
        assert "struct BuildBlock" not in src
    assert shared.count("__ballot(bit)") == 1 and shared.count("struct BuildBlock") == 1
    assert '#include "term_device.h"' in db
    for k in ("k_db_plan", "k_db_gather", "k_db_hist", "k_db_scatter", "k_db_heads", "k_db_bytes"):
        assert k in db, k
