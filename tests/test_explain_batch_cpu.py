"""CPU: ii2_explain_batch is wired through every layer - header, export map, ctypes, both Go files, the host mirror, the Python
faces -, its kernel lives in explain_batch.hip and waits for no other workgroup, and the host-only export ii2_explain_batch_plan,
which runs the function the driver bins its queries with, agrees with plain integer arithmetic on every boundary of the size
classes, the list limit and the id limit under both values of both options.  The case table of the GPU test is checked against its
own model here too."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from tests import explain_batch_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "inverted_index_2_amd", "csrc")
OK, EINVAL = 0, -1
FIELDS = ["n_tiny", "n_small", "n_single", "n_empty", "n_rows", "n_words", "n_hits"]
CASES = bc.cases()
BY_NAME = {c.name: c for c in CASES}


def _header():
    return open(os.path.join(ROOT, "include", "ii2.h")).read()


@pytest.fixture(scope="module")
def lib():
    from inverted_index_2_amd import host
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(host.HOST_LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- wiring ------------------------------------------------------------------------------------------------------------------
def test_explain_batch_is_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "exports.map")).read(), flags=re.S)
    exported = re.search(r"global:(.*?);\s*local:", text, flags=re.S).group(1)
    declared = set(re.findall(r"\b(ii2_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    for name, arity in (("ii2_explain_batch", 13), ("ii2_explain_batch_plan", 7)):
        assert name in declared
        assert any(fnmatch.fnmatchcase(name, pat.strip()) for pat in exported.split(";") if pat.strip())
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == arity
        assert hasattr(lib, name)
    go = open(os.path.join(ROOT, "bindings", "go", "ii2.go")).read()
    assert "C.ii2_explain_batch(" in go and "func (c *Ctx) ExplainBatch(" in go and "C.ii2_explain_batch_stats" in go
    assert "MatchedTermsBatch(" in open(os.path.join(ROOT, "bindings", "go", "index.go")).read()


def test_the_python_faces_and_the_host_mirror():
    import inverted_index_2_amd as pkg
    from inverted_index_2_amd import host
    assert callable(pkg.pack_explain_batch) and callable(pkg.explain_batch_plan) and hasattr(pkg.Context, "explain_batch")
    assert hasattr(C.CDLL(host.HOST_LIB_PATH), "ii2h_matched_terms_batch")
    assert hasattr(host.InvertedIndex, "matched_terms_batch")


def test_stats_layout_and_constants():
    assert [f[0] for f in _lib.ExplainBatchStats._fields_] == FIELDS
    assert C.sizeof(_lib.ExplainBatchStats) == 40
    body = re.search(r"typedef struct \{([^}]*)\}\s*ii2_explain_batch_stats;\s*/\* 40 bytes", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [n for decl in re.findall(r"uint(?:32|64)_t ([^;]+);", body) for n in re.split(r",\s*", decl.strip())] == FIELDS
    h = _header()
    assert int(re.search(r"#define II2_EXPLAIN_BATCH_IDS (\d+)u", h).group(1)) == _lib.II2_EXPLAIN_BATCH_IDS == bc.BATCH_IDS
    for name, value in (("EMPTY", bc.EMPTY), ("TINY", bc.TINY), ("SMALL", bc.SMALL), ("SINGLE", bc.SINGLE)):
        assert int(re.search(rf"#define II2_EXPLAIN_BATCH_{name} (\d+)", h).group(1)) == getattr(_lib, f"II2_EXPLAIN_BATCH_{name}") == value
    from inverted_index_2_amd import engine
    assert len(engine.path_names()) == 40                       # explaining counts no kernel path


def test_the_option_is_documented_and_set():
    assert re.search(r"^ \*   batch\.explain ", _header(), flags=re.M)
    assert '"batch.explain"' in open(os.path.join(CSRC, "api.cpp")).read()


def test_the_kernel_is_built_and_waits_for_nobody():
    src = open(os.path.join(CSRC, "explain_batch.hip")).read()
    assert "lookback.h" not in src and "ii2_lookback_launch" not in src and "asm" not in src
    for k in ("k_explain_batch<256u, BATCH_TINY_POSTINGS, BATCH_TINY_BLOCKS>", "k_explain_batch<1024u, SMALL_SET_POSTINGS, SMALL_SET_BLOCKS>", "ss_decode<"):
        assert k in src, k
    assert "build/explain_batch.o" in open(os.path.join(CSRC, "Makefile")).read()
    host = open(os.path.join(CSRC, "setop.cpp")).read()
    assert "launch_explain_batch(" in host and len(re.findall(r"\bexplain_batch_form\(", host)) == 3      # defined once; the driver and the export call it


# ---- the planner ---------------------------------------------------------------------------------------------------------------
def plan(lib, n_lists, n_post, n_blocks, n_ids, explain, tiny):
    form = C.c_uint32(99)
    assert lib.ii2_explain_batch_plan(n_lists, n_post, n_blocks, n_ids, explain, tiny, C.byref(form)) == OK
    return form.value


def test_plan_on_every_boundary(lib):
    E, T, S, L = bc.EMPTY, bc.TINY, bc.SMALL, bc.SINGLE
    hand = {  # (lists, postings, blocks, ids): forms under (explain, tiny) = (1, 1), (1, 0), (0, 1), (0, 0)
        (32, 2048, 32, 10): (T, S, L, L), (32, 2049, 32, 10): (S, S, L, L), (33, 2048, 33, 10): (S, S, L, L),
        (32, 8192, 128, 10): (S, S, L, L), (32, 8193, 128, 10): (L, L, L, L), (32, 8192, 129, 10): (L, L, L, L),
        (64, 64, 32, 10): (T, S, L, L), (65, 65, 32, 10): (L, L, L, L),
        (4, 100, 4, 1024): (T, S, L, L), (4, 100, 4, 1025): (L, L, L, L), (4, 100, 4, 1): (T, S, L, L),
        (4, 100, 4, 0): (E, E, E, E), (0, 0, 0, 10): (E, E, E, E), (0, 0, 0, 0): (E, E, E, E),
    }
    for shape, want in hand.items():
        got = tuple(plan(lib, *shape, e, t) for e, t in bc.OPTIONS)
        assert got == want, shape
        assert got == tuple(bc.form(*shape, e, t) for e, t in bc.OPTIONS), shape
    for n_lists in (1, 63, 64, 65):
        for n_post in (1, 2047, 2048, 2049, 8191, 8192, 8193):
            for n_blocks in (1, 31, 32, 33, 127, 128, 129):
                for n_ids in (0, 1, 1023, 1024, 1025, 1 << 24):
                    for e, t in bc.OPTIONS:
                        assert plan(lib, n_lists, n_post, n_blocks, n_ids, e, t) == bc.form(n_lists, n_post, n_blocks, n_ids, e, t)
    assert lib.ii2_explain_batch_plan(1, 1, 1, 1, 1, 1, None) == EINVAL


def test_engine_plan_and_pack():
    from inverted_index_2_amd import explain_batch_plan, pack_explain_batch
    assert explain_batch_plan(32, 2048, 32, 10) == bc.TINY and explain_batch_plan(32, 2048, 32, 10, batch_tiny=0) == bc.SMALL
    assert explain_batch_plan(32, 2048, 32, 10, batch_explain=0) == bc.SINGLE and explain_batch_plan(1, 1, 1, 0) == bc.EMPTY
    qf, gf, segs, first, end = pack_explain_batch([[[("a", 0, 2), ("b", 1, 3)], []], [], [[("c", 4, 5)]]])
    assert qf.tolist() == [0, 2, 2, 3] and gf.tolist() == [0, 2, 2, 3] and segs == ["a", "b", "c"]
    assert first.tolist() == [0, 1, 4] and end.tolist() == [2, 3, 5] and qf.dtype == gf.dtype == first.dtype == np.uint64


# ---- the case table against its own model ------------------------------------------------------------------------------------------
def test_the_table_covers_what_it_says():
    E, T, S, L = bc.EMPTY, bc.TINY, bc.SMALL, bc.SINGLE
    assert BY_NAME["size_class_edges"].forms(1, 1) == [T, S, S, S, L] and BY_NAME["size_class_edges"].forms(1, 0) == [S, S, S, S, L]
    assert BY_NAME["list_limit"].forms(1, 1) == [S, L] and BY_NAME["id_limit"].forms(1, 1) == [T, L]
    assert BY_NAME["nothing_to_run"].forms(1, 1) == [T, E, E, E, T] and BY_NAME["nothing_to_run"].forms(0, 1) == [L, E, E, E, L]
    assert set(BY_NAME["mixed"].forms(1, 1)) == {E, T, S, L}
    for c in CASES:
        assert all(f in (E, L) for f in c.forms(0, 0)) and all(f != T for f in c.forms(1, 0))
        for s in c.segments:
            for l in s:
                assert l.dtype == np.uint32 and np.all(np.diff(l.astype(np.int64)) > 0)
        assert sum(len(l) for s in c.segments for l in s) <= 20_000
        for v, (base, src) in c.views.items():
            assert all(np.array_equal(c.segments[v][i], c.segments[base][j] if j >= 0 else []) for i, j in enumerate(src))
    ws = BY_NAME["word_seams"]
    assert [ws.n_words(q) for q in range(3)] == [3, 1, 2]
    row = dict(zip(ws.queries[0][1].tolist(), bc.rows(ws.group_lists(0), ws.queries[0][1])))[1234]
    assert row == [1 | 1 << 63, 1, 2]                            # groups 0, 63 | 64 | 129
    bg = BY_NAME["blocks_and_groups"]
    got = dict(zip(bg.queries[0][1].tolist(), bc.rows(bg.group_lists(0), bg.queries[0][1])))
    assert got[3] == [0] and got[0xFFFFFFFE] == [0] and got[0] == [0b1101] and got[0xFFFFFFFF] == [0b1101]
    long_a, long_b = bg.segments[0][0], bg.segments[0][1]
    assert got[int(long_a[255])] == [0b1101] and got[int(long_a[256])] == [0b1101] and got[int(long_b[511])] == got[int(long_b[512])] == [0b0010]


def test_the_model_keeps_a_repeated_ids_first_row():
    rp = BY_NAME["repeats_and_neighbours"]
    ids = rp.queries[0][1]
    r0, r1 = bc.rows(rp.group_lists(0), ids), bc.rows(rp.group_lists(1), ids)
    assert r0[0] != [0] and r0[-1] == [0] and r0[12] == [0] and r0[0] != r1[0]           # other groups, other bits, next query
    assert bc.rows(rp.group_lists(3), rp.queries[3][1]) == [[1]] + [[0]] * 4                # five times the same id
    assert bc.rows([[[1, 2]], [[2], [2, 3]]], [2, 2, 9, 3]) == [[3], [0], [0], [2]]


def test_offsets_and_stats_of_the_model():
    m = BY_NAME["mixed"]
    assert m.mask_off().tolist() == np.cumsum([0] + [m.n_ids(q) * m.n_words(q) for q in range(len(m.queries))]).tolist()
    assert m.expect().size == m.mask_off()[-1] and m.all_ids().size == m.ids_off()[-1]
    assert m.n_words(4) == 0 and m.n_words(7) == 1
    for c in CASES:
        for e, t in bc.OPTIONS:
            st = c.stats(e, t)
            assert st["n_tiny"] + st["n_small"] + st["n_single"] + st["n_empty"] == len(c.queries)
            assert st["n_hits"] == bc.popcount(c.expect()) > 0
