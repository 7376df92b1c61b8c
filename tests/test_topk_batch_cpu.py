"""CPU: ii2_topk_batch is wired through every layer - header, export map, binding, host mirror, the Python faces -, its kernel
lives in topk_batch.hip and waits for no other workgroup, the run rule is defined once (topk_batch_run.h), and the two host-only
exports that run the kernel's and the planner's own functions agree with plain integer arithmetic: ii2_topk_batch_run on random and
hand-written runs, ii2_topk_batch_plan on every boundary of the two size classes.  pack_topk_batch's arrays and the case table of
the GPU test are checked here too."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from inverted_index_2_amd import _lib, engine
from tests import topk_batch_cases as bc
from tests import topkw_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "inverted_index_2_amd", "csrc")
OK, EINVAL = 0, -1
FIELDS = ["n_tiny", "n_small", "n_single", "n_empty", "n_staged"]


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
def test_topk_batch_is_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "exports.map")).read(), flags=re.S)
    exported = re.search(r"global:(.*?);\s*local:", text, flags=re.S).group(1)
    declared = set(re.findall(r"\b(ii2_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    for name, arity in (("ii2_topk_batch", 18), ("ii2_topk_batch_run", 6), ("ii2_topk_batch_plan", 10)):
        assert name in declared
        assert any(fnmatch.fnmatchcase(name, pat.strip()) for pat in exported.split(";") if pat.strip())
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == arity
        assert hasattr(lib, name)
    go = open(os.path.join(ROOT, "bindings", "go", "ii2.go")).read()
    assert "C.ii2_topk_batch(" in go and "func (c *Ctx) TopKBatch(" in go and "C.ii2_topk_batch_stats" in go
    assert "func IntersectTopBatch(" in open(os.path.join(ROOT, "bindings", "go", "index.go")).read()


def test_the_host_mirror_exports_the_batch_call():
    from inverted_index_2_amd import host
    assert hasattr(C.CDLL(host.HOST_LIB_PATH), "ii2h_intersect_top_batch")
    assert hasattr(host.InvertedIndex, "intersect_top_batch")


def test_stats_layout_and_the_path_enum():
    assert [f[0] for f in _lib.TopkBatchStats._fields_] == FIELDS
    assert C.sizeof(_lib.TopkBatchStats) == 24
    body = re.search(r"typedef struct \{([^}]*)\}\s*ii2_topk_batch_stats;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [n for decl in re.findall(r"uint(?:32|64)_t ([^;]+);", body) for n in re.split(r",\s*", decl.strip())] == FIELDS
    assert len(engine.path_names()) == 40                       # the ranked family counts no kernel path


def test_the_options_are_documented_and_set():
    assert re.search(r"^ \*   batch\.topk ", _header(), flags=re.M)
    assert '"batch.topk"' in open(os.path.join(CSRC, "api.cpp")).read()


def test_the_kernel_is_built_and_the_rule_is_defined_once():
    src = open(os.path.join(CSRC, "topk_batch.hip")).read()
    assert "lookback.h" not in src and "ii2_lookback_launch" not in src and "atomic" not in src
    for k in ("k_topk_batch<256u, BATCH_TINY_POSTINGS, BATCH_TINY_BLOCKS>", "k_topk_batch<1024u, SMALL_SET_POSTINGS, SMALL_SET_BLOCKS>", "tb_run_score(",
              "tb_run_eligible(", "ss_decode<", "ss_rank<", "ss_block_scan<"):
        assert k in src, k
    assert "build/topk_batch.o" in open(os.path.join(CSRC, "Makefile")).read()
    host = open(os.path.join(CSRC, "setop.cpp")).read()
    assert host.count("tb_run_score(") == 1 and "launch_topk_batch(" in host
    # the weighted query's checks live in one helper that both entry points call
    assert len(re.findall(r"\btopkw_plan\(", host)) == 3
    assert host.count("has weight 0 (drop the group instead)") == 1
    rule = open(os.path.join(CSRC, "topk_batch_run.h")).read()
    assert len(re.findall(r"II2_HD uint32_t tb_run_score\(", rule)) == 1
    # the grouped kernels' rule and BatchQuery stay as they are
    small = open(os.path.join(CSRC, "small_set_device.h")).read()
    assert "tb_run_score" not in small and "ss_group_run_kept" in small and "ss_group_run_reaches" in small


# ---- the run rule ---------------------------------------------------------------------------------------------------------------
def run(lib, tags, n_req, weights):
    score, ex = C.c_uint32(9999), C.c_uint32(9999)
    c_tags = (C.c_uint8 * max(len(tags), 1))(*tags)
    c_w = (C.c_uint8 * max(len(weights), 1))(*weights)
    assert lib.ii2_topk_batch_run(c_tags, len(tags), n_req, c_w, C.byref(score), C.byref(ex)) == OK
    return score.value, ex.value


def plain(tags, n_req, weights):
    return sum(weights[t] for t in set(tags) if t < n_req), int(tags[-1] >= n_req)


def test_run_rule_hand_written(lib):
    w = [3, 5, 7, 11]
    assert run(lib, [0, 2], 4, w) == (10, 0)
    assert run(lib, [1, 1, 3], 4, w) == (16, 0)                 # a repeated tag counts once
    assert run(lib, [0, 1, 4], 4, w) == (8, 1)                  # the excluded tag last
    assert run(lib, [0, 4, 4], 4, w) == (3, 1)
    assert run(lib, [4], 4, w) == (0, 1)                        # a run of the excluded tag alone
    assert run(lib, [3], 4, w) == (11, 0)
    # all 64 tags, weights summing to 255: 63 ones and one 192
    w64 = [1] * 63 + [192]
    assert run(lib, list(range(64)), 64, w64) == (255, 0)
    assert run(lib, list(range(64)) + [64], 64, w64) == (255, 1)
    assert run(lib, [63], 64, w64) == (192, 0)


def test_run_rule_random(lib):
    rng = np.random.default_rng(5)
    for _ in range(2000):
        n_req = int(rng.integers(1, 65))
        weights = [int(x) for x in rng.integers(1, 256, n_req)]
        n = int(rng.integers(1, 66))
        tags = sorted(int(x) for x in rng.integers(0, n_req + 1, n))
        assert run(lib, tags, n_req, weights) == plain(tags, n_req, weights), (tags, n_req, weights)


def test_run_rule_rejects(lib):
    score, ex = C.c_uint32(), C.c_uint32()
    t, w = (C.c_uint8 * 4)(0, 1, 2, 3), (C.c_uint8 * 4)(1, 1, 1, 1)
    assert lib.ii2_topk_batch_run(None, 1, 1, w, C.byref(score), C.byref(ex)) == EINVAL
    assert lib.ii2_topk_batch_run(t, 0, 1, w, C.byref(score), C.byref(ex)) == EINVAL
    assert lib.ii2_topk_batch_run(t, 66, 1, w, C.byref(score), C.byref(ex)) == EINVAL
    assert lib.ii2_topk_batch_run(t, 4, 65, w, C.byref(score), C.byref(ex)) == EINVAL
    assert lib.ii2_topk_batch_run(t, 4, 2, w, C.byref(score), C.byref(ex)) == EINVAL        # tag 3 above n_req = 2
    assert lib.ii2_topk_batch_run(t, 4, 3, w, None, C.byref(ex)) == EINVAL


# ---- the plan -----------------------------------------------------------------------------------------------------------------------
def test_plan_boundaries(lib):
    P = lambda *a, **kw: bc.plan(lib, *a, **kw)
    # (lists, postings, blocks, counted groups, postings of the required groups, k)
    assert P(8, 2048, 8, 3, 2048, 10) == ("tiny", 10)
    assert P(8, 2049, 9, 3, 2049, 10) == ("small", 10)
    assert P(32, 100, 32, 3, 100, 10) == ("tiny", 10)
    assert P(33, 100, 33, 3, 100, 10) == ("small", 10)
    assert P(32, 8192, 32, 3, 8192, 10) == ("small", 10)
    assert P(33, 8193, 33, 3, 8193, 10) == ("single", 10)
    assert P(64, 128, 128, 3, 128, 10) == ("small", 10)
    assert P(64, 129, 129, 3, 129, 10) == ("single", 10)
    assert P(64, 64, 64, 3, 64, 10) == ("small", 10)
    assert P(65, 65, 65, 3, 65, 10) == ("single", 10)
    assert P(64, 64, 64, 64, 64, 10) == ("small", 10)
    assert P(65, 65, 65, 65, 65, 10) == ("single", 10)
    assert P(30, 30, 30, 30, 30, 10) == ("tiny", 10)
    # k below and above the postings of the required groups (excluded lists count toward the stage, not toward the bound)
    assert P(4, 100, 4, 2, 60, 59) == ("tiny", 59)
    assert P(4, 100, 4, 2, 60, 60) == ("tiny", 60)
    assert P(4, 100, 4, 2, 60, 61) == ("tiny", 60)
    assert P(4, 100, 4, 2, 60, 0) == ("tiny", 0)
    assert P(65, 10000, 200, 2, 9000, 1 << 20) == ("single", 9000)
    # no counted group: nothing runs
    assert P(0, 0, 0, 0, 0, 10) == ("empty", 0)
    # the options
    assert P(8, 2048, 8, 3, 2048, 10, tiny=0) == ("small", 10)
    assert P(8, 2048, 8, 3, 2048, 10, topk=0) == ("single", 10)
    assert P(8, 2048, 8, 3, 2048, 10, topk=0, tiny=0) == ("single", 10)
    assert P(0, 0, 0, 0, 0, 10, topk=0, tiny=0) == ("empty", 0)
    form, bound = C.c_uint32(), C.c_uint64()
    assert lib.ii2_topk_batch_plan(1, 1, 1, 1, 1, 1, 1, 1, None, C.byref(bound)) == EINVAL
    assert lib.ii2_topk_batch_plan(1, 1, 1, 1, 1, 1, 1, 1, C.byref(form), None) == EINVAL


# ---- pack_topk_batch ------------------------------------------------------------------------------------------------------------------
def test_pack_topk_batch():
    s0, s1 = object(), object()
    queries = [
        ([[(s0, 0, 2)], [(s1, 1, 2), (s0, 4, 5)]], [3, 9], 10, 2, [[(s1, 0, 1)]]),
        ([[(s1, 2, 3)]], None, 0, 1, []),
        ([], None, 5, 1, []),
        ([[(s0, 1, 2)], [(s0, 2, 3)]], [1, 255], 7, 256, [[(s0, 9, 9)], [(s1, 5, 6)]]),
    ]
    query_first, group_first, group_not, segs, first, end, weight, min_score, k = engine.pack_topk_batch(queries)
    assert query_first.tolist() == [0, 3, 4, 4, 8] and query_first.dtype == np.uint64
    assert group_first.tolist() == [0, 1, 3, 4, 5, 6, 7, 8, 9]
    assert group_not.tolist() == [0, 0, 1, 0, 0, 0, 1, 1] and group_not.dtype == np.uint8
    assert segs == [s0, s1, s0, s1, s1, s0, s0, s0, s1]
    assert first.tolist() == [0, 1, 4, 0, 2, 1, 2, 9, 5] and end.tolist() == [2, 2, 5, 1, 3, 2, 3, 9, 6]
    assert weight.tolist() == [3, 9, 1, 1, 1, 255, 1, 1] and weight.dtype == np.uint32
    assert min_score.tolist() == [2, 1, 1, 256] and min_score.dtype == np.uint32
    assert k.tolist() == [10, 0, 5, 7] and k.dtype == np.uint32
    # no query with weights: group_weight is NULL
    assert engine.pack_topk_batch([([[(s0, 0, 1)]], None, 1, 1, [])])[6] is None
    assert engine.pack_topk_batch([])[0].tolist() == [0]
    with pytest.raises(ValueError, match="query 1: one weight per group"):
        engine.pack_topk_batch([([[(s0, 0, 1)]], [1], 1, 1, []), ([[(s0, 0, 1)]], [1, 2], 1, 1, [])])
    with pytest.raises(ValueError, match="negative"):
        engine.pack_topk_batch([([[(s0, -1, 1)]], [1], 1, 1, [])])


# ---- the case tables ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", bc.CASES, ids=lambda b: b.name)
def test_seam_cases_are_what_they_say(lib, b):
    t, case = b.w, b.w.case
    assert t.total_weight <= 255 and len(t.weights) == len(case.groups)
    for m in t.min_scores:
        assert bc.form_of(lib, t, 10, m)[0] == b.form, m
        ids, scores, hist = wc.reference(case, t.weights, max(t.ks), m)
        assert ids.size > 0, m                                   # every reference is non-trivial
        if len(case.removed):
            assert int(wc.reference(case, t.weights, 0, 1, True)[2].sum()) < int(wc.reference(case, t.weights, 0, 1)[2].sum())
    n_lists, postings, blocks, n_counted, req_postings = bc.sizes(case)
    E = int(wc.reference(case, t.weights, 0, 1)[2].sum())
    if b.name == "capacity_8192":
        assert (n_lists, postings, blocks) == (64, 8192, 64) and sorted(t.ks)[-3:] == [E - 1, E, E + 1]
        # every 512 consecutive eligible docs - what one wave of the counting sort holds - take several scores
        ids, scores = wc.scores_of(case, t.weights)
        assert all(np.unique(scores[i:i + 512]).size >= 8 for i in range(0, ids.size, 512))
    if b.name == "capacity_8193":
        assert (n_lists, postings) == (64, 8193)
    if b.name == "one_class":
        assert (n_lists, postings, blocks, E) == (32, 8192, 32, 8192) and np.unique(wc.scores_of(case, t.weights)[1]).tolist() == [7]
    if b.name == "binary_padded":
        assert postings == 2058 and np.array_equal(np.flatnonzero(wc.reference(case, t.weights, 0, 1)[2]), np.arange(1, 256))
    if b.name == "shared_ids":
        ids, scores = wc.scores_of(case, t.weights)
        assert dict(zip(ids.tolist(), scores.tolist())) == {1: 7, 2: 7, 3: 9, 4: 9, 5: 2, 10: 7}
    if b.name == "required_and_excluded":
        assert wc.scores_of(case, t.weights)[0].tolist() == [1, 2, 4, 5]
    if b.name == "tiny_2048":
        assert (postings, blocks) == (2048, 32)
    if b.name == "tiny_2049":
        assert (postings, blocks) == (2049, 33)
    if b.name == "highest_id":
        assert wc.scores_of(case, t.weights)[0].tolist() == [0, 5, 0xFFFFFFFF]


def test_the_weighted_table_holds_every_form(lib):
    forms = {}
    for t in wc.CASES:
        forms.setdefault(bc.form_of(lib, t, 10, 1)[0], set()).add(t.case.name)
    assert {"small_capacity", "multi_block_wide", "dense_classes", "late_stopwords"} <= forms["small"]
    assert {"many_lists", "every_score_255"} <= forms["single"]
    assert "every_score_binary" in forms["tiny"] and len(forms["tiny"]) >= 20
    assert bc.sizes(wc.BY_NAME["every_score_binary-binary"].case)[1] == 2048
