"""GPU probe: microseconds per query of many short ranked queries, one by one through ii2_topk_weighted_ranges against ONE
ii2_topk_batch call.

The index is that of scripts/group_batch_queries.py: what Shard.Put leaves behind (50 terms, 8 per Put, one segment per Put, one
posting per term), --puts of them (default 100: a term is ~16 one-posting lists), plus one segment of 100-posting lists.  Cases
(--cases, default s,m), each for Q in --qs (default 1,64,4096), k = --k (default 10):
  s   three terms of the unmerged shard, weights 4, 2, 1: ~48 one-posting lists a query;
  m   three groups of 2 x 100 postings, weights 4, 2, 1.
Modes:
  single  the Q queries one after the other through ii2_topk_weighted_ranges - the yardstick.  With --lib it runs on THAT library
          (one built from the commit to compare against), loaded next to the package's own in the same process, with a context and
          segments of its own;
  batch   the same Q queries in one ii2_topk_batch call of the package's library, plus the device time of the batch kernel alone
          (option profile.events).
All argument arrays are built before the clock starts: wall time is the C calls and the waits.  Samples of the two modes alternate
(single, batch, single, ...), --runs of each after --warmup; a sample repeats its call until it lasts ~20 ms.  Median, min and max
in us per query, one JSON line per (case, Q).  Every batch is checked against numpy and against the yardstick's results before it is
timed."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="libii2_hip.so for the yardstick (default: the package's own)")
ap.add_argument("--cases", default="s,m")
ap.add_argument("--qs", default="1,64,4096")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--runs", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--puts", type=int, default=100)
ap.add_argument("--note", default=None, help="copied into every row (which build is which, say)")
args = ap.parse_args()

from inverted_index_2_amd import Context, _lib  # noqa: E402
from inverted_index_2_amd.engine import pack_andnot, pack_topk_batch  # noqa: E402

WEIGHTS = [4, 2, 1]


def context_on(path):
    """a Context whose calls go to the library at `path` (typed like the package's own; entry points it lacks are left out)"""
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, argtypes) in _lib.PROTOTYPES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, argtypes
    c = object.__new__(Context)
    c.lib, c.device, h = lib, 0, C.c_void_p()
    rc = lib.ii2_ctx_create(0, 0, C.byref(h))
    assert rc == 0, rc
    c.h = h
    return c


ctx = Context(0)
yctx = context_on(args.lib) if args.lib else Context(0)
rng = np.random.default_rng(7)

# ---- the index, encoded once per library -------------------------------------------------------------
N_TERMS, PER_PUT = 50, 8
put_terms = [np.sort(rng.choice(N_TERMS, PER_PUT, replace=False)) for _ in range(args.puts)]
m_lists = [np.sort(rng.choice(2000, 100, replace=False)).astype(np.uint32) for _ in range(256)]
term_ids = {t: [np.asarray([v], np.uint32) for v in range(args.puts) if t in put_terms[v]] for t in range(N_TERMS)}


def build(c):
    """(term -> its ranges, the segment of 100-posting lists) on context c"""
    where = {t: [] for t in range(N_TERMS)}
    for v, terms in enumerate(put_terms):
        seg = c.encode_lists([np.asarray([v], np.uint32)] * PER_PUT)
        for j, t in enumerate(terms):
            where[int(t)].append((seg, j, j + 1))
    return where, c.encode_lists(m_lists)


def make_queries(case, nq):
    """abstract queries: ("s", t1, t2, t3) | ("m", six list numbers)"""
    if case == "m":
        return [("m",) + tuple(int(j) for j in rng.choice(256, 6, replace=False)) for _ in range(nq)]
    return [("s",) + tuple(int(t) for t in rng.choice(N_TERMS, 3, replace=False)) for _ in range(nq)]


def bind(index, q):
    where, mseg = index
    if q[0] == "s":
        return [where[q[1]], where[q[2]], where[q[3]]]
    return [[(mseg, q[1 + 2 * g], q[1 + 2 * g] + 1), (mseg, q[2 + 2 * g], q[2 + 2 * g] + 1)] for g in range(3)]


def expect(q, k):
    groups = [term_ids[t] for t in q[1:]] if q[0] == "s" else [[m_lists[q[1 + 2 * g]], m_lists[q[2 + 2 * g]]] for g in range(3)]
    per_group = [np.unique(np.concatenate(g)) if g else np.empty(0, np.uint32) for g in groups]
    ids = np.unique(np.concatenate(per_group)).astype(np.uint32)
    score = np.zeros(ids.size, np.int64)
    for g, w in zip(per_group, WEIGHTS):
        np.add.at(score, np.searchsorted(ids, g), w)
    order = np.lexsort((ids, -score))[:k]
    return ids[order], score[order].astype(np.uint32)


def n_lists(q):
    return 6 if q[0] == "m" else sum(len(term_ids[t]) for t in q[1:])


def stats(us):
    us = sorted(us)
    return {"median_us_per_query": round(us[len(us) // 2], 3), "min": round(us[0], 3), "max": round(us[-1], 3)}


def reps_of(fn):
    for _ in range(args.warmup):
        fn()
    t = time.perf_counter()
    fn()
    return max(1, min(2000, int(0.02 / max(time.perf_counter() - t, 1e-6))))


def timed_alternating(fns, nq):
    """us per query of --runs samples of every fn, the samples of the fns taking turns"""
    reps = [reps_of(fn) for fn in fns]
    out = [[] for _ in fns]
    for _ in range(args.runs):
        for i, fn in enumerate(fns):
            t = time.perf_counter()
            for _ in range(reps[i]):
                fn()
            out[i].append((time.perf_counter() - t) / (nq * reps[i]) * 1e6)
    return [stats(o) for o in out]


def single_calls(c, index, qs, d_ids, d_scores):
    """the prebuilt argument arrays of one ii2_topk_weighted_ranges call per query, and the function that makes the calls"""
    calls = []
    w = (C.c_uint32 * 3)(*WEIGHTS)
    for q in qs:
        gf, gn, gsegs, first, end = pack_andnot(bind(index, q), [])
        hs = (C.c_void_p * max(len(gsegs), 1))(*[s.h for s in gsegs])
        calls.append((len(gn), gf, gn, hs, first, end,
                      (gf.ctypes.data_as(_lib.u64p), gn.ctypes.data_as(_lib.u8p), first.ctypes.data_as(_lib.u64p), end.ctypes.data_as(_lib.u64p))))
    cnt = C.c_uint64()
    counts = []
    lib, h, pi, ps = c.lib, c.h, C.c_void_p(d_ids.ptr), C.c_void_p(d_scores.ptr)

    def run(record=False):
        for n, _, _, hs, _, _, p in calls:
            rc = lib.ii2_topk_weighted_ranges(h, n, p[0], p[1], w, 1, args.k, hs, p[2], p[3], None, pi, ps, C.byref(cnt), None, None)
            assert rc == 0, rc
            if record:
                counts.append(cnt.value)
    return run, counts


def batch_call(c, index, qs, cap, d_ids, d_scores):
    queries = [(bind(index, q), WEIGHTS, args.k, 1, []) for q in qs]
    t = time.perf_counter()
    qf, gf, gn, qsegs, first, end, weight, min_score, k = pack_topk_batch(queries)
    pack_us = (time.perf_counter() - t) / max(len(qs), 1) * 1e6
    hs = (C.c_void_p * max(len(qsegs), 1))(*[s.h for s in qsegs])
    off = np.zeros(len(qs) + 1, np.uint64)
    st = _lib.TopkBatchStats()
    keep = (qf, gf, gn, first, end, weight, min_score, k)
    u64 = [x.ctypes.data_as(_lib.u64p) for x in (qf, gf, first, end)]
    u32 = [x.ctypes.data_as(_lib.u32p) for x in (weight, min_score, k)]
    p_gn, pi, ps, p_off = gn.ctypes.data_as(_lib.u8p), C.c_void_p(d_ids.ptr), C.c_void_p(d_scores.ptr), off.ctypes.data_as(_lib.u64p)

    def run(cc=c):
        rc = cc.lib.ii2_topk_batch(cc.h, len(qs), u64[0], u64[1], p_gn, u32[0], u32[1], u32[2], hs, u64[2], u64[3], None, pi, ps, cap, p_off, None,
                                   C.byref(st))
        assert rc == 0, (rc, cc.lib.ii2_last_error(cc.h))
    return run, off, st, pack_us, keep


index, yindex = build(ctx), build(yctx)
cap = 1 << 20
d_ids, d_scores = ctx.empty(cap), ctx.empty(cap)
yd_ids, yd_scores = yctx.empty(max(args.k, 1)), yctx.empty(max(args.k, 1))
c_kernel = Context(0)                                        # device time of the batch kernel alone: the first bracketed pass of a call
c_kernel.set_option("profile.events", 1)

for case in args.cases.split(","):
    for nq in (int(x) for x in args.qs.split(",")):
        qs = make_queries(case, nq)
        row = {"case": case, "Q": nq, "k": args.k, "lists": sum(n_lists(q) for q in qs), "yardstick_lib": args.lib or "own"}
        if args.note:
            row["note"] = args.note
        batch, off, st, row["pack_topk_batch_python_us_per_query"], _keep = batch_call(ctx, index, qs, cap, d_ids, d_scores)
        batch()                                              # the results that are being timed are the right ones
        ids, scores = d_ids.download(int(off[-1])), d_scores.download(int(off[-1]))
        for q in sorted(set(list(range(min(nq, 24))) + list(range(max(nq - 8, 0), nq)))):
            want_ids, want_scores = expect(qs[q], args.k)
            a, b = int(off[q]), int(off[q + 1])
            assert np.array_equal(ids[a:b], want_ids) and np.array_equal(scores[a:b], want_scores), (case, nq, q)
        row["entries"] = int(off[-1])
        row["forms"] = {"tiny": st.n_tiny, "small": st.n_small, "single": st.n_single, "empty": st.n_empty}
        single, counts = single_calls(yctx, yindex, qs, yd_ids, yd_scores)
        single(record=True)
        assert counts == np.diff(off.astype(np.int64)).tolist(), (case, nq)
        res = timed_alternating([single, batch], nq)
        row["single"], row["batch"] = res
        row["batch_wall_us_per_call"] = round(res[1]["median_us_per_query"] * nq, 1)
        row["single_over_batch"] = round(res[0]["median_us_per_query"] / res[1]["median_us_per_query"], 2)
        row["batch_median_below_single_min"] = res[1]["median_us_per_query"] < res[0]["min"]
        if st.n_single == 0:
            batch(c_kernel)
            c_kernel.profile_read()
            dev = []
            for _ in range(7):
                batch(c_kernel)
                ms, n = c_kernel.profile_read()
                dev.append(ms * 1e3)
            row["device_us_per_call_bracketed"] = {"median": round(sorted(dev)[3], 2), "min": round(min(dev), 2), "max": round(max(dev), 2), "pairs": n}
        print(json.dumps(row), flush=True)
for c in (c_kernel, yctx):
    c.close()
ctx.close()
