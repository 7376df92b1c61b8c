"""GPU probe: microseconds per page of explaining many short ranked pages, one by one through ii2_explain_ranges against ONE
ii2_explain_batch call on the same build.

The index and the query shapes are those of scripts/topk_batch_probe.py: what Shard.Put leaves behind (50 terms, 8 per Put, one
segment per Put, one posting per term), --puts of them (default 100: a term is ~16 one-posting lists), plus one segment of
100-posting lists.  Cases (--cases, default s,m), each for Q in --qs (default 1,16,256,4096) pages of at most k = --k (default 10)
ids - the pages ii2_topk_batch returns for the queries, left on the device:
  s   three terms of the unmerged shard: ~48 one-posting lists a query;
  m   three groups of 2 x 100 postings.
Modes, for batch.tiny = 1 and 0:
  single  the Q pages one after the other through ii2_explain_ranges, each on its slice of the ids and of the masks - existing code,
          the yardstick;
  batch   the same Q pages in one ii2_explain_batch call, plus the device time of the batch kernel alone (option profile.events).
All argument arrays are built before the clock starts: wall time is the C calls and the waits.  Samples of the two modes alternate
(single, batch, single, ...), --runs of each after --warmup; a sample repeats its call until it lasts ~20 ms.  Median, min and max
in us per page, one JSON line per (case, Q, batch.tiny), printed and appended to --out.  Every batch is checked word for word against
the yardstick's masks and, for some pages, against plain Python before it is timed."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="s,m")
ap.add_argument("--qs", default="1,16,256,4096")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--runs", type=int, default=11)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--puts", type=int, default=100)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "explain_batch_probe.jsonl"))
ap.add_argument("--note", default=None, help="copied into every row")
args = ap.parse_args()

from inverted_index_2_amd import Context, _lib  # noqa: E402
from inverted_index_2_amd.engine import pack_andnot, pack_explain_batch  # noqa: E402

WEIGHTS = [4, 2, 1]
ctx = Context(0)
rng = np.random.default_rng(7)

# ---- the index ---------------------------------------------------------------------------------------
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


def expect(q, page):
    """the page's rows (one word each) in plain Python; a ranked page holds no id twice"""
    groups = [term_ids[t] for t in q[1:]] if q[0] == "s" else [[m_lists[q[1 + 2 * g]], m_lists[q[2 + 2 * g]]] for g in range(3)]
    sets = [set(int(x) for l in g for x in l) for g in groups]
    return [sum(1 << g for g, s in enumerate(sets) if int(x) in s) for x in page]


def n_lists(q):
    return 6 if q[0] == "m" else sum(len(term_ids[t]) for t in q[1:])


def stats(us):
    us = sorted(us)
    return {"median_us_per_page": round(us[len(us) // 2], 3), "min": round(us[0], 3), "max": round(us[-1], 3)}


def reps_of(fn):
    for _ in range(args.warmup):
        fn()
    t = time.perf_counter()
    fn()
    return max(1, min(2000, int(0.02 / max(time.perf_counter() - t, 1e-6))))


def timed_alternating(fns, nq):
    """us per page of --runs samples of every fn, the samples of the fns taking turns"""
    reps = [reps_of(fn) for fn in fns]
    out = [[] for _ in fns]
    for _ in range(args.runs):
        for i, fn in enumerate(fns):
            t = time.perf_counter()
            for _ in range(reps[i]):
                fn()
            out[i].append((time.perf_counter() - t) / (nq * reps[i]) * 1e6)
    return [stats(o) for o in out]


def single_calls(c, index, qs, d_ids, off, d_masks):
    """the prebuilt argument arrays of one ii2_explain_ranges call per page, and the function that makes the calls"""
    calls = []
    for i, q in enumerate(qs):
        gf, _, gsegs, first, end = pack_andnot(bind(index, q), [])
        hs = (C.c_void_p * max(len(gsegs), 1))(*[s.h for s in gsegs])
        n_ids = int(off[i + 1] - off[i])
        calls.append((len(gf) - 1, hs, gf, first, end, gf.ctypes.data_as(_lib.u64p), first.ctypes.data_as(_lib.u64p), end.ctypes.data_as(_lib.u64p),
                      C.c_void_p(d_ids.ptr + 4 * int(off[i])), n_ids, C.c_void_p(d_masks.ptr + 8 * int(off[i]))))
    lib, h = c.lib, c.h

    def run():
        for n, hs, _, _, _, p_gf, p_first, p_end, p_ids, n_ids, p_masks in calls:
            rc = lib.ii2_explain_ranges(h, n, p_gf, hs, p_first, p_end, p_ids, n_ids, p_masks, n_ids, None)
            assert rc == 0, rc
    return run


def batch_call(c, index, qs, d_ids, off, d_masks, cap):
    t = time.perf_counter()
    qf, gf, qsegs, first, end = pack_explain_batch([bind(index, q) for q in qs])
    pack_us = (time.perf_counter() - t) / max(len(qs), 1) * 1e6
    hs = (C.c_void_p * max(len(qsegs), 1))(*[s.h for s in qsegs])
    ids_off = np.ascontiguousarray(off, np.uint64)
    mask_off = np.zeros(len(qs) + 1, np.uint64)
    st = _lib.ExplainBatchStats()
    keep = (qf, gf, first, end, ids_off)
    u64 = [x.ctypes.data_as(_lib.u64p) for x in (qf, gf, first, end, ids_off, mask_off)]
    pi, pm = C.c_void_p(d_ids.ptr), C.c_void_p(d_masks.ptr)

    def run(cc=c):
        rc = cc.lib.ii2_explain_batch(cc.h, len(qs), u64[0], u64[1], hs, u64[2], u64[3], pi, u64[4], pm, cap, u64[5], C.byref(st))
        assert rc == 0, (rc, cc.lib.ii2_last_error(cc.h))
    return run, mask_off, st, pack_us, keep


index = build(ctx)
c_kernel = Context(0)                                        # device time of the batch kernel alone: the bracketed pass of a call
c_kernel.set_option("profile.events", 1)
rows = []
for case in args.cases.split(","):
    for nq in (int(x) for x in args.qs.split(",")):
        qs = make_queries(case, nq)
        d_ids, _, off, _ = ctx.topk_batch([(bind(index, q), WEIGHTS, args.k, 1, []) for q in qs])      # the pages, left on the device
        total = int(off[-1])
        pages = d_ids.download(total)
        d_single, d_batch = ctx.empty(max(total, 1), np.uint64), ctx.empty(max(total, 1), np.uint64)
        single = single_calls(ctx, index, qs, d_ids, off, d_single)
        single()
        want = d_single.download(total)
        for q in sorted(set(list(range(min(nq, 24))) + list(range(max(nq - 8, 0), nq)))):
            a, b = int(off[q]), int(off[q + 1])
            assert want[a:b].tolist() == expect(qs[q], pages[a:b]), (case, nq, q)
        for tiny in (1, 0):
            row = {"case": case, "Q": nq, "k": args.k, "batch.tiny": tiny, "lists": sum(n_lists(q) for q in qs), "rows": total}
            if args.note:
                row["note"] = args.note
            ctx.set_option("batch.tiny", tiny)
            batch, mask_off, st, row["pack_explain_batch_python_us_per_page"], _keep = batch_call(ctx, index, qs, d_ids, off, d_batch, max(total, 1))
            d_batch.upload(np.full(max(total, 1), 0xA5A5A5A5A5A5A5A5, np.uint64))
            batch()                                          # the results that are being timed are the right ones
            assert np.array_equal(d_batch.download(total), want) and mask_off.tolist() == off.tolist(), (case, nq, tiny)
            row["forms"] = {"tiny": st.n_tiny, "small": st.n_small, "single": st.n_single, "empty": st.n_empty}
            row["hits"] = int(st.n_hits)
            res = timed_alternating([single, batch], nq)
            row["single"], row["batch"] = res
            row["batch_wall_us_per_call"] = round(res[1]["median_us_per_page"] * nq, 1)
            row["single_over_batch"] = round(res[0]["median_us_per_page"] / res[1]["median_us_per_page"], 2)
            row["batch_median_below_single_min"] = res[1]["median_us_per_page"] < res[0]["min"]
            if st.n_single == 0:
                c_kernel.set_option("batch.tiny", tiny)
                batch(c_kernel)
                c_kernel.profile_read()
                dev = []
                for _ in range(7):
                    batch(c_kernel)
                    ms, n = c_kernel.profile_read()
                    dev.append(ms * 1e3)
                row["device_us_per_call_bracketed"] = {"median": round(sorted(dev)[3], 2), "min": round(min(dev), 2), "max": round(max(dev), 2), "pairs": n}
            print(json.dumps(row), flush=True)
            rows.append(row)
        ctx.set_option("batch.tiny", 1)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
c_kernel.close()
ctx.close()
