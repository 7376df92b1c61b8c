"""GPU probe: queries per second of many AND-of-ORs / NOT queries, one by one through ii2_andnot_ranges against ONE
ii2_query_batch_groups call.

The index is what Shard.Put leaves behind (scripts/andnot_probe.py: 50 terms, 8 per Put, one segment per Put, one posting per
term), --puts of them (default 100: a term is ~16 one-posting lists), plus one segment of 100-posting lists and four of
125-posting lists.  Cases (--cases, default s,m,c), each for Q in --qs (default 1,64,4096):
  s   the unmerged-shard shape of DESIGN 4.1h: 2 required terms NOT 1 term, ~48 one-posting lists a query;
  m   2 required groups of 2 x 100 postings NOT 1 group of 2 x 100;
  c   (s) with every 64th query one at the batch kernel's capacity: 64 lists x 125 postings, 3 required groups and 1 excluded
      one of 16 lists each.  Also timed: the same batch WITHOUT those queries plus those queries one by one through the general
      form (andnot.small = 0) - what a work bound in the batch chooser would make of them.
Modes:
  single  the Q queries one after the other through ii2_andnot_ranges (it returns its count: a launch and a wait per query) -
          the yardstick.  With --lib it runs on THAT library (one built from the commit to compare against), loaded next to the
          package's own in the same process, with a context and segments of its own; the same loop then also times the
          one-by-one calls on the package's library (`single_own`) and the batch on THAT library (`batch_yardstick`), so that
          a change of the host code shows as each call's median against the other library's min - max;
  batch   the same Q queries in one ii2_query_batch_groups call of the package's library; plus, for s and m, the device time of
          the batch kernel and of the pack kernel alone (option profile.events; of the batch without its large queries - an (s)
          query whose three terms hold more than 64 lists is one, `large_queries` counts them) - wall time minus these two is what the call
          spends on the host (checking the queries, building their descriptors) and on its two copies and one wait; divided by
          the lists of the batch: host_us_per_list, an upper bound of the descriptor time - and the time the Python layer spends
          flattening the queries (pack_group_batch).
All argument arrays are built before the clock starts: wall time is the C calls and the waits.  Samples of the two modes
alternate (single, batch, single, ...), --runs of each after --warmup; a sample repeats its call until it lasts ~20 ms.  Median,
min and max in us per query, one JSON line per (case, Q).  Every batch is checked against numpy and against the yardstick's
results before it is timed.  --mode batch leaves the yardstick out (profiler runs)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from functools import reduce

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="libii2_hip.so for the yardstick (default: the package's own)")
ap.add_argument("--mode", default="both", choices=["batch", "both"])
ap.add_argument("--cases", default="s,m,c")
ap.add_argument("--qs", default="1,64,4096")
ap.add_argument("--runs", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--puts", type=int, default=100)
ap.add_argument("--note", default=None, help="copied into every row (which build is which, say)")
args = ap.parse_args()

from inverted_index_2_amd import Context, _lib  # noqa: E402
from inverted_index_2_amd.engine import pack_andnot, pack_group_batch  # noqa: E402


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
yctx = None if args.mode == "batch" else context_on(args.lib) if args.lib else Context(0)
rng = np.random.default_rng(7)

# ---- the index, encoded once per library -------------------------------------------------------------
N_TERMS, PER_PUT = 50, 8
put_terms = [np.sort(rng.choice(N_TERMS, PER_PUT, replace=False)) for _ in range(args.puts)]
m_lists = [np.sort(rng.choice(2000, 100, replace=False)).astype(np.uint32) for _ in range(256)]
c_lists = [np.sort(rng.choice(4000, 125, replace=False)).astype(np.uint32) for _ in range(64)]
term_ids = {t: [np.asarray([v], np.uint32) for v in range(args.puts) if t in put_terms[v]] for t in range(N_TERMS)}


def build(c):
    """(term -> its ranges, the segment of 100-posting lists, the four segments of 125-posting lists) on context c"""
    where = {t: [] for t in range(N_TERMS)}
    for v, terms in enumerate(put_terms):
        seg = c.encode_lists([np.asarray([v], np.uint32)] * PER_PUT)
        for j, t in enumerate(terms):
            where[int(t)].append((seg, j, j + 1))
    return where, c.encode_lists(m_lists), [c.encode_lists(c_lists[16 * s:16 * s + 16]) for s in range(4)]


def make_queries(case, nq):
    """abstract queries: ("s", t1, t2, x) | ("m", six list numbers) | ("c",)"""
    qs = []
    for q in range(nq):
        if case == "m":
            qs.append(("m",) + tuple(int(j) for j in rng.choice(256, 6, replace=False)))
        elif case == "c" and q % 64 == 63:
            qs.append(("c",))
        else:
            qs.append(("s",) + tuple(int(t) for t in rng.choice(N_TERMS, 3, replace=False)))
    return qs


def bind(index, q):
    where, mseg, csegs = index
    if q[0] == "s":
        return [where[q[1]], where[q[2]]], [where[q[3]]]
    if q[0] == "m":
        return [[(mseg, q[1], q[1] + 1), (mseg, q[2], q[2] + 1)], [(mseg, q[3], q[3] + 1), (mseg, q[4], q[4] + 1)]], \
               [[(mseg, q[5], q[5] + 1), (mseg, q[6], q[6] + 1)]]
    return [[(csegs[g], 0, 16)] for g in range(3)], [[(csegs[3], 0, 16)]]


def expect(q):
    if q[0] == "s":
        req, ex = [term_ids[q[1]], term_ids[q[2]]], term_ids[q[3]]
    elif q[0] == "m":
        req, ex = [[m_lists[q[1]], m_lists[q[2]]], [m_lists[q[3]], m_lists[q[4]]]], [m_lists[q[5]], m_lists[q[6]]]
    else:
        req, ex = [c_lists[16 * g:16 * g + 16] for g in range(3)], c_lists[48:64]
    sets = [np.unique(np.concatenate(g)) if g else np.empty(0, np.uint32) for g in req]
    return np.setdiff1d(reduce(np.intersect1d, sets), np.concatenate(ex + [np.empty(0, np.uint32)])).astype(np.uint32)


def n_lists(q):
    return {"m": 6, "c": 64}.get(q[0]) or sum(len(term_ids[t]) for t in q[1:])


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


def single_calls(c, index, qs, cap, d_out):
    """the prebuilt argument arrays of one ii2_andnot_ranges call per query, and the function that makes the calls"""
    calls = []
    for q in qs:
        gf, gn, gsegs, first, end = pack_andnot(*bind(index, q))
        hs = (C.c_void_p * max(len(gsegs), 1))(*[s.h for s in gsegs])
        calls.append((len(gn), gf, gn, hs, first, end,
                      (gf.ctypes.data_as(_lib.u64p), gn.ctypes.data_as(_lib.u8p), first.ctypes.data_as(_lib.u64p), end.ctypes.data_as(_lib.u64p))))
    cnt = C.c_uint64()
    counts = []
    lib, h, po = c.lib, c.h, C.c_void_p(d_out.ptr)

    def run(record=False):
        for n, _, _, hs, _, _, p in calls:
            rc = lib.ii2_andnot_ranges(h, n, p[0], p[1], hs, p[2], p[3], None, po, cap, C.byref(cnt))
            assert rc == 0, rc
            if record:
                counts.append(cnt.value)
    return run, counts


def batch_call(c, index, qs, cap, d_out):
    queries = [bind(index, q) for q in qs]
    t = time.perf_counter()
    qf, gf, gn, qsegs, first, end = pack_group_batch(queries)
    pack_us = (time.perf_counter() - t) / max(len(qs), 1) * 1e6
    hs = (C.c_void_p * max(len(qsegs), 1))(*[s.h for s in qsegs])
    off = np.zeros(len(qs) + 1, np.uint64)
    keep = (qf, gf, gn, first, end)
    a = [x.ctypes.data_as(_lib.u64p) for x in (qf, gf)] + [gn.ctypes.data_as(_lib.u8p)] + [x.ctypes.data_as(_lib.u64p) for x in (first, end)]
    po, p_off = C.c_void_p(d_out.ptr), off.ctypes.data_as(_lib.u64p)

    def run(cc=c):
        rc = cc.lib.ii2_query_batch_groups(cc.h, len(qs), a[0], a[1], a[2], hs, a[3], a[4], None, po, cap, p_off)
        assert rc == 0, (rc, cc.lib.ii2_last_error(cc.h))
    return run, off, pack_us, keep


index = build(ctx)
yindex = None if yctx is None else build(yctx)
cap = 1 << 22
d_out = ctx.empty(cap)
yd_out = None if yctx is None else yctx.empty(cap)
# device time of the two kernels alone: profile.events = 2 brackets every second pass of a context, and a batch of short queries
# has exactly two (batch kernel, pack kernel) - a fresh context times the first of them, one that has bracketed one pass before
# (a single short query) the second
c_kernel, c_pack = Context(0), Context(0)
for c in (c_kernel, c_pack):
    c.set_option("profile.events", 2)
c_pack.andnot_ranges(*bind(index, ("m", 0, 1, 2, 3, 4, 5)))
c_pack.profile_read()

for case in args.cases.split(","):
    for nq in (int(x) for x in args.qs.split(",")):
        qs = make_queries(case, nq)
        row = {"case": case, "Q": nq, "lists": sum(n_lists(q) for q in qs), "yardstick_lib": args.lib or "own"}
        if args.note:
            row["note"] = args.note
        batch, off, row["pack_group_batch_python_us_per_query"], _keep = batch_call(ctx, index, qs, cap, d_out)
        batch()                                          # the results that are being timed are the right ones
        ids = d_out.download(int(off[-1]))
        check = sorted(set(list(range(min(nq, 24))) + list(range(max(nq - 8, 0), nq)) + [q for q in (63, 127) if q < nq]))
        for q in check:
            assert np.array_equal(ids[int(off[q]):int(off[q + 1])], expect(qs[q])), (case, nq, q)
        row["ids"] = int(off[-1])
        fns = [batch]
        if yctx is not None:
            single, counts = single_calls(yctx, yindex, qs, cap, yd_out)
            single(record=True)
            assert counts == np.diff(off.astype(np.int64)).tolist(), (case, nq)
            fns = [single, batch]
            if args.lib:                                 # ... and each call on the OTHER library, in the same loop
                y_batch = batch_call(yctx, yindex, qs, cap, yd_out)
                fns += [single_calls(ctx, index, qs, cap, d_out)[0], y_batch[0]]
        res = timed_alternating(fns, nq)
        row["batch"] = res[1 if yctx is not None else 0]
        row["batch_wall_us_per_call"] = round(row["batch"]["median_us_per_query"] * nq, 1)
        if yctx is not None:
            row["single"] = res[0]
            row["batch_over_single_qps"] = round(res[0]["median_us_per_query"] / row["batch"]["median_us_per_query"], 2)
        if len(fns) == 4:
            row["single_own"], row["batch_yardstick"] = res[2], res[3]
        # an (s) query whose three terms hold more than 64 lists is beyond one workgroup: a large query with passes and waits of
        # its own.  The device times and the host time are those of the batch WITHOUT them (`fit_only` when there are any)
        fit = [q for q in qs if q[0] != "s" or n_lists(q) <= 64]
        row["large_queries"] = nq - len(fit)
        if case != "c" and fit:
            b_fit, wall_fit, lists_fit = batch, row["batch_wall_us_per_call"], row["lists"]
            if len(fit) != nq:
                b_fit = batch_call(ctx, index, fit, cap, d_out)[0]
                lists_fit = sum(n_lists(q) for q in fit)
                r = timed_alternating([b_fit], len(fit))[0]
                wall_fit = round(r["median_us_per_query"] * len(fit), 1)
                row["fit_only"] = {"Q": len(fit), "lists": lists_fit, "batch": r, "batch_wall_us_per_call": wall_fit}
            for key, c in (("batch_kernel_device_us", c_kernel), ("pack_kernel_device_us", c_pack)):
                b_fit(c)
                c.profile_read()
                dev = []
                for _ in range(7):
                    b_fit(c)
                    ms, n = c.profile_read()
                    assert n == 1, n                     # (two passes a call, every second one bracketed)
                    dev.append(ms * 1e3)
                row[key] = {"median": round(sorted(dev)[3], 2), "min": round(min(dev), 2), "max": round(max(dev), 2)}
            host = wall_fit - row["batch_kernel_device_us"]["median"] - row["pack_kernel_device_us"]["median"]
            row["host_copies_wait_us_per_call"] = round(host, 1)
            row["host_us_per_list"] = round(host / lists_fit, 4)
            if nq == 4096:                               # every query in the 1024-thread form
                ctx.set_option("batch.tiny", 0)
                row["batch_1024_threads_only"] = timed_alternating([batch], nq)[0]
                ctx.set_option("batch.tiny", 1)
        elif case == "c":
            # what a work bound would do: the capacity-sized queries out of the batch and through the general form one by one
            rest = [q for q in qs if q[0] != "c"]
            stragglers = [q for q in qs if q[0] == "c"]
            row["capacity_queries"] = len(stragglers)
            if stragglers and rest:
                b_rest, _, _, _keep2 = batch_call(ctx, index, rest, cap, d_out)
                general, _ = single_calls(ctx, index, stragglers, cap, d_out)

                def bounded():
                    b_rest()
                    ctx.set_option("andnot.small", 0)
                    general()
                    ctx.set_option("andnot.small", 1)
                r = timed_alternating([batch, bounded], nq)
                row["batch_again"] = r[0]
                row["rest_in_batch_capacity_queries_general_form"] = r[1]
        print(json.dumps(row), flush=True)
for c in (c_kernel, c_pack, yctx):
    if c is not None:
        c.close()
ctx.close()
