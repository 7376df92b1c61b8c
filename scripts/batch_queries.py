"""GPU probe: queries per second of many small AND / OR queries, one by one against ii2_query_batch.

Queries are drawn from one synthetic Zipf dictionary (synth.zipf_list: the term of rank r holds D / r postings) whose lists
are device-resident in one segment.  Shapes: AND of 10 + 44 postings, AND of 100 + 434, OR of 8 x 100, OR of 64 x 20 (the
shapes DESIGN 4.1c quotes) and a mixed batch with 1 % large queries.  For Q in {1, 64, 4096}:
  single  the Q queries one after the other through ii2_intersect_async (one ii2_ctx_sync at the end) / ii2_union (it returns
          its count: one wait per query) - the yardstick; run it with --lib pointing at a library built from the commit to
          compare against;
  batch   the same Q queries in one ii2_query_batch call; plus the device time of the batch kernel and of the pack kernel
          alone (option profile.events; wall time minus these two is what the call spends on the host - checking the queries,
          building their descriptors - and on its two copies and one wait) and the time the Python layer spends flattening the
          queries (pack_batch).
All argument arrays are built before the clock starts: wall time is the C calls and the waits.  Warm-up runs, then --runs timed
runs; median, min and max in us per query, one JSON line per (shape, Q, mode)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="libii2_hip.so to load instead of the package's own")
ap.add_argument("--mode", default="both", choices=["single", "batch", "both"])
ap.add_argument("--runs", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--per-class", type=int, default=256, help="lists of every size class in the dictionary")
args = ap.parse_args()

from inverted_index_2_amd import _lib  # noqa: E402
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
    other = C.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.PROTOTYPES if not hasattr(other, n)]:      # a library from before an entry point (this probe's
        _lib.PROTOTYPES.pop(name)                                           # ii2_query_batch among them: the yardstick only)
from inverted_index_2_amd import Context, synth  # noqa: E402
from inverted_index_2_amd.engine import pack_batch  # noqa: E402

D = args.docs
SIZES = (10, 20, 44, 100, 434, 50_000)
ctx = Context(0)
rng = np.random.default_rng(7)
lists, cls = [], {}
for n in SIZES:
    k = args.per_class if n < 10_000 else 4
    first = len(lists)
    r0 = D // n
    for i in range(k):                                   # ranks around D / n: lists of about n postings
        lists.append(synth.zipf_list(max(r0 - i, 1), D))
    cls[n] = (first, first + k)
seg = ctx.encode_lists(lists)
have_batch = "ii2_query_batch" in _lib.PROTOTYPES
# device time of the two kernels alone: profile.events = 2 brackets every second pass of a context, and a batch of small queries
# has exactly two (batch kernel, pack kernel) - a fresh context times the first of them, one that has bracketed one pass before
# (a single small union) the second
c_kernel = c_pack = None
if have_batch and args.mode != "single":
    c_kernel, c_pack = Context(0), Context(0)
    for c in (c_kernel, c_pack):
        c.set_option("profile.events", 2)
    c_pack.union([(seg, cls[10][0]), (seg, cls[10][0] + 1)])
    c_pack.profile_read()


def pick(n):
    a, b = cls[n]
    return int(rng.integers(a, b))


def shape_queries(shape, nq):
    qs = []
    for q in range(nq):
        if shape == "and_10_44":
            qs.append(("and", [pick(10), pick(44)]))
        elif shape == "and_100_434":
            qs.append(("and", [pick(100), pick(434)]))
        elif shape == "or_8x100":
            qs.append(("or", [pick(100) for _ in range(8)]))
        elif shape == "or_64x20":
            qs.append(("or", [pick(20) for _ in range(64)]))
        else:                                            # mixed: the four shapes in turn, 1 % large (two lists of ~50 000 postings)
            if q % 100 == 99:
                qs.append(("and" if q % 200 == 99 else "or", [pick(50_000), pick(50_000)]))
            else:
                qs.append(shape_queries(("and_10_44", "and_100_434", "or_8x100", "or_64x20")[q % 4], 1)[0])
    return qs


def stats(us):
    us = sorted(us)
    return {"median_us_per_query": round(us[len(us) // 2], 3), "min": round(us[0], 3), "max": round(us[-1], 3)}


def timed(fn, nq):
    """us per query of --runs samples; a sample repeats fn until it lasts ~20 ms (a shorter window times the clock)"""
    for _ in range(args.warmup):
        fn()
    ctx.sync()
    t = time.perf_counter()
    fn()
    reps = max(1, min(2000, int(0.02 / max(time.perf_counter() - t, 1e-6))))
    out = []
    for _ in range(args.runs):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        out.append((time.perf_counter() - t) / (nq * reps) * 1e6)
    return out


def expect(name, ls):
    if name == "or":
        return np.unique(np.concatenate([lists[j] for j in ls]))
    w = lists[ls[0]]
    for j in ls[1:]:
        w = np.intersect1d(w, lists[j], assume_unique=True)
    return w


cap = 1 << 23
d_out = ctx.empty(cap)
d_cnt = ctx.empty(8, np.uint64)
for shape in ("and_10_44", "and_100_434", "or_8x100", "or_64x20", "mixed_1pct_large"):
    for nq in (1, 64, 4096):
        qs = shape_queries(shape, nq)
        row = {"shape": shape, "Q": nq}
        if args.mode in ("single", "both"):
            calls = []
            for name, ls in qs:
                segs = (C.c_void_p * len(ls))(*[seg.h] * len(ls))
                idx = (C.c_uint64 * len(ls))(*ls)
                calls.append((name == "and", len(ls), segs, idx))
            cnt = C.c_uint64()
            lib, h, po, pc = ctx.lib, ctx.h, C.c_void_p(d_out.ptr), C.c_void_p(d_cnt.ptr)

            def single():
                for is_and, n, segs, idx in calls:
                    if is_and:
                        rc = lib.ii2_intersect_async(h, n, segs, idx, None, po, cap, pc)
                    else:
                        rc = lib.ii2_union(h, n, segs, idx, None, po, cap, C.byref(cnt))
                    assert rc == 0
                ctx.sync()

            row["single"] = stats(timed(single, nq))
        if args.mode in ("batch", "both") and have_batch:
            queries = [(name, [(seg, j, j + 1) for j in ls]) for name, ls in qs]
            t = time.perf_counter()
            op, qf, qsegs, first, end = pack_batch(queries)
            row["pack_batch_python_us_per_query"] = round((time.perf_counter() - t) / nq * 1e6, 3)
            hs = (C.c_void_p * len(qsegs))(*[s.h for s in qsegs])
            off = np.zeros(nq + 1, np.uint64)
            a = [op.ctypes.data_as(_lib.u8p), qf.ctypes.data_as(_lib.u64p), hs, first.ctypes.data_as(_lib.u64p), end.ctypes.data_as(_lib.u64p)]

            def batch(c=ctx):
                rc = c.lib.ii2_query_batch(c.h, nq, a[0], a[1], a[2], a[3], a[4], None, C.c_void_p(d_out.ptr), cap, off.ctypes.data_as(_lib.u64p))
                assert rc == 0, rc

            batch()                                      # the results that are being timed are the right ones
            ids = d_out.download(int(off[-1]))
            for q in list(range(min(nq, 24))) + list(range(max(nq - 8, 0), nq)) + ([99, 199] if nq > 200 else []):
                assert np.array_equal(ids[int(off[q]):int(off[q + 1])], expect(*qs[q])), (shape, nq, q)
            row["batch"] = stats(timed(batch, nq))
            if nq == 4096:                               # every small query in the 1024-thread form
                ctx.set_option("batch.tiny", 0)
                row["batch_1024_threads_only"] = stats(timed(batch, nq))
                ctx.set_option("batch.tiny", 1)
                if shape != "mixed_1pct_large":
                    c_kernel.set_option("batch.tiny", 0)
                    batch(c_kernel)
                    c_kernel.profile_read()
                    dev = []
                    for _ in range(7):
                        batch(c_kernel)
                        dev.append(c_kernel.profile_read()[0] * 1e3)
                    c_kernel.set_option("batch.tiny", 1)
                    row["batch_kernel_device_us_1024_threads_only"] = round(sorted(dev)[3], 2)
            if shape != "mixed_1pct_large":              # (its large queries bracket passes of their own)
                for key, c in (("batch_kernel_device_us", c_kernel), ("pack_kernel_device_us", c_pack)):
                    batch(c)
                    c.profile_read()
                    dev = []
                    for _ in range(7):
                        batch(c)
                        ms, n = c.profile_read()
                        assert n == 1, n
                        dev.append(ms * 1e3)
                    row[key] = {"median": round(sorted(dev)[3], 2), "min": round(min(dev), 2), "max": round(max(dev), 2)}
            row["batch_wall_us_per_call"] = round(row["batch"]["median_us_per_query"] * nq, 1)
            if "single" in row:
                row["batch_over_single_qps"] = round(row["single"]["median_us_per_query"] / row["batch"]["median_us_per_query"], 2)
        print(json.dumps(row), flush=True)
for c in (c_kernel, c_pack):
    if c is not None:
        c.close()
ctx.close()
