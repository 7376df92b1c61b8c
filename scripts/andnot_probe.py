"""ii2_andnot_ranges against what a caller had to do without it, wall clock, every case checked against numpy at the size it is timed:
  yardstick  ii2_intersect_ranges (required groups) + ii2_union_ranges (excluded lists) + two ii2_copy_d2h + np.setdiff1d - every
             library that has ii2_intersect_ranges can run it: --lib points at one built from the commit to compare with;
  new        one ii2_andnot_ranges + one ii2_copy_d2h of the result (skipped when the library lacks the entry point).
Cases (PROBE_CASES=s,s120,sp,a,c; default all):
  s     2 required terms NOT 1 term over 200 Put segments (50 terms, 8 per Put: a term is ~32 one-posting lists - 96 lists in all,
        beyond the one-launch form's II2_MAX_LISTS), with andnot.small 2 (the one-launch form up to its capacity) and 0;
  s120  the same over 120 Put segments (~19 lists a term: fits the one-launch form), with andnot.small 2 and 0;
  sp    a query at the one-launch form's capacity: 64 lists of 125 postings (8000 in all), 3 required groups and 1 excluded group of
        16 lists each, with andnot.small 2 and 0;
  a     C2's lists (100M docs): rank 2, cut by doc range over 4 segments, NOT rank 3, cut the same way;
  c     the rank-2 term of a C3-scale segment NOT its lists 1000 .. 20999 (20 000 lists);
  sweep (only when named) 4 - 64 lists of 512 - 8000 postings in all, 2 required groups and 1 excluded one: the one-launch form
        (andnot.small = 2: up to its capacity) against the general form - where the default limit comes from.
One JSON line: per case and variant the median, minimum and maximum of PROBE_N (default 15, at least 10) timed runs after 3 warm-up
runs, in microseconds.  Run parent and new library in alternating processes; under `rocprofv3 --kernel-trace --stats -- python
scripts/andnot_probe.py` (PROBE_VARIANTS=new) for the device time per kernel."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from functools import reduce

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="libii2_hip.so to load instead of the package's own")
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inverted_index_2_amd import _lib  # noqa: E402
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
    other = C.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.PROTOTYPES if not hasattr(other, n)]:      # a library from before an entry point (this probe's
        _lib.PROTOTYPES.pop(name)                                           # ii2_andnot_ranges among them: the yardstick only)
from inverted_index_2_amd import Context, synth  # noqa: E402

N = max(int(os.environ.get("PROBE_N", "15")), 10)
CASES = os.environ.get("PROBE_CASES", "s,s120,sp,a,c").split(",")
VARIANTS = os.environ.get("PROBE_VARIANTS", "yardstick,new").split(",")
have_new = "ii2_andnot_ranges" in _lib.PROTOTYPES


def stats(fn):
    for _ in range(3):
        fn()
    t = []
    for _ in range(N):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(float(np.median(t)), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def truth(required, excluded):
    sets = [np.unique(np.concatenate(g)) for g in required]
    return np.setdiff1d(reduce(np.intersect1d, sets), np.concatenate(excluded + [np.empty(0, np.uint32)])).astype(np.uint32)


def run_case(ctx, groups, exclude, want, cap_req, cap_ex, small_modes=(1,)):
    """groups / exclude as Context.andnot_ranges takes them; cap_req / cap_ex: ids the required / excluded side may give"""
    res = {"ids": int(want.size)}
    ex_ranges = [r for g in exclude for r in g]
    if "yardstick" in VARIANTS:
        d_req, d_ex = ctx.empty(cap_req + 1), ctx.empty(cap_ex + 1)
        got = [None]

        def old_route():
            _, n = ctx.intersect_ranges(groups, out=d_req)
            _, m = ctx.union_ranges(ex_ranges, out=d_ex)
            got[0] = np.setdiff1d(d_req.download(n), d_ex.download(m), assume_unique=True)
        r = stats(old_route)
        r["correct"] = bool(np.array_equal(got[0], want))
        res["yardstick"] = r
    if "new" in VARIANTS and have_new:
        d_out = ctx.empty(cap_req + 1)
        for small in small_modes:
            ctx.set_option("andnot.small", 2 if small else 0)       # (2: the one-launch form up to its capacity, whatever the default limit)
            got = [None]

            def new_route():
                _, n = ctx.andnot_ranges(groups, exclude, out=d_out)
                got[0] = d_out.download(n)
            r = stats(new_route)
            r["correct"] = bool(np.array_equal(got[0], want))
            res["new" if small else "new_small0"] = r
        ctx.set_option("andnot.small", 1)
    return res


def put_segments(ctx, rng, puts):
    """what `puts` Shard.Put calls of 8 of 50 terms leave behind: one segment per Put, one posting per term; term -> its ranges, ids"""
    where = {t: [] for t in range(50)}
    ids = {t: [] for t in range(50)}
    for v in range(puts):
        terms = np.sort(rng.choice(50, 8, replace=False))
        seg = ctx.encode_lists([np.asarray([v], np.uint32)] * 8)
        for j, t in enumerate(terms):
            where[int(t)].append((seg, j, j + 1))
            ids[int(t)].append(np.asarray([v], np.uint32))
    return where, ids


def case_puts(ctx, rng, res, name, puts):
    where, ids = put_segments(ctx, rng, puts)
    groups, exclude = [where[0], where[1]], [where[2]]
    want = truth([ids[0], ids[1]], ids[2])
    res[name] = run_case(ctx, groups, exclude, want, puts, puts, small_modes=(1, 0))
    res[name]["lists"] = sum(len(where[t]) for t in (0, 1, 2))


def case_sp(ctx, rng, res):
    lists = [np.unique(rng.integers(0, 4000, 400))[:125].astype(np.uint32) for _ in range(64)]
    lists = [l for l in lists if l.size == 125]
    assert len(lists) == 64
    segs = [ctx.encode_lists(lists[16 * s:16 * s + 16]) for s in range(4)]
    groups = [[(segs[g], 0, 16)] for g in range(3)]
    exclude = [[(segs[3], 0, 16)]]
    want = truth([lists[0:16], lists[16:32], lists[32:48]], lists[48:64])
    res["sp_capacity_64_lists_8000_postings"] = run_case(ctx, groups, exclude, want, 2000, 2000, small_modes=(1, 0))


def case_sweep(ctx, rng, res):
    """where the one-launch form stops paying: L lists of P / L postings each, 2 required groups and 1 excluded group (the general
    form's cheapest shape with an exclusion: three waits), the one-launch form up to its capacity (andnot.small = 2) against the
    general form (0)"""
    rows = []
    for L in (4, 8, 16, 32, 64):
        for P in (512, 1024, 2048, 4096, 8000):
            n = P // L
            lists = [np.sort(rng.choice(8 * P, n, replace=False)).astype(np.uint32) for _ in range(L)]
            seg = ctx.encode_lists(lists)
            a, b = 3 * L // 8, 6 * L // 8
            groups, exclude = [[(seg, 0, a)], [(seg, a, b)]], [[(seg, b, L)]]
            want = truth([lists[0:a], lists[a:b]], lists[b:L])
            d_out = ctx.empty(P + 1)
            row = {"lists": L, "postings": n * L, "ids": int(want.size)}
            for small in (2, 0):
                ctx.set_option("andnot.small", small)
                got = [None]

                def call():
                    _, k = ctx.andnot_ranges(groups, exclude, out=d_out)
                    got[0] = d_out.download(k)
                r = stats(call)
                row["one_launch" if small else "general"] = r
                row["correct"] = row.get("correct", True) and bool(np.array_equal(got[0], want))
            ctx.set_option("andnot.small", 1)
            rows.append(row)
    res["sweep_2_required_1_excluded"] = rows


def by_doc_range(l, k, D):
    cut = np.searchsorted(l, np.linspace(0, D, k + 1).astype(np.int64))
    return [l[cut[s]:cut[s + 1]] for s in range(k)]


def case_a(ctx, rng, res):
    D = 100_000_000
    a, b = synth.zipf_list(2, D), synth.zipf_list(3, D)
    segs = [ctx.encode_lists([pa, pb]) for pa, pb in zip(by_doc_range(a, 4, D), by_doc_range(b, 4, D))]
    groups, exclude = [[(s, 0, 1) for s in segs]], [[(s, 1, 2) for s in segs]]
    res["a_c2_rank2_not_rank3_4_segments"] = run_case(ctx, groups, exclude, np.setdiff1d(a, b), a.size, b.size)


def case_c(ctx, rng, res):
    T, D3 = 1_000_000, 100_000_000
    w = 1.0 / np.arange(1, T + 1)
    sizes = np.maximum(1, np.floor(w * (62.5 * T / w.sum()))).astype(np.int64)
    key = (np.repeat(np.arange(T, dtype=np.uint64), sizes) << np.uint64(32)) | rng.integers(0, D3, int(sizes.sum())).astype(np.uint64)
    key = np.unique(key)
    term = (key >> np.uint64(32)).astype(np.int64)
    vals = (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    off = np.zeros(T + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(term, minlength=T))
    seg3 = ctx.encode(off, vals)
    dense = vals[int(off[1]):int(off[2])]
    many = vals[int(off[1000]):int(off[21000])]
    want = np.setdiff1d(dense, many).astype(np.uint32)
    res["c_rank2_not_20000_lists"] = run_case(ctx, [[(seg3, 1, 2)]], [[(seg3, 1000, 21000)]], want, dense.size, many.size)


def main():
    ctx = Context(0)
    rng = np.random.default_rng(1)
    res = {"lib": args.lib or "package", "has_andnot": have_new, "runs": N}
    for name, fn in (("s", lambda *a: case_puts(*a, "s_200_put_segments", 200)), ("s120", lambda *a: case_puts(*a, "s120_120_put_segments", 120)),
                     ("sp", case_sp), ("a", case_a), ("c", case_c), ("sweep", case_sweep)):
        if name in CASES:
            fn(ctx, rng, res)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
