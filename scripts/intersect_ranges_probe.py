"""ii2_intersect_ranges timings (device time from HIP events on the context stream, cold = first call, warm = mean of the next N),
every case checked against numpy at the size it is timed:
  (a) C2's two lists (100M docs, ranks 2 and 3), each cut by doc range over 4 segments, next to ii2_intersect on the uncut
      lists (the floor) and to merge_to_segment + ii2_intersect (what a caller had to do before);
  (b) C5's eight lists (ranks 2 ... 16384 with a 10 000-id common core; PROBE_C5_DOCS docs, default 100M = a tenth of C5) each
      spread over 4 segments at random, next to ii2_intersect on the uncut lists;
  (c) 20 000 lists of a C3-scale segment (ranks 1001-21000, the union probe's case (b)) ANDed with its rank-2 term;
  (d) the host mirror's Intersect of 2 terms, wall clock, over 200 Put segments and over a merged index of 2 x 10k C1 documents
      put one by one, next to the route it replaces rebuilt from public calls: read(t, t) per term, then intersect_host.
Each of (a) - (c) runs with the filter choice of option intersect.ranges_mark forced both ways as well.
Run plain for the times and under `rocprofv3 --kernel-trace --stats -- python scripts/intersect_ranges_probe.py` for per-kernel time;
PROBE_CASES=a,b,c,d (default: all) runs only the cases named, PROBE_MODES=default,probe,mark only those filter choices (a trace
of one case in one mode gives that path's kernels alone)."""
import json
import os
import sys
import time
from functools import reduce

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inverted_index_2_amd import Context, synth  # noqa: E402

N = int(os.environ.get("PROBE_N", "10"))
CASES = os.environ.get("PROBE_CASES", "a,b,c,d").split(",")
MODES = os.environ.get("PROBE_MODES", "default,probe,mark").split(",")
ALWAYS_MARK = 1 << 40


def timed(ctx, fn):
    ctx.profile_region(True)
    fn()
    ctx.profile_region(False)
    cold = ctx.profile_region_ms() * 1e3
    ctx.profile_region(True)
    for _ in range(N):
        fn()
    ctx.profile_region(False)
    return {"cold_us": round(cold, 1), "warm_us": round(ctx.profile_region_ms() * 1e3 / N, 1)}


def ranges_case(ctx, groups, want, out):
    """the call with the default filter choice, forced probe and forced mark: times + correctness"""
    res = {}
    for name, mark in (("default", None), ("probe", 0), ("mark", ALWAYS_MARK)):
        if name not in MODES:
            continue
        if mark is not None:
            ctx.set_option("intersect.ranges_mark", mark)
        cnt = [0]

        def call():
            cnt[0] = ctx.intersect_ranges(groups, out=out)[1]
        r = timed(ctx, call)
        r["correct"] = bool(cnt[0] == want.size and np.array_equal(out.download(cnt[0]), want))
        res[name] = r
        ctx.set_option("intersect.ranges_mark", 64)
    res["ids"] = int(want.size)
    return res


def by_doc_range(l, k, D):
    cut = np.searchsorted(l, np.linspace(0, D, k + 1).astype(np.int64))
    return [l[cut[s]:cut[s + 1]] for s in range(k)]


def at_random(rng, l, k):
    home = rng.integers(0, k, l.size)
    return [l[home == s] for s in range(k)]


def case_a(ctx, rng, res):
    # (a) C2, each list cut by doc range over 4 segments
    D = 100_000_000
    a, b = synth.zipf_list(2, D), synth.zipf_list(3, D)
    want = np.intersect1d(a, b)
    whole = ctx.encode_lists([a, b])
    out = ctx.empty(b.size + 1)
    cnt = [0]

    def floor():
        cnt[0] = ctx.intersect([(whole, 0), (whole, 1)], out=out)[1]
    res["a_floor_intersect"] = timed(ctx, floor)
    segs = [ctx.encode_lists([pa, pb]) for pa, pb in zip(by_doc_range(a, 4, D), by_doc_range(b, 4, D))]
    groups = [[(s, t, t + 1) for s in segs] for t in (0, 1)]
    res["a_c2_4_segments"] = ranges_case(ctx, groups, want, out)

    def merge_then_and():
        m, _ = ctx.merge_to_segment(segs)
        cnt[0] = ctx.intersect([(m, 0), (m, 1)], out=out)[1]
        m.free()
    res["a_merge_then_intersect"] = timed(ctx, merge_then_and)


def case_b(ctx, rng, res):
    # (b) C5's shape: 8 lists with a common core, each spread over 4 segments at random
    D5 = int(os.environ.get("PROBE_C5_DOCS", "100000000"))
    core = np.unique(np.random.default_rng(55).integers(0, D5, 10_000)).astype(np.uint32)
    lists = [np.union1d(synth.zipf_list(r, D5), core).astype(np.uint32) for r in (2, 4, 16, 64, 256, 1024, 4096, 16384)]
    want5 = reduce(np.intersect1d, lists)
    whole5 = ctx.encode_lists(lists)
    out5 = ctx.empty(lists[-1].size + 1)
    cnt = [0]

    def floor5():
        cnt[0] = ctx.intersect([(whole5, i) for i in range(8)], out=out5)[1]
    res["b_floor_intersect"] = timed(ctx, floor5)
    parts = [at_random(rng, l, 4) for l in lists]
    segs5 = [ctx.encode_lists([parts[t][s] for t in range(8)]) for s in range(4)]
    groups5 = [[(s, t, t + 1) for s in segs5] for t in range(8)]
    res["b_c5_4_segments"] = ranges_case(ctx, groups5, want5, out5)

    def merge_then_and5():
        m, _ = ctx.merge_to_segment(segs5)
        cnt[0] = ctx.intersect([(m, i) for i in range(8)], out=out5)[1]
        m.free()
    res["b_merge_then_intersect"] = timed(ctx, merge_then_and5)


def case_c(ctx, rng, res):
    # (c) a C3-scale segment: 20 000 lists ANDed with the rank-2 term
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
    want3 = np.intersect1d(np.unique(vals[int(off[1000]):int(off[21000])]), vals[int(off[1]):int(off[2])])
    out3 = ctx.empty(int(off[2] - off[1]) + 1)
    res["c_20000_lists_and_rank2"] = ranges_case(ctx, [[(seg3, 1000, 21000)], [(seg3, 1, 2)]], want3, out3)


def case_d(ctx, rng, res):
    # (d) the host mirror
    res["d_200_put_segments"] = host_case(ctx, rng, puts=200)
    res["d_c1_merged_2x10k"] = host_case(ctx, rng, c1=True)


def main():
    ctx = Context(0)
    rng = np.random.default_rng(1)
    res = {}
    for name, fn in (("a", case_a), ("b", case_b), ("c", case_c), ("d", case_d)):
        if name in CASES:
            fn(ctx, rng, res)
    ctx.close()
    print(json.dumps(res))


def host_case(ctx, rng, puts=0, c1=False):
    from inverted_index_2_amd.host import InvertedIndex
    ii = InvertedIndex(ctx)
    if c1:
        rank, doc = synth.c1_workload(1_000_000, 10_000, 2)
        names = synth.random_terms(1_000_000)
        order = np.argsort(doc, kind="stable")
        rank, doc = rank[order], doc[order]
        cut = np.flatnonzero(np.diff(doc)) + 1
        for r, d in zip(np.split(rank, cut), doc[np.r_[0, cut]]):
            ii.put([names[x] for x in r], int(d))
        while ii.merge(2, 100, 1):
            pass
        t1, t2 = names[0], names[1]
    else:
        vocab = [b"t%03d" % i for i in range(50)]
        for v in range(puts):
            ii.put([vocab[i] for i in rng.choice(50, 8, replace=False)], v)
        t1, t2 = vocab[0], vocab[1]

    def old_route():
        return ctx.intersect_host([dict(ii.read(t, t)).get(t, []) for t in (t1, t2)])
    want = old_route()
    got = ii.intersect([t1, t2])
    r = {"correct": bool(list(map(int, want)) == got), "ids": len(got)}
    for name, fn in (("intersect_wall_us", lambda: ii.intersect([t1, t2])), ("read_then_intersect_host_wall_us", old_route)):
        fn()
        t0 = time.perf_counter()
        for _ in range(N):
            fn()
        r[name] = round((time.perf_counter() - t0) / N * 1e6, 1)
    ii.close()
    return r


if __name__ == "__main__":
    main()
