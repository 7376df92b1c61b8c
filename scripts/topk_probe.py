"""ii2_topk_ranges ("the k docs in the most groups, with their scores") against what a caller had to do without it, wall clock with
the results left on the device unless stated, every case checked against numpy at the size it is timed.  Every case runs in a child
process of its own under a time limit (the parent never opens the GPU and stops at the first child that fails); --lib points at
another build - the parent commit's, for the yardsticks:
  loop   what a caller does without the entry point for the same ids: ii2_atleast_ranges with min_match = n', n' - 1, ... until at
         least k ids have come back; every round that brought new ids is downloaded and the ids new in it (they have score
         min_match exactly) are appended smallest first: the cut on the host.  Every library that has ii2_atleast_ranges can run it;
  floor  one counting-form ii2_atleast_ranges at min_match = 1 (atleast.handoff 0, atleast.small 0), no download: the same marks
         and adds, then a select and a compaction instead of the two passes;
  topk   one ii2_topk_ranges (skipped when the library lacks the entry point), no download; "topk_dl" adds the download of the k
         (id, score) pairs.  With option profile.events the device time of k_top_hist (a k = 0 call, which runs pass 1 alone and
         cleans up in it) and of k_top_hist + k_top_emit (first window each).
Cases (PROBE_CASES=a,b; default both):
  a  8 groups of one Zipf list each (ranks 2 .. 9) over 10 M docs, k = 10, 1000, 100 000 (PROBE_A_KS names others);
  b  3 terms spread over 200 Put segments (50 terms, 8 per Put: a term is ~32 one-posting lists), k = 100.
One JSON line per case: per variant the median, minimum and maximum of PROBE_N (default 20, at least 20) timed runs after 3 warm-up
runs, in microseconds."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="libii2_hip.so to load instead of the package's own")
ap.add_argument("--case", default=None, help="run this one case in this process (what the parent starts)")
ap.add_argument("--timeout", type=int, default=240, help="seconds a case may take")
args = ap.parse_args()

N = max(int(os.environ.get("PROBE_N", "20")), 20)
CASES = os.environ.get("PROBE_CASES", "a,b").split(",")
A_KS = [int(k) for k in os.environ.get("PROBE_A_KS", "10,1000,100000").split(",")]
VARIANTS = os.environ.get("PROBE_VARIANTS", "loop,floor,topk,topk_dl,device").split(",")
COUNTING = {"atleast.handoff": 0, "atleast.small": 0}


def stats(fn):
    for _ in range(3):
        fn()
    t = []
    for _ in range(N):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(float(np.median(t)), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def truth(groups_ids, k):
    ids, cnt = np.unique(np.concatenate([np.unique(np.concatenate(g)) for g in groups_ids]), return_counts=True)
    order = np.lexsort((ids, -cnt))[:k]
    return ids[order].astype(np.uint32), cnt[order].astype(np.uint32)


def run_case(ctx, have_new, groups, groups_ids, ks, cap):
    """groups as Context.topk_ranges takes them, groups_ids their lists' ids; cap: ids a union of all of them may give"""
    n = len(groups)
    d_out = ctx.empty(cap + 1)
    res = {}
    if "floor" in VARIANTS:
        for key, v in COUNTING.items():
            ctx.set_option(key, v)
        form = [None]

        def floor_route():
            _, _, form[0] = ctx.atleast_ranges(groups, 1, out=d_out, stats=True)
        r = stats(floor_route)
        r.update(form=int(form[0].form), planes=int(form[0].n_planes), windows=int(form[0].n_windows))
        res["floor"] = r
        for key in COUNTING:
            ctx.set_option(key, 1)
    for k in ks:
        want_ids, want_scores = truth(groups_ids, k)
        row = {"ids": int(want_ids.size)}
        if "loop" in VARIANTS:
            got, rounds = [None], [0]

            def loop_route():
                m, have = n, np.empty(0, np.uint32)
                while True:
                    _, cnt = ctx.atleast_ranges(groups, m, out=d_out)
                    if cnt > have.size:                    # the rounds nest: the ids new in this one have score m exactly
                        ids = d_out.download(cnt)
                        have = np.concatenate([have, np.setdiff1d(ids, have, assume_unique=True)])
                    if have.size >= k or m == 1:
                        break
                    m -= 1
                rounds[0] = n - m + 1
                got[0] = have[:k]
            r = stats(loop_route)
            r.update(rounds=rounds[0], correct=bool(np.array_equal(got[0], want_ids)))
            row["loop"] = r
        if have_new:
            d_ids, d_scores = ctx.empty(max(k, 1)), ctx.empty(max(k, 1))
            got = [None]

            def new_route():
                got[0] = ctx.topk_ranges(groups, k, stats=True, out=(d_ids, d_scores))

            def new_route_dl():
                got[0] = ctx.topk_ranges(groups, k, stats=True, out=(d_ids, d_scores))
                got[0] = got[0] + (d_ids.download(got[0][2]), d_scores.download(got[0][2]))
            if "topk" in VARIANTS:
                r = stats(new_route)
                _, _, cnt, hist, st = got[0][:5]
                r.update(correct=bool(np.array_equal(d_ids.download(cnt), want_ids) and np.array_equal(d_scores.download(cnt), want_scores)),
                         planes=int(st.n_planes), windows=int(st.n_windows), marks=int(st.n_marks), eligible=int(st.n_eligible),
                         cut_score=int(st.cut_score), n_cut=int(st.n_cut), max_score=int(st.max_score))
                row["topk"] = r
            if "topk_dl" in VARIANTS:
                row["topk_dl"] = stats(new_route_dl)
            if "device" in VARIANTS:
                ctx.set_option("profile.events", 1)
                ctx.profile_read()
                for _ in range(N):
                    ctx.topk_ranges(groups, 0)
                ms, launches = ctx.profile_read()
                row["k_top_hist_us"] = round(ms * 1e3 / max(launches, 1), 1)
                for _ in range(N):
                    new_route()
                ms, launches = ctx.profile_read()
                row["k_top_hist_plus_emit_us"] = round(ms * 1e3 / max(launches // 2, 1), 1)
                ctx.set_option("profile.events", 0)
        res[f"k{k}"] = row
    return res


def case_a(ctx, rng, have_new, synth):
    D = 10_000_000
    lists = [synth.zipf_list(r, D) for r in range(2, 10)]
    seg = ctx.encode_lists(lists)
    return run_case(ctx, have_new, [[(seg, j, j + 1)] for j in range(8)], [[l] for l in lists], A_KS, sum(l.size for l in lists))


def case_b(ctx, rng, have_new, synth):
    where = {t: [] for t in range(50)}
    ids = {t: [] for t in range(50)}
    for v in range(200):
        terms = np.sort(rng.choice(50, 8, replace=False))
        seg = ctx.encode_lists([np.asarray([v], np.uint32)] * 8)
        for j, t in enumerate(terms):
            where[int(t)].append((seg, j, j + 1))
            ids[int(t)].append(np.asarray([v], np.uint32))
    res = run_case(ctx, have_new, [where[0], where[1], where[2]], [ids[0], ids[1], ids[2]], [100], 200)
    res["lists"] = sum(len(where[t]) for t in (0, 1, 2))
    return res


def child(name):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from inverted_index_2_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
        other = C.CDLL(_lib.LIB_PATH)
        for sym in [s for s in _lib.PROTOTYPES if not hasattr(other, s)]:        # a library from before an entry point: the yardsticks only
            _lib.PROTOTYPES.pop(sym)
    from inverted_index_2_amd import Context, synth
    have_new = "ii2_topk_ranges" in _lib.PROTOTYPES
    ctx = Context(0)
    res = {"case": name, "lib": args.lib or "package", "has_topk": have_new, "runs": N}
    res.update({"a": case_a, "b": case_b}[name](ctx, np.random.default_rng(1), have_new, synth))
    ctx.close()
    print(json.dumps(res), flush=True)


def main():
    if args.case:
        return child(args.case)
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name] + (["--lib", args.lib] if args.lib else [])
        rc = subprocess.run(cmd, timeout=args.timeout).returncode
        if rc:
            sys.exit(f"case {name} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
