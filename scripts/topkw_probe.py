"""ii2_topk_weighted_ranges ("the k docs of the highest weighted score") measured three ways, results left on the device, every
variant checked against numpy at the size it is timed.  Every case runs in a child process of its own under a time limit (the parent
never opens the GPU and stops at the first child that fails).  Within a case the variants alternate call by call, so that they
share whatever else the machine is doing; per variant the median, minimum and maximum over PROBE_N (default 20, at least 20)
rounds after 3 warm-up rounds, of the wall clock around the call (which ends in a wait for the stream) and of the device time
between two events around it (ii2_profile_region), in microseconds.
Cases (PROBE_CASES=a,b,c; default all):
  a  the cost of the weighted add: topk_probe.py's shape a - 8 groups of one Zipf list each (ranks 2 .. 9) over 10 M docs, k = 10,
     1000, 100 000 - as ii2_topk_ranges ("topk": the parent commit's code path, unchanged) and as the weighted call with all-one
     weights ("w1": same planes, same bytes, the other add kernel).  "band": whether w1's median lies inside topk's min .. max.
  b  the plane-skipping saving, on the same shape at k = 1000: all weights 8 ("w8": W' = 64, 7 planes, every add touches planes
     3 .. 6) against 7 x 9 + 1 ("w9": the same W' and planes, every add touches all 7) and against all ones ("w1": 4 planes).
  c  the late-mode saving: a stop-word of 10^7 postings (every tenth doc of 10^8) with weight 1 and three rare terms of 10^4
     uniform postings each with weights 6, 9 and 5, min_score 2, k = 1000, with option topk.late 1 and 0.  "early_chunks": the share
     of the 2048-doc chunks that hold a doc of a rare term - what a late add still has to touch.
One JSON line per case."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--case", default=None, help="run this one case in this process (what the parent starts)")
ap.add_argument("--timeout", type=int, default=300, help="seconds a case may take")
args = ap.parse_args()

N = max(int(os.environ.get("PROBE_N", "20")), 20)
CASES = os.environ.get("PROBE_CASES", "a,b,c").split(",")
A_KS = [int(k) for k in os.environ.get("PROBE_A_KS", "10,1000,100000").split(",")]


def summary(t):
    return {"median_us": round(float(np.median(t)), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def alternate(ctx, variants):
    """variants: {name: fn}; every round calls each once, in turn.  {name: {"wall": ..., "device": ...}}"""
    wall, dev = {v: [] for v in variants}, {v: [] for v in variants}
    for r in range(3 + N):
        for name, fn in variants.items():
            ctx.profile_region(True)
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            ctx.profile_region(False)
            if r >= 3:
                wall[name].append((t1 - t0) * 1e6)
                dev[name].append(ctx.profile_region_ms() * 1e3)
    return {v: {"wall": summary(wall[v]), "device": summary(dev[v])} for v in variants}


def truth(lists, weights, k, min_score=1):
    ids = np.unique(np.concatenate(lists))
    score = np.zeros(ids.size, np.int64)
    for l, w in zip(lists, weights):
        score[np.searchsorted(ids, l)] += w                     # (a list holds an id once)
    keep = score >= min_score
    ids, score = ids[keep], score[keep]
    order = np.lexsort((ids, -score))[:k]
    return ids[order].astype(np.uint32), score[order].astype(np.uint32)


def weighted(ctx, groups, lists, weights, k, min_score, out):
    """a timed variant and its check: fn() runs the call; after the rounds check() compares what the last call left with numpy"""
    got = [None]

    def fn():
        got[0] = ctx.topk_weighted_ranges(groups, weights, k, min_score, stats=True, out=out)

    def check():
        _, _, cnt, _, st = got[0]
        want_ids, want_scores = truth(lists, weights, k, min_score)
        ok = bool(cnt == want_ids.size and np.array_equal(out[0].download(cnt), want_ids) and np.array_equal(out[1].download(cnt), want_scores))
        return {"correct": ok, "total_weight": int(st.total_weight), "planes": int(st.n_planes), "windows": int(st.n_windows), "marks": int(st.n_marks),
                "late": int(st.n_late), "eligible": int(st.n_eligible), "cut_score": int(st.cut_score), "max_score": int(st.max_score)}
    return fn, check


def zipf_groups(ctx, synth):
    lists = [synth.zipf_list(r, 10_000_000) for r in range(2, 10)]
    seg = ctx.encode_lists(lists)
    return [[(seg, j, j + 1)] for j in range(8)], lists


def case_a(ctx, synth):
    groups, lists = zipf_groups(ctx, synth)
    res = {}
    for k in A_KS:
        out_t, out_w = (ctx.empty(k), ctx.empty(k)), (ctx.empty(k), ctx.empty(k))
        got = [None]

        def topk():
            got[0] = ctx.topk_ranges(groups, k, stats=True, out=out_t)
        w1, check = weighted(ctx, groups, lists, [1] * 8, k, 1, out_w)
        row = alternate(ctx, {"topk": topk, "w1": w1})
        want_ids, want_scores = truth(lists, [1] * 8, k)
        cnt = got[0][2]
        row["topk"]["correct"] = bool(np.array_equal(out_t[0].download(cnt), want_ids) and np.array_equal(out_t[1].download(cnt), want_scores))
        row["w1"].update(check())
        for clock in ("wall", "device"):
            row[f"band_{clock}"] = bool(row["topk"][clock]["min_us"] <= row["w1"][clock]["median_us"] <= row["topk"][clock]["max_us"])
        res[f"k{k}"] = row
    return res


def case_b(ctx, synth):
    groups, lists = zipf_groups(ctx, synth)
    k = 1000
    vectors = {"w8": [8] * 8, "w9": [9] * 7 + [1], "w1": [1] * 8}
    fns, checks = {}, {}
    for name, w in vectors.items():
        fns[name], checks[name] = weighted(ctx, groups, lists, w, k, 1, (ctx.empty(k), ctx.empty(k)))
    res = alternate(ctx, fns)
    for name in vectors:
        res[name].update(checks[name]())
    return res


def case_c(ctx, synth):
    D = 100_000_000
    rng = np.random.default_rng(synth.GLOBAL_SEED)
    lists = [np.arange(0, D, 10, dtype=np.uint32)] + [np.unique(rng.integers(0, D, 10_000, dtype=np.int64)).astype(np.uint32) for _ in range(3)]
    weights, k, min_score = [1, 6, 9, 5], 1000, 2
    seg = ctx.encode_lists(lists)
    groups = [[(seg, j, j + 1)] for j in range(4)]
    fns, checks = {}, {}
    for late in (1, 0):
        fn, checks[f"late{late}"] = weighted(ctx, groups, lists, weights, k, min_score, (ctx.empty(k), ctx.empty(k)))

        def with_option(fn=fn, late=late):
            ctx.set_option("topk.late", late)
            fn()
        fns[f"late{late}"] = with_option
    res = alternate(ctx, fns)
    ctx.set_option("topk.late", 1)
    for name in fns:
        res[name].update(checks[name]())
    early = np.unique(np.concatenate(lists[1:]) // 2048).size
    res["early_chunks"] = round(early / np.unique(lists[0] // 2048).size, 3)
    res["postings"] = [int(l.size) for l in lists]
    return res


def child(name):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from inverted_index_2_amd import Context, synth
    ctx = Context(0)
    res = {"case": name, "runs": N}
    res.update({"a": case_a, "b": case_b, "c": case_c}[name](ctx, synth))
    ctx.close()
    print(json.dumps(res), flush=True)


def main():
    if args.case:
        return child(args.case)
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name]
        rc = subprocess.run(cmd, timeout=args.timeout).returncode
        if rc:
            sys.exit(f"case {name} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
