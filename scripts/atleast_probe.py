"""ii2_atleast_ranges ("docs in at least m of n groups") against what a caller had to do without it, wall clock, every case checked
against numpy at the size it is timed.  Every case runs in a child process of its own under a time limit (the parent never opens
the GPU and stops at the first child that fails); --lib points at another build - the parent commit's, for the yardsticks:
  yardstick  m = n: ii2_intersect_ranges;  m = 1: ii2_union_ranges;  1 < m < n: n ii2_union_ranges calls, n downloads and a numpy
             count - every library that has the range entry points can run it;
  new        one ii2_atleast_ranges + one download (skipped when the library lacks the entry point), as the default options choose
             ("new"), with the hand-offs off ("no_handoff"), with the one-launch form up to its capacity ("small2") and with
             neither ("count": the counting form).
Cases (PROBE_CASES=a,b,c; default all):
  a  8 groups of one Zipf list each (ranks 2 .. 9) over 10 M docs, m = 1 .. 8 (PROBE_A_MS=1,4,8 names the thresholds to run);
  b  3 terms spread over 200 Put segments (50 terms, 8 per Put: a term is ~32 one-posting lists), m = 2;
  c  64 groups of 300 short lists (2 postings each) over 1 M docs, m = 32 - the lists drawn from 3000 ids, so that docs reach m.
One JSON line per case: per variant the median, minimum and maximum of PROBE_N (default 15, at least 10) timed runs after 3 warm-up
runs, in microseconds, and the form that ran.  Under `rocprofv3 --kernel-trace --stats -- python scripts/atleast_probe.py --case a`
(PROBE_VARIANTS=count) for the device time per kernel."""
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

N = max(int(os.environ.get("PROBE_N", "15")), 10)
CASES = os.environ.get("PROBE_CASES", "a,b,c").split(",")
A_MS = [int(m) for m in os.environ.get("PROBE_A_MS", "1,2,3,4,5,6,7,8").split(",")]
VARIANTS = os.environ.get("PROBE_VARIANTS", "yardstick,new,no_handoff,small2,count").split(",")
MODES = {"new": {}, "no_handoff": {"atleast.handoff": 0}, "small2": {"atleast.handoff": 0, "atleast.small": 2},
         "count": {"atleast.handoff": 0, "atleast.small": 0}}
FORMS = ["none", "small", "count", "and", "or"]


def stats(fn):
    for _ in range(3):
        fn()
    t = []
    for _ in range(N):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(float(np.median(t)), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def truth(groups_ids, m):
    ids, cnt = np.unique(np.concatenate([np.unique(np.concatenate(g)) for g in groups_ids]), return_counts=True)
    return ids[cnt >= m].astype(np.uint32)


def run_case(ctx, have_new, groups, groups_ids, ms, cap):
    """groups as Context.atleast_ranges takes them, groups_ids their lists' ids; cap: ids a union of all of them may give"""
    n = len(groups)
    d_out = ctx.empty(cap + 1)
    res = {}
    for m in ms:
        want = truth(groups_ids, m)
        row = {"ids": int(want.size)}
        if "yardstick" in VARIANTS:
            got = [None]

            def old_route():
                if m == n:
                    _, k = ctx.intersect_ranges(groups, out=d_out)
                    got[0] = d_out.download(k)
                elif m == 1:
                    _, k = ctx.union_ranges([r for g in groups for r in g], out=d_out)
                    got[0] = d_out.download(k)
                else:
                    parts = []
                    for g in groups:
                        _, k = ctx.union_ranges(g, out=d_out)
                        parts.append(d_out.download(k))
                    ids, cnt = np.unique(np.concatenate(parts), return_counts=True)
                    got[0] = ids[cnt >= m]
            r = stats(old_route)
            r["correct"] = bool(np.array_equal(got[0], want))
            row["yardstick"] = r
        for name, opts in MODES.items():
            if name not in VARIANTS or not have_new:
                continue
            for k, v in opts.items():
                ctx.set_option(k, v)
            got, form = [None], [0]

            def new_route():
                _, k, st = ctx.atleast_ranges(groups, m, out=d_out, stats=True)
                got[0], form[0] = d_out.download(k), st
            r = stats(new_route)
            st = form[0]
            r.update(correct=bool(np.array_equal(got[0], want)), form=FORMS[st.form], planes=st.n_planes, windows=st.n_windows, late=st.n_late)
            row[name] = r
            for k in opts:
                ctx.set_option(k, 1)
        res[f"m{m}"] = row
    return res


def case_a(ctx, rng, have_new, synth):
    D = 10_000_000
    lists = [synth.zipf_list(r, D) for r in range(2, 10)]
    seg = ctx.encode_lists(lists)
    return run_case(ctx, have_new, [[(seg, j, j + 1)] for j in range(8)], [[l] for l in lists], A_MS, sum(l.size for l in lists))


def case_b(ctx, rng, have_new, synth):
    where = {t: [] for t in range(50)}
    ids = {t: [] for t in range(50)}
    for v in range(200):
        terms = np.sort(rng.choice(50, 8, replace=False))
        seg = ctx.encode_lists([np.asarray([v], np.uint32)] * 8)
        for j, t in enumerate(terms):
            where[int(t)].append((seg, j, j + 1))
            ids[int(t)].append(np.asarray([v], np.uint32))
    res = run_case(ctx, have_new, [where[0], where[1], where[2]], [ids[0], ids[1], ids[2]], [2], 200)
    res["lists"] = sum(len(where[t]) for t in (0, 1, 2))
    return res


def case_c(ctx, rng, have_new, synth):
    pool = np.sort(rng.choice(1_000_000, 3000, replace=False)).astype(np.uint32)
    groups, groups_ids = [], []
    for g in range(64):
        lists = [np.sort(rng.choice(pool, 2, replace=False)).astype(np.uint32) for _ in range(300)]
        seg = ctx.encode_lists(lists)
        groups.append([(seg, 0, 300)])
        groups_ids.append(lists)
    return run_case(ctx, have_new, groups, groups_ids, [32], 64 * 600)


def child(name):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from inverted_index_2_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
        other = C.CDLL(_lib.LIB_PATH)
        for sym in [s for s in _lib.PROTOTYPES if not hasattr(other, sym)]:        # a library from before an entry point: the yardstick only
            _lib.PROTOTYPES.pop(sym)
    from inverted_index_2_amd import Context, synth
    have_new = "ii2_atleast_ranges" in _lib.PROTOTYPES
    ctx = Context(0)
    res = {"case": name, "lib": args.lib or "package", "has_atleast": have_new, "runs": N}
    res.update({"a": case_a, "b": case_b, "c": case_c}[name](ctx, np.random.default_rng(1), have_new, synth))
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
