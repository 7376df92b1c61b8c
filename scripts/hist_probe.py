"""ii2_histogram_ranges against what a caller had to do without it, wall clock around synchronous calls, every case checked against
numpy at the size it is timed.  count_probe.py's workload: PROBE_TERMS (default 2000) Zipf lists over PROBE_DOCS (default 10 M)
docs, filter sets of 10^3, 10^5 and 10^7 ids on the device; B = 1, 24, 256 and 4096 uniform buckets over the docs.  Per (set, B):
  hist_whole1 / hist_whole0   ii2_histogram_ranges with hist.whole 1 (default) and 0, with n_whole / n_split / n_wide of each;
  count (B = 1)               ii2_count_ranges on the same arguments: the same walk, code this call does not touch;
  slices (B <= 256)           the route there was: B ii2_count_ranges calls, each against the slice of the device set inside one
                              bucket - the slice bounds from a host copy by np.searchsorted, outside the timed region.
The forms of one (set, B) are timed alternately, round by round, after 3 warm-up rounds: the median, minimum and maximum of PROBE_N
(default 15) rounds in microseconds - min to max of the count is the run-to-run spread the B = 1 histogram is held against.  The
driver (no argument) runs every set size in a child process of its own under a timeout, stops at the first that does not end
cleanly, prints ONE JSON line and appends it to profiles/hist_probe.jsonl."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from count_probe import DOCS, TERMS, filter_set, zipf_segment  # noqa: E402

N = max(int(os.environ.get("PROBE_N", "15")), 5)
CASES = ["set_1e3", "set_1e5", "set_1e7"]
BUCKETS = [1, 24, 256, 4096]
CASE_TIMEOUT = int(os.environ.get("PROBE_CASE_TIMEOUT", "300"))


def alternate(forms):
    """{name: fn} timed round by round: every round runs each form once"""
    for _ in range(3):
        for fn in forms.values():
            fn()
    t = {k: [] for k in forms}
    for _ in range(N):
        for k, fn in forms.items():
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e6)
    return {k: {"median_us": round(float(np.median(v)), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in t.items()}


def run_case(name):
    from inverted_index_2_amd import Context, _lib
    n_set = int(float(name.rsplit("_", 1)[1]))
    rng = np.random.default_rng(7)
    ctx = Context(0)
    off, vals = zipf_segment(rng)
    n_lists = off.size - 1
    seg = ctx.encode(off, vals)
    ids = filter_set(rng, n_set)
    d_set = ctx.empty(ids.size).upload(ids)
    member = np.zeros(DOCS, bool)
    member[ids] = True
    hit = member[vals]
    list_of = np.repeat(np.arange(n_lists, dtype=np.int64), np.diff(off).astype(np.int64))[hit]
    hit_vals = vals[hit].astype(np.int64)
    res = {"lists": n_lists, "postings": int(vals.size), "set_ids": int(ids.size), "hits": int(hit.sum()), "rounds": N}
    segs = (C.c_void_p * 1)(seg.h)
    first, end = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(n_lists)
    for B in BUCKETS:
        edges = np.asarray([DOCS * b // B for b in range(B + 1)], np.uint64)
        want = np.bincount(list_of * B + (np.searchsorted(edges[:-1].astype(np.int64), hit_vals, "right") - 1), minlength=n_lists * B).reshape(n_lists, B)
        counts = np.zeros((n_lists, B), np.uint64)
        st = _lib.HistStats()

        def run_hist(whole):
            ctx.set_option("hist.whole", whole)
            ctx._ck(ctx.lib.ii2_histogram_ranges(ctx.h, 1, segs, first, end, d_set.data_ptr(), ids.size, None, B, edges.ctypes.data_as(_lib.u64p),
                                                 counts.ctypes.data_as(_lib.u64p), counts.size, C.byref(st)))
        forms, checks = {}, {}
        for whole in (1, 0):
            run_hist(whole)
            checks["hist_whole%d" % whole] = dict(correct=bool(np.array_equal(counts, want)), n_whole=int(st.n_whole), n_split=int(st.n_split),
                                                  n_wide=int(st.n_wide), n_blocks=int(st.n_blocks), n_windows=int(st.n_windows))
            forms["hist_whole%d" % whole] = lambda whole=whole: run_hist(whole)
        if B == 1:
            one = np.zeros(n_lists, np.uint64)
            cst = _lib.CountStats()

            def run_count():
                ctx._ck(ctx.lib.ii2_count_ranges(ctx.h, 1, segs, first, end, d_set.data_ptr(), ids.size, None, one.ctypes.data_as(_lib.u64p), n_lists,
                                                 C.byref(cst)))
            run_count()
            checks["count"] = dict(correct=bool(np.array_equal(one, want[:, 0])), n_decoded=int(cst.n_decoded))
            forms["count"] = run_count
        if B <= 256:
            cut = np.searchsorted(ids, edges.astype(np.int64)).astype(np.int64)          # the slices of the set, from a host copy
            rows = np.zeros((B, n_lists), np.uint64)

            def run_slices():
                for b in range(B):
                    ctx._ck(ctx.lib.ii2_count_ranges(ctx.h, 1, segs, first, end, d_set.data_ptr() + 4 * int(cut[b]), int(cut[b + 1] - cut[b]), None,
                                                     rows[b].ctypes.data_as(_lib.u64p), n_lists, None))
            run_slices()
            checks["slices"] = dict(correct=bool(np.array_equal(rows.T, want)))
            forms["slices"] = run_slices
        r = alternate(forms)
        for k in r:
            r[k].update(checks[k])
        res["B%d" % B] = r
    ctx.set_option("hist.whole", 1)
    ctx.close()
    return res


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--case":
        print(json.dumps(run_case(sys.argv[2])))
        return 0
    out = {"terms": TERMS, "docs": DOCS}
    for name in [c for c in os.environ.get("PROBE_CASES", ",".join(CASES)).split(",") if c]:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], capture_output=True, text=True, timeout=CASE_TIMEOUT)
        except subprocess.TimeoutExpired:
            out[name] = {"error": "timeout after %d s" % CASE_TIMEOUT}
            break                               # nothing more is started on the GPU after a case that did not end
        if p.returncode != 0:
            out[name] = {"error": "exit status %d" % p.returncode, "stderr": p.stderr[-2000:]}
            break
        out[name] = json.loads(p.stdout.strip().splitlines()[-1])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", os.environ.get("PROBE_OUT", "hist_probe.jsonl")), "a") as f:
        f.write(line + "\n")
    return 0 if all("error" not in v for v in out.values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
