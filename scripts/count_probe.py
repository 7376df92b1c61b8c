"""ii2_count_ranges against what a caller had to do without it, wall clock around synchronous calls, every case checked against
numpy at the size it is timed.  A facet workload: PROBE_TERMS (default 2000) terms under one prefix - one run of consecutive lists
of a segment, Zipf lengths, the longest a fifth of the PROBE_DOCS (default 10 M) docs - counted against filter sets of 10^3, 10^5
and 10^7 ids (the last one: every doc).  The filter is the cheapest one there is, a single list holding the set.  Per set size:
  filter        one ii2_union_ranges of the filter list into the device array that ii2_count_ranges takes as d_set (what the new
                route pays once, on top of the count);
  count_skip1 / count_skip0   ii2_count_ranges with count.summary_skip 1 (default) and 0, and n_decoded / n_blocks of each;
  baseline      ii2_query_batch_groups with cap = 0 and d_out = NULL: one query per term - the filter's group plus the term's
                group - the sizes read from out_off under II2_ECAPACITY, in chunks of 2^20 queries.  Existing code on the same
                machine and commit: the yardstick.
One adversarial case: a single list that owns every block (PROBE_DOCS / 2 postings), so every wave of the count kernel adds to the
same counter.
The driver (no argument) runs every case in a child process of its own under a timeout and stops at the first one that does not
end cleanly; it prints ONE JSON line.  Timed: the median, minimum and maximum of PROBE_N (default 10) runs after 3 warm-up runs
(fewer runs, at least 3, of a call that takes seconds), in microseconds; the arrays of the calls are packed once, outside the timed region."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N = max(int(os.environ.get("PROBE_N", "10")), 5)
TERMS = int(os.environ.get("PROBE_TERMS", "2000"))
DOCS = int(os.environ.get("PROBE_DOCS", "10000000"))
CASES = ["set_1e3", "set_1e5", "set_1e7", "one_list_1e5", "one_list_1e7"]
CASE_TIMEOUT = int(os.environ.get("PROBE_CASE_TIMEOUT", "240"))


def stats(fn):
    t0 = time.perf_counter()
    fn()
    first = time.perf_counter() - t0
    runs = min(N, max(3, int(20.0 / max(first, 1e-6))))      # a call of seconds (the yardstick on a large set) is timed fewer times
    for _ in range(2):
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(float(np.median(t)), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1), "runs": runs}


def zipf_segment(rng):
    """TERMS lists of Zipf lengths over DOCS docs as (offsets u64 [TERMS + 1], values u32)"""
    sizes = np.maximum(1, (DOCS // 5) / np.arange(1, TERMS + 1)).astype(np.int64)
    key = (np.repeat(np.arange(TERMS, dtype=np.uint64), sizes) << np.uint64(32)) | rng.integers(0, DOCS, int(sizes.sum())).astype(np.uint64)
    key = np.unique(key)
    term = (key >> np.uint64(32)).astype(np.int64)
    off = np.zeros(TERMS + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(term, minlength=TERMS))
    return off, (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def filter_set(rng, n):
    if n >= DOCS:
        return np.arange(DOCS, dtype=np.uint32)
    return np.unique(rng.integers(0, DOCS, n)).astype(np.uint32)


def run_case(name):
    from inverted_index_2_amd import Context, _lib
    from inverted_index_2_amd.engine import pack_group_batch
    kind, size = name.rsplit("_", 1)
    n_set = int(float(size))
    rng = np.random.default_rng(7)
    ctx = Context(0)
    if kind == "set":
        off, vals = zipf_segment(rng)
    else:                                       # one list that owns every block
        vals = np.flatnonzero(rng.random(DOCS) < 0.5).astype(np.uint32)
        off = np.asarray([0, vals.size], np.uint64)
    n_lists = off.size - 1
    seg = ctx.encode(off, vals)
    ids = filter_set(rng, n_set)
    fseg = ctx.encode_lists([ids])
    want = np.zeros(n_lists, np.uint64)
    member = np.zeros(DOCS, bool)
    member[ids] = True
    hit = member[vals]
    want[:] = np.add.reduceat(hit, off[:-1].astype(np.int64)) if n_lists > 1 else [hit.sum()]
    res = {"lists": n_lists, "postings": int(vals.size), "set_ids": int(ids.size), "hits": int(want.sum()), "runs": N}

    d_set = ctx.empty(ids.size + 1)
    n_ids = [0]

    def run_filter():
        _, n_ids[0] = ctx.union_ranges([(fseg, 0, 1)], out=d_set)
    res["filter"] = stats(run_filter)
    assert n_ids[0] == ids.size

    segs = (C.c_void_p * 1)(seg.h)
    first, end = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(n_lists)
    counts = np.zeros(n_lists, np.uint64)
    st = _lib.CountStats()

    def run_count():
        ctx._ck(ctx.lib.ii2_count_ranges(ctx.h, 1, segs, first, end, d_set.data_ptr(), n_ids[0], None, counts.ctypes.data_as(_lib.u64p), n_lists,
                                         C.byref(st)))
    for skip in (1, 0):
        ctx.set_option("count.summary_skip", skip)
        r = stats(run_count)
        r.update(correct=bool(np.array_equal(counts, want)), n_decoded=int(st.n_decoded), n_blocks=int(st.n_blocks),
                 decoded_share=round(st.n_decoded / max(st.n_blocks, 1), 4), n_windows=int(st.n_windows))
        res["count_skip%d" % skip] = r
    ctx.set_option("count.summary_skip", 1)

    # the yardstick: one query per term, the filter's group plus the term's, no output buffer
    CHUNK = 1 << 20
    chunks = []
    for a in range(0, n_lists, CHUNK):
        b = min(a + CHUNK, n_lists)
        qf, gf, gn, qsegs, lf, le = pack_group_batch([([[(fseg, 0, 1)], [(seg, k, k + 1)]], []) for k in range(a, b)])
        chunks.append((b - a, qf, gf, gn, (C.c_void_p * len(qsegs))(*[s.h for s in qsegs]), lf, le, np.zeros(b - a + 1, np.uint64)))
    got = np.zeros(n_lists, np.uint64)

    def run_baseline():
        at = 0
        for nq, qf, gf, gn, hs, lf, le, out_off in chunks:
            rc = ctx.lib.ii2_query_batch_groups(ctx.h, nq, qf.ctypes.data_as(_lib.u64p), gf.ctypes.data_as(_lib.u64p), gn.ctypes.data_as(_lib.u8p),
                                                hs, lf.ctypes.data_as(_lib.u64p), le.ctypes.data_as(_lib.u64p), None, None, 0,
                                                out_off.ctypes.data_as(_lib.u64p))
            if rc != -4:                        # II2_ECAPACITY fills the offsets; no hit at all is II2_OK
                ctx._ck(rc)
            got[at:at + nq] = np.diff(out_off)
            at += nq
    r = stats(run_baseline)
    r["correct"] = bool(np.array_equal(got, want))
    res["baseline_query_batch_groups_cap0"] = r
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
    print(json.dumps(out))
    return 0 if all("error" not in v for v in out.values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
