"""Bulk ingestion (ii2_seg_build / PutBatch) against what a caller had to do without it, every case checked against numpy at the size
it is timed.  Cases (PROBE_CASES=p,q; default both):
  p   one Shard, 200 docs of 8 terms from a 50-term vocabulary (the (s) shape of DESIGN.md §4.1h), wall clock:
        yardstick  200 x put, then merge(2, 64) until one segment is left - any library can run it: --libdir points at a directory
                   with libii2_hip.so and libii2_host.so built from the commit to compare with;
        new        one put_batch (skipped when the libraries lack it).
  q   the sort rate: build_segment from device arrays of 8 M pairs - 1 M docs x 8 terms drawn from a 100 000-term Zipf vocabulary
      (p(rank) ~ 1 / rank, seeded with synth.GLOBAL_SEED) - wall clock and device time (profile_region); beside it, with
      PROBE_TORCH=1, torch.sort of the same keys as int64 + torch.unique_consecutive on the same card.
One JSON line: per case and variant the median, minimum and maximum of PROBE_N (default 15, at least 10) timed runs after 3 warm-up
runs, in microseconds.  Run parent and new libraries in alternating processes; under `rocprofv3 --kernel-trace --stats -- python
scripts/put_batch_probe.py` (PROBE_CASES=q) for the device time per kernel."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--libdir", default=None, help="directory whose libii2_hip.so / libii2_host.so are loaded instead of the package's own")
ap.add_argument("--label", default=None, help="what the JSON line calls the libraries (default: this commit / the --libdir)")
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if args.libdir:      # (the host mirror's path is read when its module is imported)
    os.environ["II2_HOST_LIB"] = os.path.join(os.path.abspath(args.libdir), "libii2_host.so")
from inverted_index_2_amd import _lib  # noqa: E402
if args.libdir:
    _lib.LIB_PATH = os.path.join(os.path.abspath(args.libdir), "libii2_hip.so")
    other = C.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.PROTOTYPES if not hasattr(other, n)]:      # a library from before an entry point: the yardstick only
        _lib.PROTOTYPES.pop(name)
from inverted_index_2_amd import Context, host, synth  # noqa: E402
if args.libdir:      # a host library from before PutBatch: the binding types every export it knows, so the absent ones get a stand-in
    host._host = C.CDLL(host.HOST_LIB_PATH)
    for name in ("ii2h_put_batch", "ii2h_index_segment_count"):
        if not hasattr(host._host, name):
            setattr(host._host, name, type("Absent", (), {})())
from inverted_index_2_amd._lib import II2_DEVICE  # noqa: E402

N = max(int(os.environ.get("PROBE_N", "15")), 10)
CASES = os.environ.get("PROBE_CASES", "p,q").split(",")
have_new = "ii2_seg_build" in _lib.PROTOTYPES


def summary(t):
    return {"median_us": round(float(np.median(t)), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def timed(fn, warm=3):
    """fn() returns the seconds it measured itself"""
    for _ in range(warm):
        fn()
    return summary([fn() * 1e6 for _ in range(N)])


def case_p(ctx):
    rng = np.random.default_rng(8)
    vocab = [b"term%02d" % i for i in range(50)]
    docs = [([vocab[i] for i in rng.choice(50, 8, replace=False)], int(v)) for v in rng.choice(100_000, 200, replace=False)]
    want = {}
    for terms, v in docs:
        for t in terms:
            want.setdefault(t, []).append(v)
    want = sorted((t, sorted(set(vs))) for t, vs in want.items())
    res, last = {"docs": len(docs), "pairs": 8 * len(docs)}, {}

    def puts_then_merges():
        s = host.Shard(ctx)
        t0 = time.perf_counter()
        for terms, v in docs:
            s.put(terms, v)
        merges = 0
        while s.n_segments > 1:
            s.merge(2, 64)
            merges += 1
        dt = time.perf_counter() - t0
        last["yardstick"], last["merges"] = s.read(), merges
        s.close()
        return dt

    def put_batch():
        s = host.Shard(ctx)
        t0 = time.perf_counter()
        s.put_batch(docs)
        dt = time.perf_counter() - t0
        last["new"], last["segments"] = s.read(), s.n_segments
        s.close()
        return dt

    res["yardstick"] = timed(puts_then_merges)
    res["yardstick"].update(correct=last["yardstick"] == want, merges=last["merges"])
    if have_new:
        res["new"] = timed(put_batch)
        res["new"].update(correct=last["new"] == want, segments=last["segments"])
    return res


def case_q(ctx):
    n_docs, per_doc, n_terms = 1_000_000, 8, 100_000
    rng = np.random.default_rng(synth.GLOBAL_SEED)
    cdf = np.cumsum(1.0 / np.arange(1, n_terms + 1))
    lid = np.searchsorted(cdf, rng.random(n_docs * per_doc) * cdf[-1]).astype(np.uint32)
    val = np.repeat(np.arange(n_docs, dtype=np.uint32), per_doc)
    perm = rng.permutation(lid.size)             # (pairs arrive in no order)
    lid, val = lid[perm], val[perm]
    keys = lid.astype(np.uint64) << np.uint64(32) | val.astype(np.uint64)
    uniq = np.unique(keys)
    res = {"pairs": int(lid.size), "lists": n_terms, "postings": int(uniq.size)}
    if have_new:
        d_lid, d_val = ctx.empty(lid.size).upload(lid), ctx.empty(val.size).upload(val)
        dev_ms, st_last = [], [None]

        def build():
            t0 = time.perf_counter()
            ctx.profile_region(True)
            seg, st = ctx.build_segment(d_lid, d_val, n_terms, where=II2_DEVICE)
            ctx.profile_region(False)
            dt = time.perf_counter() - t0
            dev_ms.append(ctx.profile_region_ms())
            st_last[0] = st
            seg.free()
            return dt
        res["new_wall"] = timed(build)
        res["new_device"] = summary([1e3 * x for x in dev_ms[-N:]])
        res["pairs_per_s_device"] = round(lid.size / (res["new_device"]["median_us"] * 1e-6))
        res["pairs_per_s_wall"] = round(lid.size / (res["new_wall"]["median_us"] * 1e-6))
        seg, st = ctx.build_segment(d_lid, d_val, n_terms, where=II2_DEVICE)
        po, v = seg.decode()
        res["correct"] = bool(np.array_equal(v, (uniq & np.uint64(0xFFFFFFFF)).astype(np.uint32)) and
                              np.array_equal(po, np.searchsorted(uniq >> np.uint64(32), np.arange(n_terms + 1, dtype=np.uint64))) and
                              st.n_postings == uniq.size)
        res["passes"] = int(st.n_passes)
    if os.environ.get("PROBE_TORCH", "0") == "1":
        import torch
        t_keys = torch.from_numpy(keys.astype(np.int64)).cuda()
        out = [None]

        def sort_unique():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s, _ = torch.sort(t_keys)
            out[0] = torch.unique_consecutive(s)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        res["torch_sort_unique_wall"] = timed(sort_unique)
        res["torch_correct"] = bool(np.array_equal(out[0].cpu().numpy().astype(np.uint64), uniq))
    return res


def main():
    ctx = Context(0)
    line = {"lib": args.label or args.libdir or "this commit", "has_seg_build": have_new, "runs": N}
    if "p" in CASES:
        line["p_200_docs_8_terms_50_vocab"] = case_p(ctx)
    if "q" in CASES:
        line["q_8m_pairs_100k_zipf_terms"] = case_q(ctx)
    print(json.dumps(line))
    ctx.close()


if __name__ == "__main__":
    main()
