"""The dictionary build on the device (ii2_dict_build / PutBatch's device route, SetBuild) against the host's std::sort +
std::unique + one bisection per occurrence, on the same libraries, the two routes alternating run by run; every case checked
against Python at the size it is timed.  Cases (PROBE_CASES=p,q,r; default p,r):
  p   one Shard, 200 docs of 8 terms from a 50-term vocabulary through put_batch: set_build(0) against set_build(1).
  q   8 M occurrences - 1 M docs x 8 terms drawn from a 100 000-term Zipf vocabulary of [a-zA-Z]{10..19} (p(rank) ~ 1 / rank) -
      through put_batch under both modes, and ii2_dict_build alone from device arrays: wall clock and device time
      (profile_region), the passes it ran and the bytes they move, computed from the plan.  Under `rocprofv3 --kernel-trace
      --stats -- python scripts/dict_build_probe.py` (PROBE_CASES=q PROBE_Q_BUILD_ONLY=1: the build alone, a run of its own) for
      the device time per kernel.
  r   batch sizes doubling from 256 to 1 M occurrences (docs of 8 terms, a vocabulary of a tenth of the occurrences) through
      put_batch under both modes: the threshold of SetBuild(-1) is the smallest size at which the device route's [min - max]
      lies wholly below the host route's.
The timed region is the C call ii2h_put_batch on arrays packed beforehand (a fresh Shard per run).  One JSON line per case:
median, minimum and maximum of PROBE_N (default 15) timed runs after 3 warm-up runs, in microseconds."""
import ctypes as C
import json
import os
import random
import string
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inverted_index_2_amd import Context, host  # noqa: E402
from inverted_index_2_amd._lib import II2_DEVICE  # noqa: E402

N = max(int(os.environ.get("PROBE_N", "15")), 1)
WARM = 3
CASES = os.environ.get("PROBE_CASES", "p,r").split(",")


def summary(t):
    return {"median_us": round(float(np.median(t)), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def make_vocab(n, seed=258):
    rnd = random.Random(seed)
    seen = set()
    while len(seen) < n:
        seen.add("".join(rnd.choice(string.ascii_letters) for _ in range(rnd.randint(10, 19))).encode())
    out = sorted(seen)
    rnd.shuffle(out)
    return out


def pack(vocab, draws, per_doc):
    """flat arrays of ii2h_put_batch: occurrence i is vocab[draws[i]], doc d owns occurrences [d * per_doc, (d + 1) * per_doc)"""
    lens = np.array([len(t) for t in vocab], np.uint64)
    voff = np.zeros(len(vocab) + 1, np.uint64)
    voff[1:] = np.cumsum(lens)
    vblob = np.frombuffer(b"".join(vocab), np.uint8)
    off = np.zeros(draws.size + 1, np.uint64)
    off[1:] = np.cumsum(lens[draws])
    idx = np.repeat(voff[draws].astype(np.int64) - off[:-1].astype(np.int64), lens[draws].astype(np.int64)) + np.arange(int(off[-1]), dtype=np.int64)
    blob = np.concatenate([vblob[idx], np.zeros(1, np.uint8)])
    n_docs = draws.size // per_doc
    doc_first = (np.arange(n_docs + 1, dtype=np.uint64) * np.uint64(per_doc))
    vals = np.arange(n_docs + 1, dtype=np.uint32)
    return blob, off, doc_first, vals, n_docs


def expected(vocab, draws, per_doc):
    """Read() of the shard: every drawn term with the docs that drew it"""
    order = np.argsort(draws, kind="stable")
    d_sorted, docs = draws[order], (order // per_doc).astype(np.uint32)
    starts = np.flatnonzero(np.r_[True, d_sorted[1:] != d_sorted[:-1]])
    ends = np.r_[starts[1:], d_sorted.size]
    return sorted((vocab[int(d_sorted[a])], np.unique(docs[a:b]).tolist()) for a, b in zip(starts, ends))


def routes(ctx, vocab, draws, per_doc, check=True):
    """put_batch under mode 0 and mode 1, alternating; -> {"host": summary, "device": summary}"""
    blob, off, doc_first, vals, n_docs = pack(vocab, draws, per_doc)
    want = expected(vocab, draws, per_doc) if check else None
    times, correct = {0: [], 1: []}, {0: True, 1: True}
    for run in range(WARM + N):
        for mode in (0, 1):
            s = host.Shard(ctx)
            s.set_build(mode)
            t0 = time.perf_counter()
            rc = s.lib.ii2h_put_batch(s.h, blob.ctypes.data, off.ctypes.data, doc_first.ctypes.data, vals.ctypes.data, n_docs)
            dt = time.perf_counter() - t0
            s._ck(rc)
            if run >= WARM:
                times[mode].append(dt * 1e6)
            if check and run == WARM + N - 1:
                correct[mode] = s.read() == want and s.n_segments == 1
            s.close()
        if draws.size >= (1 << 20):
            print("run", run, "of", WARM + N, "at", draws.size, "occurrences", file=sys.stderr, flush=True)      # (a sign of life: a run takes seconds)
    return {"occurrences": int(draws.size), "vocabulary": len(vocab), "host": dict(summary(times[0]), correct=correct[0]),
            "device": dict(summary(times[1]), correct=correct[1])}


def case_p(ctx):
    rng = np.random.default_rng(8)
    vocab = [b"term%02d" % i for i in range(50)]
    draws = np.concatenate([rng.choice(50, 8, replace=False) for _ in range(200)])
    return routes(ctx, vocab, draws, 8)


def zipf_draws(rng, n, n_terms):
    cdf = np.cumsum(1.0 / np.arange(1, n_terms + 1))
    return np.searchsorted(cdf, rng.random(n) * cdf[-1]).astype(np.int64)


def case_q(ctx):
    n_terms, n = 100_000, 8_000_000
    vocab = make_vocab(n_terms)
    draws = zipf_draws(np.random.default_rng(20240229), n, n_terms)
    res = routes(ctx, vocab, draws, 8) if os.environ.get("PROBE_Q_BUILD_ONLY", "0") != "1" else {"occurrences": n, "vocabulary": n_terms}
    # the build alone, from device arrays
    blob, off, _, _, _ = pack(vocab, draws, 8)
    d_blob, d_off = ctx.empty(blob.size, np.uint8).upload(blob), ctx.empty(off.size, np.uint64).upload(off)
    wall, dev, st = [], [], None
    for run in range(WARM + N):
        t0 = time.perf_counter()
        ctx.profile_region(True)
        d, ids, st = ctx.build_dictionary(d_blob, d_off, II2_DEVICE)
        ctx.profile_region(False)
        dt = time.perf_counter() - t0
        if run >= WARM:
            wall.append(dt * 1e6)
            dev.append(ctx.profile_region_ms() * 1e3)
        if run == WARM + N - 1:
            uniq = sorted({vocab[int(i)] for i in np.unique(draws)})
            where = {t: i for i, t in enumerate(uniq)}
            rank = np.array([where.get(t, 0) for t in vocab], np.uint32)
            res["build_correct"] = bool(d.export() == uniq and np.array_equal(ids.download(n), rank[draws]))
        d.free()
        ids.free()
    res["build_wall"], res["build_device"] = summary(wall), summary(dev)
    res["passes"] = int(st.n_passes)
    res["min_len"], res["max_len"], res["unique"] = int(st.min_len), int(st.max_len), int(st.n_unique)
    # a pass reads the keys twice and the indices once and writes both: (8 + 8 + 4 + 8 + 4) bytes per occurrence
    res["pass_bytes"] = int(st.n_passes) * n * 32
    return res


def case_r(ctx):
    out = []
    size = 256
    while size <= (1 << 20):
        n_terms = max(size // 10, 8)
        vocab = make_vocab(n_terms, seed=size)
        draws = zipf_draws(np.random.default_rng(size), size, n_terms)
        out.append(routes(ctx, vocab, draws, 8))
        size *= 2
    first = next((r["occurrences"] for i, r in enumerate(out) if all(x["device"]["max_us"] < x["host"]["min_us"] for x in out[i:])), None)
    return {"sizes": out, "device_wholly_below_host_from": first}


def main():
    ctx = Context(0)
    for name, fn in (("p", case_p), ("q", case_q), ("r", case_r)):
        if name in CASES:
            print(json.dumps({"case": name, "runs": N, "warmups": WARM, **fn(ctx)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
