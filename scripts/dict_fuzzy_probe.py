"""GPU probe: what a typo-tolerant term search costs - ii2_dict_fuzzy on BASELINE.md's stand-in vocabulary, one resident dictionary
of --terms (default 1 000 000) unique [a-zA-Z]{10..19} terms (synth.random_terms, as scripts/dict_match_probe.py makes it).  One
JSON line per measurement, appended to --out (default profiles/dict_fuzzy_probe.jsonl).

For 1, 8 and 16 patterns (terms of the vocabulary with one byte changed) at distance 1 and 2, with and without prefix 2, with and
without II2_FUZZY_TRANSPOSE, the four settings of fuzzy.stage x fuzzy.wide alternating call by call, median [min - max] of --runs
calls after --warmup, between an event pair (ii2_profile_region):
  scan_us     the call with cap = 0: the patterns' upload, k_dict_fuzzy, the two scans, the offsets' gather and the copies
  tested      ii2_fuzzy_stats.n_tested / (patterns x terms): the share of pairs that passed the length and prefix filter
The yardsticks, never the code under test: ii2_dict_match CONTAINS with the same number of patterns, timed in the same run
(match_us); the bytes moved at the 6.29 TB/s a float4 copy reaches (floor_us); and a host DP over the same terms (host_ms, one
pattern, plain Levenshtein, numpy over all the terms at once), whose count of matching terms must agree with the device's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--terms", type=int, default=1_000_000)
ap.add_argument("--counts", default="1,8,16")
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-host", action="store_true", help="skip the host baseline")
ap.add_argument("--out", default=None)
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from inverted_index_2_amd import Context, synth  # noqa: E402
from inverted_index_2_amd._lib import II2_FUZZY_TRANSPOSE, II2_MATCH_CONTAINS  # noqa: E402

OUT = args.out or os.path.join(ROOT, "profiles", "dict_fuzzy_probe.jsonl")
HBM_BYTES_PER_US = 6.29e6


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def summary(t):
    return {"median": round(float(np.median(t)), 1), "min": round(min(t), 1), "max": round(max(t), 1)}


def host_levenshtein_count(pattern, padded, lens, d):
    """terms within d edits of pattern: the plain DP, row by row, over all the terms at once (padded: [N, width] bytes)"""
    n_terms, width = padded.shape
    prev = np.broadcast_to(np.arange(width + 1, dtype=np.int16), (n_terms, width + 1)).copy()
    for i in range(1, len(pattern) + 1):
        cur = np.empty_like(prev)
        cur[:, 0] = i
        diff = (padded != pattern[i - 1]).astype(np.int16)
        for j in range(1, width + 1):
            cur[:, j] = np.minimum(np.minimum(prev[:, j] + 1, cur[:, j - 1] + 1), prev[:, j - 1] + diff[:, j - 1])
        prev = cur
    return int((prev[np.arange(n_terms), lens] <= d).sum())


ctx = Context(0)
terms = sorted(synth.random_terms(args.terms))
off = np.zeros(len(terms) + 1, np.uint64)
off[1:] = np.cumsum([len(t) for t in terms])
d = ctx.dictionary_flat(np.frombuffer(b"".join(terms) + b"\0", np.uint8).copy(), off)
n_bytes = int(off[-1])
moved = n_bytes + 8 * (len(terms) + 1) + 8 * len(terms)
rng = np.random.default_rng(6)


def flat(pats):
    p_off = np.zeros(len(pats) + 1, np.uint64)
    p_off[1:] = np.cumsum([len(p) for p in pats])
    return np.frombuffer(b"".join(pats) + b"\0", np.uint8).copy(), p_off


SETTINGS = [(stage, wide) for stage in (1, 0) for wide in (0, 1)]
for n in [int(x) for x in args.counts.split(",")]:
    picked = [terms[int(i)] for i in rng.choice(len(terms), n, replace=False)]
    pats = [t[:5] + (b"q" if t[5:6] != b"q" else b"r") + t[6:] for t in picked]      # one substitution in the middle
    p_blob, p_off = flat(pats)
    m_blob, m_off = flat([t[3:7] for t in picked])                                   # the yardstick: CONTAINS of 4 bytes
    m_kinds = np.full(n, II2_MATCH_CONTAINS, np.uint8)
    run_off = np.zeros(n + 1, np.uint64)
    for dist in (1, 2):
        for prefix in (0, 2):
            for flags in (0, II2_FUZZY_TRANSPOSE):
                a_dist, a_pre, a_fl = np.full(n, dist, np.uint8), np.full(n, prefix, np.uint8), np.full(n, flags, np.uint8)
                times = {s: [] for s in SETTINGS}
                match_times, results = [], {}
                for r in range(args.warmup + args.runs):
                    for stage, wide in SETTINGS:
                        ctx.set_option("fuzzy.stage", stage)
                        ctx.set_option("fuzzy.wide", wide)
                        ctx.profile_region(True)
                        rc, st = ctx.dict_fuzzy_flat([d], p_blob, p_off, a_dist, a_pre, a_fl, run_off, None, None, None, 0)
                        ctx.profile_region(False)
                        assert rc in (0, -4), rc
                        if r >= args.warmup:
                            times[(stage, wide)].append(ctx.profile_region_ms() * 1e3)
                        results[(stage, wide)] = (run_off.copy(), st.n_matched, st.n_tested, st.word_bits)
                    ctx.profile_region(True)
                    rc, _ = ctx.dict_match_flat([d], m_blob, m_off, m_kinds, run_off, None, None, None, 0)
                    ctx.profile_region(False)
                    assert rc in (0, -4), rc
                    if r >= args.warmup:
                        match_times.append(ctx.profile_region_ms() * 1e3)
                ctx.set_option("fuzzy.stage", 1)
                ctx.set_option("fuzzy.wide", 0)
                base = results[(1, 0)]
                assert all((res[0] == base[0]).all() and res[1:3] == base[1:3] for res in results.values())
                assert base[3] == 32 and results[(1, 1)][3] == 64
                row = {"patterns": n, "dist": dist, "prefix": prefix, "transpose": int(bool(flags)), "terms": len(terms), "dict_bytes": n_bytes,
                       "bytes_moved": moved, "matched_pairs": int(base[1]), "tested": round(base[2] / (n * len(terms)), 4),
                       "floor_us": round(moved / HBM_BYTES_PER_US, 1), "match_contains_us": summary(match_times)}
                for stage, wide in SETTINGS:
                    row["stage%d_w%d" % (stage, 64 if wide else 32)] = summary(times[(stage, wide)])
                if not args.no_host and n == 1 and prefix == 0 and flags == 0:
                    width = max(len(t) for t in terms)
                    padded = np.zeros((len(terms), width), np.uint8)
                    lens = np.array([len(t) for t in terms])
                    for length in set(lens.tolist()):
                        rows = np.flatnonzero(lens == length)
                        padded[rows, :length] = np.frombuffer(b"".join(terms[int(i)] for i in rows), np.uint8).reshape(-1, length)
                    t0 = time.perf_counter()
                    hits = host_levenshtein_count(pats[0], padded, lens, dist)
                    row["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    assert hits == row["matched_pairs"], (hits, row["matched_pairs"])
                emit(row)
d.free()
ctx.close()
