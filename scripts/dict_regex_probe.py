"""GPU probe: what a regular-expression term search costs - ii2_dict_regex on BASELINE.md's stand-in vocabulary, one resident
dictionary of --terms (default 1 000 000) unique [a-zA-Z]{10..19} terms (synth.random_terms, as scripts/dict_fuzzy_probe.py makes
it).  One JSON line per measurement, appended to --out (default profiles/dict_regex_probe.jsonl).

Per row, regex.stage 1 and 0 and the yardstick alternating call by call, median [min - max] of --runs calls after --warmup,
between an event pair (ii2_profile_region): the call with cap = 0 - the patterns' upload, k_dict_regex, the two scans, the
offsets' gather and the copies.
  twins      patterns that ii2_dict_match answers as well (`.*time.*` / CONTAINS time, `.*ing` / SUFFIX, `a.c.*` / GLOB a?c*,
             `.*(abc|xyz|qrs).*` / three CONTAINS, the NOCASE forms of the first two; 1 and 8 patterns): the yardstick is that
             call on the twin, timed in the same run (match_us), and the match counts must agree (for the alternation, one
             pattern against three, the sets of matching terms)
  own        patterns no other mode answers (`[a-f]{10,12}`, `.*[A-Z]{3}[a-z]+`, a pattern of 64 positions): the yardsticks are
             the bytes moved at the 6.29 TB/s a float4 copy reaches (floor_us) and `re` on the host over the same terms
             (host_ms), whose count must agree"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--terms", type=int, default=1_000_000)
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-host", action="store_true", help="skip the host baseline")
ap.add_argument("--out", default=None)
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from inverted_index_2_amd import Context, synth  # noqa: E402
from inverted_index_2_amd._lib import II2_MATCH_CONTAINS, II2_MATCH_GLOB, II2_MATCH_NOCASE, II2_MATCH_SUFFIX  # noqa: E402

OUT = args.out or os.path.join(ROOT, "profiles", "dict_regex_probe.jsonl")
HBM_BYTES_PER_US = 6.29e6


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def summary(t):
    return {"median": round(float(np.median(t)), 1), "min": round(min(t), 1), "max": round(max(t), 1)}


ctx = Context(0)
terms = sorted(synth.random_terms(args.terms))
off = np.zeros(len(terms) + 1, np.uint64)
off[1:] = np.cumsum([len(t) for t in terms])
d = ctx.dictionary_flat(np.frombuffer(b"".join(terms) + b"\0", np.uint8).copy(), off)
n_bytes = int(off[-1])
moved = n_bytes + 8 * (len(terms) + 1) + 8 * len(terms)


def flat(pats):
    p_off = np.zeros(len(pats) + 1, np.uint64)
    p_off[1:] = np.cumsum([len(p) for p in pats])
    return np.frombuffer(b"".join(pats) + b"\0", np.uint8).copy(), p_off


def timed(call):
    ctx.profile_region(True)
    rc, st = call()
    ctx.profile_region(False)
    assert rc in (0, -4), rc
    return ctx.profile_region_ms() * 1e3, st


def matched_terms(result):
    """the indices of the terms that any pattern of a call matches, from its runs"""
    _, first, end, _, _ = result
    hit = np.zeros(len(terms) + 1, np.int64)
    np.add.at(hit, first.astype(np.int64), 1)
    np.add.at(hit, end.astype(np.int64), -1)
    return np.flatnonzero(np.cumsum(hit)[:-1] > 0).tolist()


def measure(name, pats, flags, twin=None):
    """twin: (patterns, kinds) of the ii2_dict_match call that answers the same"""
    p_blob, p_off = flat(pats)
    p_fl = np.full(len(pats), flags, np.uint8)
    run_off = np.zeros(len(pats) + 1, np.uint64)
    if twin:
        m_blob, m_off = flat(twin[0])
        m_kinds = np.array(twin[1], np.uint8)
        m_run_off = np.zeros(len(twin[0]) + 1, np.uint64)
    times, match_times, stats = {1: [], 0: []}, [], {}
    for r in range(args.warmup + args.runs):
        for stage in (1, 0):
            ctx.set_option("regex.stage", stage)
            us, st = timed(lambda: ctx.dict_regex_flat([d], p_blob, p_off, p_fl, run_off, None, None, None, 0))
            stats[stage] = (run_off.copy(), st.n_matched, st.n_tested, st.max_positions)
            if r >= args.warmup:
                times[stage].append(us)
        if twin:
            us, m_st = timed(lambda: ctx.dict_match_flat([d], m_blob, m_off, m_kinds, m_run_off, None, None, None, 0))
            if r >= args.warmup:
                match_times.append(us)
    ctx.set_option("regex.stage", 1)
    assert (stats[1][0] == stats[0][0]).all() and stats[1][1:] == stats[0][1:]
    row = {"name": name, "patterns": len(pats), "nocase": int(bool(flags)), "positions": int(stats[1][3]), "terms": len(terms), "dict_bytes": n_bytes,
           "bytes_moved": moved, "matched_pairs": int(stats[1][1]), "tested": round(stats[1][2] / (len(pats) * len(terms)), 4),
           "floor_us": round(moved / HBM_BYTES_PER_US, 1), "stage1": summary(times[1]), "stage0": summary(times[0])}
    if twin:
        row["match_us"] = summary(match_times)
        if len(twin[0]) == len(pats):
            assert int(m_st.n_matched) == row["matched_pairs"], (name, int(m_st.n_matched), row["matched_pairs"])
        else:               # an alternation of three is ONE regex and three CONTAINS patterns: the TERMS either call matches are compared
            assert matched_terms(ctx.dict_regex([d], pats, flags)) == matched_terms(ctx.dict_match([d], twin[0], m_kinds)), name
    elif not args.no_host:
        rx = [re.compile(p, re.DOTALL | (re.IGNORECASE if flags else 0)) for p in pats]
        t0 = time.perf_counter()
        hits = sum(1 for x in rx for t in terms if x.fullmatch(t))
        row["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        assert hits == row["matched_pairs"], (name, hits, row["matched_pairs"])
    emit(row)


C, S, G, NC = II2_MATCH_CONTAINS, II2_MATCH_SUFFIX, II2_MATCH_GLOB, II2_MATCH_NOCASE
measure("contains", [b".*time.*"], 0, ([b"time"], [C]))
measure("suffix", [b".*ing"], 0, ([b"ing"], [S]))
measure("glob", [b"a.c.*"], 0, ([b"a?c*"], [G]))
measure("contains-3", [b".*(abc|xyz|qrs).*"], 0, ([b"abc", b"xyz", b"qrs"], [C, C, C]))
measure("contains-nocase", [b".*time.*"], NC, ([b"time"], [C | NC]))
measure("suffix-nocase", [b".*ing"], NC, ([b"ing"], [S | NC]))
stems = [b"time", b"ing", b"abc", b"xyz", b"qrs", b"err", b"out", b"con"]
measure("contains-x8", [b".*" + s + b".*" for s in stems], 0, (stems, [C] * 8))
measure("suffix-x8", [b".*" + s for s in stems], 0, (stems, [S] * 8))
measure("class-counted", [b"[a-f]{10,12}"], 0)
measure("class-run", [b".*[A-Z]{3}[a-z]+"], 0)
measure("64-positions", [b"[a-zA-Z]{0,64}"], 0)
measure("64-positions-x8", [b"[a-zA-Z]{0,%d}[a-m]{0,%d}" % (64 - i, i) for i in range(8)], 0)
d.free()
ctx.close()
