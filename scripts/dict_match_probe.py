"""GPU probe: what a substring / suffix / wildcard term search costs - ii2_dict_match on BASELINE.md's stand-in vocabulary, one
resident dictionary of --terms (default 1 000 000) unique [a-zA-Z]{10..19} terms (synth.random_terms, seeded as
tests/test_config1_cpu.py seeds it).  One JSON line per measurement, appended to --out (default profiles/dict_match_probe.jsonl).

For 1, 8 and 64 patterns of each kind (CONTAINS, CONTAINS | NOCASE, SUFFIX, GLOB), option match.stage 1 and 0 alternating call
by call, median [min - max] of --runs calls after --warmup, between an event pair (ii2_profile_region):
  scan_us   the call with cap = 0: the patterns' upload, k_dict_match, the two scans, the offsets' gather and the copies of
            run_off and the counters - every term byte is read here
  call_us   the whole call with a buffer that fits: the above, the host's turn after the first wait, k_match_place and the
            copies of the runs
  gbps      the dictionary's bytes + its offsets + the match words written (8 bytes per term), over scan_us
  floor_us  the same bytes at the 6.29 TB/s a float4 copy reaches on this GPU: what no scan can beat
and the only baseline there is, the same search on the host over the same terms (host_ms, one run): bytes.find over the terms
joined by newlines for the literal kinds, one compiled `re` per pattern over the same blob for globs (`*` = [^\\n]*), bytes.lower
first under NOCASE.  The host's and the device's numbers of matching (pattern, term) pairs must agree."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--terms", type=int, default=1_000_000)
ap.add_argument("--counts", default="1,8,64")
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-host", action="store_true", help="skip the host baseline")
ap.add_argument("--out", default=None)
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from inverted_index_2_amd import Context, synth  # noqa: E402
from inverted_index_2_amd._lib import II2_MATCH_CONTAINS, II2_MATCH_GLOB, II2_MATCH_NOCASE, II2_MATCH_SUFFIX  # noqa: E402

OUT = args.out or os.path.join(ROOT, "profiles", "dict_match_probe.jsonl")
HBM_BYTES_PER_US = 6.29e6
KINDS = {"contains": II2_MATCH_CONTAINS, "contains_nocase": II2_MATCH_CONTAINS | II2_MATCH_NOCASE, "suffix": II2_MATCH_SUFFIX, "glob": II2_MATCH_GLOB}


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def summary(t):
    return {"median": round(float(np.median(t)), 1), "min": round(min(t), 1), "max": round(max(t), 1)}


def patterns_of(name, n, terms, rng):
    """n distinct patterns cut out of the vocabulary: 4 letters from inside a term (contains), its last 3 (suffix), and for globs a
    mix of *abc*, ab*yz, a?c* and *ab?d"""
    out = []
    while len(out) < n:
        t = terms[int(rng.integers(0, len(terms)))]
        i = int(rng.integers(1, len(t) - 5))
        if name.startswith("contains"):
            p = t[i:i + 4]
        elif name == "suffix":
            p = t[-3:]
        else:
            p = (b"*" + t[i:i + 3] + b"*", t[:2] + b"*" + t[-2:], t[:1] + b"?" + t[2:3] + b"*", b"*" + t[-4:-2] + b"?" + t[-1:])[len(out) % 4]
        if p not in out:
            out.append(p)
    return out


def host_count(name, patterns, blob, lowered):
    """(pattern, term) pairs that match, on the host: the terms are the lines of blob"""
    pairs = 0
    for p in patterns:
        text = blob
        if name.endswith("nocase"):
            text, p = lowered(), p.lower()
        if name == "glob":
            rx = re.compile(b"^" + b"".join(b"[^\n]*" if c == 42 else b"[^\n]" if c == 63 else re.escape(bytes([c])) for c in p) + b"$", re.MULTILINE)
            pairs += sum(1 for _ in rx.finditer(text))
            continue
        if name == "suffix":
            p = p + b"\n"
        i = text.find(p)
        while i >= 0:                                   # one hit per term: on to the next line
            pairs += 1
            j = text.find(b"\n", i + len(p) - (1 if name == "suffix" else 0))
            i = text.find(p, j + 1) if j >= 0 else -1
    return pairs


ctx = Context(0)
terms = sorted(synth.random_terms(args.terms))
off = np.zeros(len(terms) + 1, np.uint64)
off[1:] = np.cumsum([len(t) for t in terms])
d = ctx.dictionary_flat(np.frombuffer(b"".join(terms) + b"\0", np.uint8).copy(), off)
n_bytes = int(off[-1])
moved = n_bytes + 8 * (len(terms) + 1) + 8 * len(terms)
blob = b"\n".join(terms) + b"\n"
_low = []


def lowered():
    if not _low:
        _low.append(blob.lower())
    return _low[0]


rng = np.random.default_rng(5)
for name, kind in KINDS.items():
    for n in [int(x) for x in args.counts.split(",")]:
        pats = patterns_of(name, n, terms, rng)
        p_off = np.zeros(n + 1, np.uint64)
        p_off[1:] = np.cumsum([len(p) for p in pats])
        p_blob = np.frombuffer(b"".join(pats) + b"\0", np.uint8).copy()
        kinds = np.full(n, kind, np.uint8)
        run_off = np.zeros(n + 1, np.uint64)
        rc, st = ctx.dict_match_flat([d], p_blob, p_off, kinds, run_off, None, None, None, 0)
        assert rc in (0, -4), rc
        need = int(run_off[-1])
        first, end, which = np.zeros(need + 1, np.uint64), np.zeros(need + 1, np.uint64), np.zeros(need + 1, np.uint32)
        times = {(stage, what): [] for stage in (1, 0) for what in ("scan", "call")}
        results = {}
        for r in range(args.warmup + args.runs):
            for stage in (1, 0):
                ctx.set_option("match.stage", stage)
                for what, cap in (("scan", 0), ("call", need + 1)):
                    ctx.profile_region(True)
                    rc, st = ctx.dict_match_flat([d], p_blob, p_off, kinds, run_off, first, end, which, cap)
                    ctx.profile_region(False)
                    assert rc == (-4 if cap < need else 0), rc
                    if r >= args.warmup:
                        times[(stage, what)].append(ctx.profile_region_ms() * 1e3)
                results[stage] = (run_off.copy(), first[:need].copy(), end[:need].copy(), st.n_matched, st.n_staged, st.n_global)
        ctx.set_option("match.stage", 1)
        assert all((a == b).all() for a, b in zip(results[0][:3], results[1][:3])) and results[0][3] == results[1][3]
        row = {"kind": name, "patterns": n, "terms": len(terms), "dict_bytes": n_bytes, "bytes_moved": moved, "matched_pairs": int(results[1][3]), "runs": need,
               "staged_workgroups": int(results[1][4]), "global_workgroups_when_staged": int(results[1][5]), "floor_us": round(moved / HBM_BYTES_PER_US, 1)}
        for stage in (1, 0):
            scan = summary(times[(stage, "scan")])
            row["stage%d" % stage] = {"scan_us": scan, "call_us": summary(times[(stage, "call")]), "gbps": round(moved / scan["median"] / 1e3, 1)}
        if not args.no_host:
            t0 = time.perf_counter()
            pairs = host_count(name, pats, blob, lowered)
            row["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            assert pairs == row["matched_pairs"], (pairs, row["matched_pairs"])
        emit(row)
d.free()
ctx.close()
