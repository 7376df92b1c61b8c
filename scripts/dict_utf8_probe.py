"""GPU probe: what II2_MATCH_UTF8 costs in ii2_dict_fuzzy - the price of decoding where nothing needs it, and the price of the
hashed symbol lookup where every symbol goes through it.  One JSON line per measurement, appended to --out (default
profiles/dict_utf8_probe.jsonl).

Three resident dictionaries of --terms (default 1 000 000) unique terms each: BASELINE.md's stand-in vocabulary ([a-zA-Z]{10..19},
synth.random_terms, as scripts/dict_fuzzy_probe.py makes it: `ascii`), and the same terms letter by letter in Cyrillic (two-byte
symbols: `cyrillic`) and in CJK ideographs (three-byte symbols: `cjk`).  For 1, 8 and 16 patterns (terms of the dictionary with
one symbol changed) at distance 1 and 2, the unflagged and the flagged call alternating call by call, median [min - max] of --runs
calls after --warmup, between an event pair (ii2_profile_region): the call with cap = 0 - the patterns' upload, k_dict_fuzzy, the
two scans, the offsets' gather and the copies.

--root names the checkout whose library is measured and --label what to call it, so that one session can alternate a parent
build and the tree process by process: a build without the flag (the parent) times the unflagged call alone.  On `ascii` the two
calls of one build must give the same runs; on the other two the flagged call must match at least what the unflagged one does at
the same distance (between well-formed strings the symbol distance never exceeds the byte distance) and find the term each
pattern was made from."""
import argparse
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--terms", type=int, default=1_000_000)
ap.add_argument("--counts", default="1,8,16")
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--dicts", default="ascii,cyrillic,cjk")
ap.add_argument("--root", default=None, help="the checkout to load the package from (default: this one)")
ap.add_argument("--label", default="tree")
ap.add_argument("--out", default=None)
args = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(args.root) if args.root else HERE
sys.path.insert(0, ROOT)
from inverted_index_2_amd import Context, _lib, synth  # noqa: E402

UTF8 = getattr(_lib, "II2_MATCH_UTF8", None)              # None: a build without the flag
OUT = args.out or os.path.join(HERE, "profiles", "dict_utf8_probe.jsonl")


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def summary(t):
    return {"median": round(float(np.median(t)), 1), "min": round(min(t), 1), "max": round(max(t), 1)}


LETTERS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
ALPHABETS = {"ascii": None, "cyrillic": [chr(0x410 + i) for i in range(52)], "cjk": [chr(0x4E00 + 37 * i) for i in range(52)]}


def flat(items):
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in items])
    return np.frombuffer(b"".join(items) + b"\0", np.uint8).copy(), off


ctx = Context(0)
plain = synth.random_terms(args.terms)
rng = np.random.default_rng(6)
for name in args.dicts.split(","):
    al = ALPHABETS[name]
    table = None if al is None else {ord(c): al[i] for i, c in enumerate(LETTERS)}
    terms = sorted(plain) if al is None else sorted(t.decode("ascii").translate(table).encode("utf-8") for t in plain)
    blob, off = flat(terms)
    d = ctx.dictionary_flat(blob, off)
    width = 1 if al is None else len(al[0].encode("utf-8"))
    spare = b"q" if al is None else chr(0x44F if name == "cyrillic" else 0x9FA5).encode("utf-8")      # a symbol the alphabet lacks (q / r: as dict_fuzzy_probe)
    for n in [int(x) for x in args.counts.split(",")]:
        picked = [terms[int(i)] for i in rng.choice(len(terms), n, replace=False)]
        pats = [t[:5 * width] + (spare if t[5 * width:6 * width] != spare else b"r") + t[6 * width:] for t in picked]      # one symbol changed in the middle
        assert all(len(p) <= 64 for p in pats)
        p_blob, p_off = flat(pats)
        run_off = np.zeros(n + 1, np.uint64)
        for dist in (1, 2):
            a_dist, a_pre = np.full(n, dist, np.uint8), np.zeros(n, np.uint8)
            modes = [("bytes", np.zeros(n, np.uint8))] + ([("utf8", np.full(n, UTF8, np.uint8))] if UTF8 is not None else [])
            times, results = {m: [] for m, _ in modes}, {}
            for r in range(args.warmup + args.runs):
                for mode, a_fl in modes:
                    ctx.profile_region(True)
                    rc, st = ctx.dict_fuzzy_flat([d], p_blob, p_off, a_dist, a_pre, a_fl, run_off, None, None, None, 0)
                    ctx.profile_region(False)
                    assert rc in (0, -4), rc
                    if r >= args.warmup:
                        times[mode].append(ctx.profile_region_ms() * 1e3)
                    results[mode] = (run_off.copy(), int(st.n_matched), int(st.n_tested), int(st.word_bits))
            row = {"build": args.label, "dict": name, "patterns": n, "dist": dist, "terms": len(terms), "dict_bytes": int(off[-1]),
                   "pattern_bytes": max(len(p) for p in pats)}
            for mode, _ in modes:
                row[mode + "_us"] = summary(times[mode])
                row[mode + "_matched"], row[mode + "_tested"], row[mode + "_word_bits"] = results[mode][1:]
            if "utf8" in results:
                if al is None:
                    assert (results["utf8"][0] == results["bytes"][0]).all() and results["utf8"][1:] == results["bytes"][1:]
                else:
                    assert results["utf8"][1] >= results["bytes"][1] and results["utf8"][1] >= n
            emit(row)
    d.free()
ctx.close()
