"""GPU probe: what turning terms into list ranges costs - ii2_dict_find's kernel, and the host mirror's IntersectMany
with its terms looked up on the host against the device.  One JSON line per measurement, appended to --out (default
profiles/dict_find_probe.jsonl).  Parts (--parts kernel,mirror):
  kernel  k = 8 resident dictionaries of --terms (default 1 000 000) terms of 10 - 19 bytes each (synth.random_terms, BASELINE.md's
          stand-in), device arrays in and out: Q = 64, 4096 and 98 304 exact probes (half of them terms of the dictionaries) and
          4096 prefix probes (the first 3 bytes of a term); device time of one call between an event pair (ii2_profile_region:
          the memset, the offsets' check, the lookup kernel and the 16-byte copy), median [min - max] of --runs calls after
          --warmup.  A library that still has the option dict_find.staged (the LDS-sample form of the kernel, measured once and
          removed: DESIGN 4.4b) is timed with it on and off, the samples alternating, and the two results compared.
  mirror  one shard of 8 segments of --mirror-terms (default 100 000) terms each (8 x put_batch), Q = --qs (default 64,512,4096)
          queries of three terms, nine of ten terms present; wall time of the C call ii2h_intersect_batch alone (the arrays are
          packed before the clock starts), mode 0 against mode 1 alternating (--modes 0: one mode alone, whose calls then find
          the caches as their predecessor left them, like the parent's), median [min - max].  With --libdir the libraries of
          THAT directory run it (libii2_hip.so and libii2_host.so built from the commit to compare with - they have no mode: one
          row, "parent").  Run the two in alternating processes; the spread between the processes of one kind is the noise."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--libdir", default=None, help="directory whose libii2_hip.so / libii2_host.so are loaded instead of the package's own (mirror part only)")
ap.add_argument("--parts", default="kernel,mirror")
ap.add_argument("--terms", type=int, default=1_000_000)
ap.add_argument("--mirror-terms", type=int, default=100_000)
ap.add_argument("--qs", default="64,512,4096")
ap.add_argument("--modes", default="0,1", help="mirror part: the ii2h_set_resolve modes timed, alternating call by call (one mode: that mode alone)")
ap.add_argument("--runs", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--note", default=None, help="copied into every row (which process of an alternating series, say)")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if args.libdir:      # (the host mirror's path is read when its module is imported)
    os.environ["II2_HOST_LIB"] = os.path.join(os.path.abspath(args.libdir), "libii2_host.so")
from inverted_index_2_amd import _lib  # noqa: E402
if args.libdir:
    _lib.LIB_PATH = os.path.join(os.path.abspath(args.libdir), "libii2_hip.so")
    other = C.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.PROTOTYPES if not hasattr(other, n)]:      # a library from before an entry point
        _lib.PROTOTYPES.pop(name)
from inverted_index_2_amd import Context, host, synth  # noqa: E402
if args.libdir:      # a host library from before the switch: the binding types every export it knows, so the absent one gets a stand-in
    host._host = C.CDLL(host.HOST_LIB_PATH)
    for name in ("ii2h_set_resolve", "ii2h_set_first_cap", "ii2h_second_calls"):
        if not hasattr(host._host, name):
            setattr(host._host, name, type("Absent", (), {})())
from inverted_index_2_amd._lib import II2_DEVICE  # noqa: E402
from inverted_index_2_amd.engine import DeviceArray, II2Error  # noqa: E402

OUT = args.out or os.path.join(ROOT, "profiles", "dict_find_probe.jsonl")
PARTS = args.parts.split(",")
have_switch = not args.libdir or "ii2_dict_find" in _lib.PROTOTYPES


def emit(row):
    row["build"] = "parent" if args.libdir else "this"
    if args.note:
        row["note"] = args.note
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def summary(t, unit="us"):
    return {"median_" + unit: round(float(np.median(t)), 2), "min_" + unit: round(min(t), 2), "max_" + unit: round(max(t), 2)}


def pack(terms):
    off = np.zeros(len(terms) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in terms])
    return np.frombuffer(b"".join(terms) + b"\0", np.uint8).copy(), off


def part_kernel(ctx):
    k = 8
    every = synth.random_terms(k * args.terms + 49_152, seed=11)
    spare, every = every[k * args.terms:], every[:k * args.terms]
    dicts = [ctx.dictionary_flat(*pack(sorted(every[s::k]))) for s in range(k)]
    rng = np.random.default_rng(12)
    forms = ["plain"]
    try:
        ctx.set_option("dict_find.staged", 1)
        forms.append("staged")
    except II2Error:
        pass
    for q, prefix in ((64, 0), (4096, 0), (98_304, 0), (4096, 1)):
        held = [every[int(i)] for i in rng.integers(0, len(every), q - q // 2)]
        probes = [t[:3] for t in held] + [t[:3] for t in spare[:q // 2]] if prefix else held + spare[:q // 2]
        blob, off = pack(probes)
        d_blob, d_off = DeviceArray(ctx, blob.size, np.uint8).upload(blob), DeviceArray(ctx, off.size, np.uint64).upload(off)
        d_flags = DeviceArray(ctx, q, np.uint8).upload(np.full(q, prefix, np.uint8))
        d_first, d_end = DeviceArray(ctx, q * k, np.uint64), DeviceArray(ctx, q * k, np.uint64)
        times, results, found = {f: [] for f in forms}, {}, {}
        for r in range(args.warmup + args.runs):
            for form in forms:
                if form != "plain" or len(forms) > 1:
                    ctx.set_option("dict_find.staged", 1 if form == "staged" else 0)
                ctx.profile_region(True)
                _, _, found[form] = ctx.dict_find_flat(dicts, d_blob, d_off, d_flags, II2_DEVICE, d_first, d_end)
                ctx.profile_region(False)
                if r >= args.warmup:
                    times[form].append(ctx.profile_region_ms() * 1e3)
                elif r == 0:
                    results[form] = (d_first.download(), d_end.download())
        for form in forms[1:]:
            assert found[form] == found["plain"] and all((a == b).all() for a, b in zip(results[form], results["plain"]))
        assert prefix or found["plain"] >= q - q // 2
        row = {"part": "kernel", "k": k, "terms_per_dict": args.terms, "probes": q, "prefix": prefix, "pairs": q * k, "n_found": found["plain"]}
        row.update({form: summary(times[form]) for form in forms})
        emit(row)
        for a in (d_blob, d_off, d_flags, d_first, d_end):
            a.free()
    for d in dicts:
        d.free()


def part_mirror(ctx):
    n, segs = args.mirror_terms, 8
    # one shard: every term starts with the same two bytes (the shard key is the first two bytes >> 6)
    vocab = sorted({b"te" + t for t in synth.random_terms(2 * n, seed=13)})
    index = host.InvertedIndex(ctx)
    rng = np.random.default_rng(14)
    for s in range(segs):      # a segment holds a random half of the vocabulary: 10 terms per doc
        mine = [vocab[int(i)] for i in rng.choice(len(vocab), n, replace=False)]
        index.put_batch([(mine[d:d + 10], s * 100_000 + d // 10) for d in range(0, n, 10)])
    assert index.n_shards == 1 and index.n_segments == segs
    absent = [b"te" + t for t in synth.random_terms(4096, seed=15)]
    lib, h = index.lib, index.h
    for q in [int(x) for x in args.qs.split(",")]:
        queries = [[absent[int(rng.integers(0, len(absent)))] if rng.random() < 0.1 else vocab[int(rng.integers(0, len(vocab)))] for _ in range(3)]
                   for _ in range(q)]
        blob, off = pack([t for terms in queries for t in terms])
        q_first = (np.arange(q + 1) * 3).astype(np.uint64)
        q_req = np.full(q, 3, np.uint64)
        distinct = len({t for terms in queries for t in terms})
        n_out = C.c_uint64()

        def call():
            t0 = time.perf_counter()
            rc = lib.ii2h_intersect_batch(h, blob.ctypes.data, off.ctypes.data, q_first.ctypes.data, q_req.ctypes.data, q, C.byref(n_out))
            dt = time.perf_counter() - t0
            assert rc == 0, rc
            return dt * 1e6

        modes = tuple(int(m) for m in args.modes.split(",")) if have_switch else (None,)
        times, sizes = {m: [] for m in modes}, {}
        for r in range(args.warmup + args.runs):
            for m in modes:
                if m is not None:
                    index.set_resolve(m)
                dt = call()
                sizes[m] = sum(len(v) for _, v in index._results(n_out.value))
                if r >= args.warmup:
                    times[m].append(dt)
        assert len(set(sizes.values())) == 1
        row = {"part": "mirror", "segments": segs, "terms_per_segment": n, "queries": q, "terms_per_query": 3, "distinct_terms": distinct,
               "pairs": distinct * segs, "result_ids": sizes[modes[0]]}
        for m in modes:
            row["parent" if m is None else "mode%d" % m] = summary(times[m])
        emit(row)
    index.close()


ctx = Context(0)
if "kernel" in PARTS and not args.libdir:
    part_kernel(ctx)
if "mirror" in PARTS:
    part_mirror(ctx)
