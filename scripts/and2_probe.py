"""C2 (2-term AND over 100M docs) through the two dense paths: intersect.and2 = 1 (intersect_and2.hip) against 0 (the n-list
streaming kernel), device time per pass from an event pair around a run of back-to-back passes, result checked against numpy
once.  Extra arguments `name=value` are set as options first; `stamps` prints the per-phase cycle shares of the and2 kernels;
`words` times the one-launch form with intersect.and2_words = 0 (the shorter list's blocks against the longer list's dense form)
and = 2 (both lists' dense forms ANDed word by word, intersect_words.hip) in this one process, alternating, and the first query
of the pair - the one that builds the forms - before that; then the word kernel's instances against each other, alternating as
well: intersect.and2_words_order (0 both chunks staged before the first store, 1 chunk 0's stores first) x
intersect.and2_words_store (0 plain, 1 write-through).  With `stamps` too,
every instance's phase table and, beside it, the pass time less the mean life of a wave (CYCLES_PER_US cycles of the stamps'
clock to the microsecond)."""
import time
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C

import numpy as np

from inverted_index_2_amd import Context, synth

D = int(os.environ.get("D", 100_000_000))
CYCLES_PER_US = 2330.0          # the stamps' clock against the event clock (profiles/and2_words_stamps.txt)
INSTANCES = [(o, st) for st in (0, 1) for o in (0, 1)]        # (and2_words_order, and2_words_store)
ctx = Context(0)
want_stamps = want_words = False
for kv in sys.argv[1:]:
    if kv in ("stamps", "words"):
        want_stamps, want_words = want_stamps or kv == "stamps", want_words or kv == "words"
        continue
    k, v = kv.split("=")
    ctx.set_option(k, int(v))
a, b = synth.zipf_list(2, D), synth.zipf_list(3, D)
want = np.intersect1d(a, b, assume_unique=True)
seg = ctx.encode_lists([a, b])
out = ctx.empty(min(a.size, b.size) + 512)
dcnt = ctx.empty(8, np.uint64)
lists = [(seg, 0), (seg, 1)]
removed = synth.geometric_postings(0.01, D, synth.term_seed(10**6))
tomb = ctx.tombstones(removed)
want_t = np.setdiff1d(want, removed, assume_unique=True)


def timed(tb, steps=50, warm=10):
    for _ in range(warm):
        ctx.intersect_async(lists, tb, out, dcnt)
    ctx.sync()
    ctx.profile_region(True)
    for _ in range(steps):
        ctx.intersect_async(lists, tb, out, dcnt)
    ctx.profile_region(False)
    ctx.sync()
    return ctx.profile_region_ms() * 1e3 / steps


if want_words:
    for w in (0, 2):                    # the first query on the pair: w = 0 builds the longer list's form, w = 2 the shorter one's as well
        ctx.set_option("intersect.and2_words", w)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.intersect_async(lists, None, out, dcnt)
        ctx.sync()
        print(f"and2_words={w} first query {(time.perf_counter() - t0) * 1e6:9.1f} us (host clock, forms built: {seg.dense_form_bytes()} bytes held)", flush=True)
    for w in (0, 2, 0, 2):
        ctx.set_option("intersect.and2_words", w)
        for tb, wnt, name in ((None, want, "plain"), (tomb, want_t, "tombstones")):
            ctx.intersect_async(lists, tb, out, dcnt)
            ctx.sync()
            n = int(dcnt.download(1)[0])
            ok = n == wnt.size and np.array_equal(out.download(n), wnt)
            print(f"and2_words={w} {name:10s} ok={ok} n={n} {timed(tb):8.2f} us per pass", flush=True)
    ctx.set_option("intersect.and2_words", 2)
    pass_us = {}
    for _ in range(3):
        for o, st in INSTANCES:
            ctx.set_option("intersect.and2_words_order", o)
            ctx.set_option("intersect.and2_words_store", st)
            for tb, wnt, name in ((None, want, "plain"), (tomb, want_t, "tombstones")):
                out.upload(np.zeros(16, np.uint32))
                ctx.intersect_async(lists, tb, out, dcnt)
                ctx.sync()
                n = int(dcnt.download(1)[0])
                ok = n == wnt.size and np.array_equal(out.download(n), wnt)
                us = timed(tb)
                pass_us.setdefault((o, st, name), []).append(us)
                print(f"order={o} store={st} {name:10s} ok={ok} n={n} {us:8.2f} us per pass", flush=True)
    ctx.set_option("intersect.and2_words_order", 0)
    ctx.set_option("intersect.and2_words_store", 1)
    ctx.set_option("intersect.and2_words", 1)

for and2 in (() if want_words else (1, 2, 0, 1)):
    ctx.set_option("intersect.and2", and2)
    for tb, w, name in ((None, want, "plain"), (tomb, want_t, "tombstones")):
        ctx.intersect_async(lists, tb, out, dcnt)
        ctx.sync()
        n = int(dcnt.download(1)[0])
        ok = n == w.size and np.array_equal(out.download(n), w)
        us = timed(tb)
        print(f"and2={and2} {name:10s} ok={ok} n={n} {us:8.2f} us per pass", flush=True)

if want_stamps:
    ctx.set_option("intersect.and2", 1)
    # (with A's dense form - intersect.dense_form=0 turns it off - phase 1 is the requests and phase 2 the form's words into LDS;
    # at two tiles a wave - intersect.and2_tiles=1 turns that off - a row is a workgroup of half the grid and every phase is the
    # sum over both tiles: the entries and the requests happen once, the landing, test, stage and flush once per tile)
    # (the word-by-word instance - intersect_words.hip - has seven phases of its own and a row per workgroup of 2048 words)
    names = {0: ["prologue", "clear+fetch", "mark A", "tomb+test B", "count+publish", "stage", "look-back", "flush"],
             2: ["requests", "landing+count+publish", "stage, first rounds", "look-back", "flush c0", "stage c1", "flush c1"]}
    # with `words` both instances, each forced; else the one the options in force give
    for w in ((0, 2) if want_words else (None,)):
        if w is not None:
            ctx.set_option("intersect.and2_words", w)
        ctx.set_option("debug.stamps", 1)
        ctx.intersect_async(lists, None, out, dcnt)
        ctx.sync()
        buf = (C.c_uint64 * (2048 * 8))()
        ctx._ck(ctx.lib.ii2_debug_read(ctx.h, buf, 2048 * 8))
        ctx.set_option("debug.stamps", 0)
        if w is None:                   # the word AND ran if, and only if, the options in force gave the shorter list a form
            w = 2 if seg.dense_form(0 if a.size <= b.size else 1, words=False) is not None else 0
        arr = np.frombuffer(buf, dtype=np.uint64).reshape(-1, 8).astype(np.float64)
        arr = arr[arr.sum(axis=1) > 0]
        tot = arr.sum(axis=1).mean() / 4
        print("and2_words", w, "rows", arr.shape[0], "mean cycles per wave", tot)
        for i, nm in enumerate(names[w]):
            print(f"    {nm:22s} {arr[:, i].mean() / 4:10.0f}  {100 * arr[:, i].mean() / 4 / tot:5.1f}%")
    for o, st in (INSTANCES if want_words else ()):
        ctx.set_option("intersect.and2_words", 2)
        ctx.set_option("intersect.and2_words_order", o)
        ctx.set_option("intersect.and2_words_store", st)
        ctx.set_option("debug.stamps", 1)
        ctx.intersect_async(lists, None, out, dcnt)
        ctx.sync()
        buf = (C.c_uint64 * (2048 * 8))()
        ctx._ck(ctx.lib.ii2_debug_read(ctx.h, buf, 2048 * 8))
        ctx.set_option("debug.stamps", 0)
        arr = np.frombuffer(buf, dtype=np.uint64).reshape(-1, 8).astype(np.float64)
        arr = arr[arr.sum(axis=1) > 0]
        tot = arr.sum(axis=1).mean() / 4
        us = float(np.median(pass_us[(o, st, "plain")]))
        print(f"order={o} store={st} rows {arr.shape[0]} mean cycles per wave {tot:.0f} = {tot / CYCLES_PER_US:.2f} us of life; "
              f"pass {us:.2f} us (median of {len(pass_us[(o, st, 'plain')])}); pass - life {us - tot / CYCLES_PER_US:.2f} us")
        for i, nm in enumerate(names[2]):
            print(f"    {nm:22s} {arr[:, i].mean() / 4:10.0f}  {100 * arr[:, i].mean() / 4 / tot:5.1f}%")
    if want_words:
        ctx.set_option("intersect.and2_words_order", 0)
        ctx.set_option("intersect.and2_words_store", 1)
        ctx.set_option("intersect.and2_words", 1)
