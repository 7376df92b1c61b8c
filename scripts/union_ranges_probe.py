"""ii2_union_ranges timings (device time from HIP events on the context stream, cold = first call, warm = mean of the next N):
  (a) the union of every list of a C3-scale segment (1M lists, sizes ~ 1/rank, mean 62.5 postings = one of C3's 16 segments,
      100M docs) next to ii2_seg_decode of the same segment (the same payload read: the floor), and the same union with the
      mark kernel's atomics left out (option debug.union_many_no_atomics: timing only, results wrong);
  (b) a range of 20 000 of its lists;
  (c) a prefix of ~1 000 short lists spread over 200 small segments;
  (d) PrefixSearch wall time through the host mirror for a prefix of ~1 000 terms in 200 Put segments.
Run plain for the times and under `rocprofv3 --kernel-trace --stats -- python scripts/union_ranges_probe.py` for per-kernel time."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inverted_index_2_amd import Context  # noqa: E402
from inverted_index_2_amd._lib import II2_DEVICE  # noqa: E402

N = int(os.environ.get("PROBE_N", "10"))


def zipf_segment(ctx, rng, T, mean, D):
    w = 1.0 / np.arange(1, T + 1)
    sizes = np.maximum(1, np.floor(w * (mean * T / w.sum()))).astype(np.int64)
    key = (np.repeat(np.arange(T, dtype=np.uint64), sizes) << np.uint64(32)) | rng.integers(0, D, int(sizes.sum())).astype(np.uint64)
    key = np.unique(key)
    term = (key >> np.uint64(32)).astype(np.int64)
    off = np.zeros(T + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(term, minlength=T))
    return ctx.encode(off, (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)), off


def timed(ctx, fn):
    ctx.profile_region(True)
    fn()
    ctx.profile_region(False)
    cold = ctx.profile_region_ms() * 1e3
    ctx.profile_region(True)
    for _ in range(N):
        fn()
    ctx.profile_region(False)
    return {"cold_us": round(cold, 1), "warm_us": round(ctx.profile_region_ms() * 1e3 / N, 1)}


def main():
    ctx = Context(0)
    rng = np.random.default_rng(1)
    res = {}
    T, D = 1_000_000, 100_000_000
    seg, off = zipf_segment(ctx, rng, T, 62.5, D)
    n_post = int(off[-1])
    res["segment"] = {"lists": T, "postings": n_post, "blocks": int(seg.info.n_blocks), "payload_bytes": int(seg.info.n_bytes)}
    d_off, d_vals = ctx.empty(T + 1, np.uint64), ctx.empty(n_post)
    res["a_decode"] = timed(ctx, lambda: ctx._ck(ctx.lib.ii2_seg_decode(ctx.h, seg.h, d_off.ptr, d_vals.ptr, II2_DEVICE)))
    out = ctx.empty(seg.info.n_blocks * 256)
    cnt = [0]

    def all_lists():
        cnt[0] = ctx.union_ranges([(seg, 0, T)], out=out)[1]
    res["a_union_all"] = timed(ctx, all_lists)
    res["a_union_all"]["ids"] = cnt[0]
    want = np.unique(d_vals.download(n_post))
    res["a_union_all"]["correct"] = bool(cnt[0] == want.size and np.array_equal(out.download(cnt[0]), want))
    ctx.set_option("debug.union_many_no_atomics", 1)
    res["a_union_all_no_atomics"] = timed(ctx, all_lists)
    ctx.set_option("debug.union_many_no_atomics", 0)
    all_lists()                                          # (the experiment left no bit set; one real call to be sure)

    def range20k():
        cnt[0] = ctx.union_ranges([(seg, 1000, 21000)], out=out)[1]
    res["b_range_20000"] = timed(ctx, range20k)
    res["b_range_20000"]["ids"] = cnt[0]
    # (c) 200 small segments of 5 short lists each
    small = [ctx.encode_lists([np.unique(rng.integers(0, 1_000_000, int(rng.integers(1, 40)))).astype(np.uint32) for _ in range(5)])
             for _ in range(200)]
    ranges = [(s, 0, 5) for s in small]
    out_c = ctx.empty(200 * 5 * 256)

    def prefix_lists():
        cnt[0] = ctx.union_ranges(ranges, out=out_c)[1]
    res["c_1000_short_lists"] = timed(ctx, prefix_lists)
    res["c_1000_short_lists"]["ids"] = cnt[0]
    # (d) the host mirror: 200 Puts of 5 terms each from 1000 terms of one prefix (one shard)
    from inverted_index_2_amd.host import InvertedIndex
    ii = InvertedIndex(ctx)
    vocab = [b"a" + b"%04d" % i for i in range(1000)]
    for v in range(200):
        ii.put([vocab[i] for i in rng.choice(1000, 5, replace=False)], v)
    ii.prefix_search([b"a"])
    t0 = time.perf_counter()
    for _ in range(N):
        r = ii.prefix_search([b"a"])
    res["d_prefix_search_wall_us"] = round((time.perf_counter() - t0) / N * 1e6, 1)
    res["d_ids"] = len(r[b"a"])
    ii.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
