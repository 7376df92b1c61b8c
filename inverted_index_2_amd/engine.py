"""Thin Python host layer over the C ABI (include/ii2.h): contexts, device segments,
tombstones and the three hot-path operators.  numpy arrays are host buffers; DeviceArray
(or any object with .data_ptr(), e.g. a torch CUDA tensor) is a device buffer.

Nothing here computes postings on the CPU — every operator is a call into libii2_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import II2_FUZZY_TRANSPOSE, II2_MATCH_UTF8, FuzzyStats  # noqa: F401
from ._lib import RegexStats
from ._lib import II2_DEVICE, II2_HOST, II2_MATCH_CONTAINS, II2_MATCH_GLOB, II2_MATCH_NOCASE, II2_MATCH_SUFFIX, II2_OP_AND, II2_OP_OR, AtleastStats, BuildStats, CountStats, DictBuildStats, ExplainBatchStats, ExplainStats, HistStats, MatchStats, MergeStats, SegInfo, TopkBatchStats, TopkStats, TopkwStats

SKIP_DTYPE = np.dtype([("first_doc", "<u4"), ("byte_off", "<u4")])


class II2Error(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ii2 error {code} ({_lib.ERRORS.get(code, '?')}): {msg}")
        self.code = code


def _np(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a) -> C.c_void_p:
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    if isinstance(a, int):
        return C.c_void_p(a)
    raise TypeError(type(a))


def _flat(byte_strings):
    """(blob, off) of a list of bytes as the ABI takes them: u8 bytes, padded by one so that the array is never empty, and u64
    offsets [n + 1] from 0."""
    off = np.zeros(len(byte_strings) + 1, np.uint64)
    if byte_strings:
        off[1:] = np.cumsum([len(t) for t in byte_strings])
    return np.frombuffer(b"".join(byte_strings) + b"\0", dtype=np.uint8).copy(), off


def _flat_dicts(dictionaries):
    """(flat, blob, off, first) of k dictionaries (lists of bytes): all their terms in one list, those flattened (_flat), and
    the u64 first term of each dictionary [k + 1]."""
    flat = [t for d in dictionaries for t in d]
    first = np.zeros(len(dictionaries) + 1, np.uint64)
    first[1:] = np.cumsum([len(d) for d in dictionaries])
    return (flat, *_flat(flat), first)


def _per_pattern(v, n, who, what):
    """A per-pattern u8 argument of `who`: one value for all the n patterns (a Python or numpy integer) or one per pattern;
    `what` names it in the error, as in "kind per pattern"."""
    a = np.full(n, int(v), np.uint8) if isinstance(v, (int, np.integer)) else _np(v, np.uint8)
    if a.size != n:
        raise ValueError(f"{who}: one {what}")
    return a


_BATCH_OPS = {"and": II2_OP_AND, "or": II2_OP_OR}


def pack_batch(queries):
    """The flat arrays ii2_query_batch takes, from queries = [("and" | "or", [(segment, first, end), ...]), ...]: (op u8 [Q],
    query_first u64 [Q + 1], segments [R], list_first u64 [R], list_end u64 [R]) with R ranges in all; query q owns the ranges
    query_first[q] .. query_first[q + 1] - 1.  Pure host code: the segments are passed through as they are."""
    op = np.zeros(len(queries), np.uint8)
    query_first = np.zeros(len(queries) + 1, np.uint64)
    segs, first, end = [], [], []
    for q, (name, ranges) in enumerate(queries):
        key = name.lower() if isinstance(name, str) else name
        if key not in _BATCH_OPS:
            raise ValueError(f"query {q}: unknown op {name!r} (\"and\" or \"or\")")
        op[q] = _BATCH_OPS[key]
        for s, a, b in ranges:
            a, b = int(a), int(b)
            if a < 0 or b < 0:
                raise ValueError(f"query {q}: negative list index")
            segs.append(s)
            first.append(a)
            end.append(b)
        query_first[q + 1] = len(segs)
    return op, query_first, segs, np.array(first, np.uint64), np.array(end, np.uint64)


def pack_andnot(groups, exclude):
    """The flat arrays ii2_andnot_ranges takes, from groups / exclude = [[(segment, first, end), ...], ...]: (group_first u64
    [G + 1], group_not u8 [G], segments [R], list_first u64 [R], list_end u64 [R]) - the required groups first (flags 0), then the
    excluded ones (flags 1); group g owns the ranges group_first[g] .. group_first[g + 1] - 1.  Pure host code: the segments are
    passed through as they are."""
    groups, exclude = list(groups), list(exclude)
    n = len(groups) + len(exclude)
    group_first = np.zeros(n + 1, np.uint64)
    group_not = np.zeros(n, np.uint8)
    group_not[len(groups):] = 1
    segs, first, end = [], [], []
    for g, ranges in enumerate(groups + exclude):
        for s, a, b in ranges:
            a, b = int(a), int(b)
            if a < 0 or b < 0:
                raise ValueError(f"group {g}: negative list index")
            segs.append(s)
            first.append(a)
            end.append(b)
        group_first[g + 1] = len(segs)
    return group_first, group_not, segs, np.array(first, np.uint64), np.array(end, np.uint64)


def pack_group_batch(queries):
    """The flat arrays ii2_query_batch_groups takes, from queries = [(groups, exclude), ...] with groups / exclude = [[(segment,
    first, end), ...], ...] as pack_andnot takes them: (query_first u64 [Q + 1], group_first u64 [G + 1], group_not u8 [G],
    segments [R], list_first u64 [R], list_end u64 [R]) - within every query the required groups first (flags 0), then the
    excluded ones (flags 1); query q owns the groups query_first[q] .. query_first[q + 1] - 1, group g the ranges
    group_first[g] .. group_first[g + 1] - 1.  Pure host code: the segments are passed through as they are."""
    query_first = np.zeros(len(queries) + 1, np.uint64)
    group_first, group_not = [0], []
    segs, first, end = [], [], []
    for q, (groups, exclude) in enumerate(queries):
        groups, exclude = list(groups), list(exclude)
        for g, ranges in enumerate(groups + exclude):
            for s, a, b in ranges:
                a, b = int(a), int(b)
                if a < 0 or b < 0:
                    raise ValueError(f"query {q}: group {g}: negative list index")
                segs.append(s)
                first.append(a)
                end.append(b)
            group_first.append(len(segs))
            group_not.append(0 if g < len(groups) else 1)
        query_first[q + 1] = len(group_not)
    return (query_first, np.array(group_first, np.uint64), np.array(group_not, np.uint8), segs, np.array(first, np.uint64),
            np.array(end, np.uint64))


def pack_topk_batch(queries):
    """The flat arrays ii2_topk_batch takes, from queries = [(groups, weights | None, k, min_score, exclude), ...] with groups /
    exclude as pack_andnot takes them and one weight per group of `groups`: pack_group_batch's six arrays for [(groups, exclude),
    ...], then (group_weight u32 [G] - None when no query has weights, else 1 for the groups of a query without and for every
    excluded group, whose entry the library ignores -, min_score u32 [Q], k u32 [Q]).  Pure host code."""
    packed = pack_group_batch([(groups, exclude) for groups, _, _, _, exclude in queries])
    weight = []
    for q, (groups, weights, _, _, exclude) in enumerate(queries):
        groups = list(groups)
        if weights is not None and len(weights) != len(groups):
            raise ValueError(f"query {q}: one weight per group")
        weight += [int(w) for w in weights] if weights is not None else [1] * len(groups)
        weight += [1] * len(list(exclude))
    group_weight = None if all(w is None for _, w, _, _, _ in queries) else np.array(weight, np.uint32)
    return packed + (group_weight, np.array([int(m) for _, _, _, m, _ in queries], np.uint32), np.array([int(k) for _, _, k, _, _ in queries], np.uint32))


def pack_explain_batch(queries):
    """The flat arrays ii2_explain_batch takes, from queries = [groups, ...] with groups = [[(segment, first, end), ...], ...] as
    explain_ranges takes them: (query_first u64 [Q + 1], group_first u64 [G + 1], segments [R], list_first u64 [R], list_end u64
    [R]) - pack_group_batch's arrays without the flags: an excluded group is one more group.  Pure host code."""
    query_first, group_first, _, segs, first, end = pack_group_batch([(groups, []) for groups in queries])
    return query_first, group_first, segs, first, end


def explain_batch_plan(n_lists: int, n_postings: int, n_blocks: int, n_ids: int, batch_explain: int = 1, batch_tiny: int = 1) -> int:
    """The form ii2_explain_batch's planner gives a query of n_lists non-empty lists that hold n_postings postings in n_blocks
    blocks, with n_ids ids, under the two option values (ii2_explain_batch_plan): one of II2_EXPLAIN_BATCH_EMPTY / TINY / SMALL /
    SINGLE.  Needs no context and no GPU."""
    lib = _lib.load()
    form = C.c_uint32(0)
    rc = lib.ii2_explain_batch_plan(int(n_lists), int(n_postings), int(n_blocks), int(n_ids), int(batch_explain), int(batch_tiny), C.byref(form))
    if rc != 0:
        raise II2Error(rc, "ii2_explain_batch_plan")
    return form.value


def path_names():
    """The names of the kernel paths the library counts (ii2_path_name), in id order.  Needs no context and no GPU."""
    lib = _lib.load()
    names = []
    while True:
        name = lib.ii2_path_name(len(names))
        if name is None:
            return names
        names.append(name.decode())


def merge_event_names():
    """The names of the events the merge tile kernel counts (ii2_merge_event_name), in id order.  Needs no context and no GPU."""
    lib = _lib.load()
    names = []
    while True:
        name = lib.ii2_merge_event_name(len(names))
        if name is None:
            return names
        names.append(name.decode())


def term_match(kind: int, pattern: bytes, term: bytes) -> bool:
    """One pattern against one term by the functions ii2_dict_match's kernel runs (ii2_term_match).  kind: II2_MATCH_CONTAINS /
    SUFFIX / GLOB, optionally | II2_MATCH_NOCASE and / or II2_MATCH_UTF8 (the glob's `?` and `*` take whole UTF-8 symbols of the
    term; the pattern must be well-formed UTF-8).  Needs no context and no GPU."""
    lib = _lib.load()
    m = C.c_int(-1)
    rc = lib.ii2_term_match(int(kind), C.c_char_p(bytes(pattern)) if pattern else None, len(pattern), C.c_char_p(bytes(term)) if term else None,
                            len(term), C.byref(m))
    if rc:
        raise II2Error(rc, "ii2_term_match")
    return bool(m.value)


def term_fuzzy(pattern: bytes, term: bytes, max_dist: int, prefix: int = 0, flags: int = 0):
    """One pattern against one term by the functions ii2_dict_fuzzy's kernel runs (ii2_term_fuzzy): (match, dist) - whether the
    term shares the pattern's first `prefix` bytes and lies within `max_dist` edits, and the exact distance whatever those two
    are.  flags: 0, II2_FUZZY_TRANSPOSE, II2_MATCH_NOCASE and / or II2_MATCH_UTF8 - then prefix and distance count UTF-8 symbols
    (a code point, or one ill-formed byte of the term), and the pattern must be well-formed UTF-8.  Needs no context and no GPU."""
    lib = _lib.load()
    m, d = C.c_int(-1), C.c_uint32(0)
    rc = lib.ii2_term_fuzzy(int(flags), C.c_char_p(bytes(pattern)) if pattern else None, len(pattern), int(prefix), int(max_dist),
                            C.c_char_p(bytes(term)) if term else None, len(term), C.byref(m), C.byref(d))
    if rc:
        raise II2Error(rc, "ii2_term_fuzzy")
    return bool(m.value), d.value


def utf8_decode(data: bytes):
    """The symbols of a byte string by the decoder the kernels run under II2_MATCH_UTF8 (ii2_utf8_decode): (symbols, well_formed).
    A well-formed sequence is its code point, any other byte b alone is 0xDC00 + b - bytes.decode("utf-8", "surrogateescape").
    Needs no context and no GPU."""
    lib = _lib.load()
    data = bytes(data)
    n, ok = C.c_uint64(0), C.c_int(-1)
    out = (C.c_uint32 * max(len(data), 1))()
    rc = lib.ii2_utf8_decode(C.c_char_p(data) if data else None, len(data), out, len(data), C.byref(n), C.byref(ok))
    if rc:
        raise II2Error(rc, "ii2_utf8_decode")
    return list(out[:n.value]), bool(ok.value)


def term_regex(pattern: bytes, term: bytes, flags: int = 0):
    """One pattern against one term by the functions ii2_dict_regex's kernel runs (ii2_term_regex): (match, n_pos) - whether the
    regular expression matches the WHOLE term, and the positions of its automaton (at most 64).  flags: 0 or II2_MATCH_NOCASE.
    A pattern outside the syntax or above a limit raises II2Error; on the position limit its n_pos attribute holds the count
    that was too large.  Needs no context and no GPU."""
    lib = _lib.load()
    m, n = C.c_int(-1), C.c_uint32(0)
    rc = lib.ii2_term_regex(int(flags), C.c_char_p(bytes(pattern)) if pattern else None, len(pattern), C.c_char_p(bytes(term)) if term else None,
                            len(term), C.byref(m), C.byref(n))
    if rc:
        e = II2Error(rc, "ii2_term_regex")
        e.n_pos = n.value
        raise e
    return bool(m.value), n.value


def explain_slot(id: int, log2_slots: int) -> int:
    """The slot an id's probe starts at in ii2_explain_ranges' id -> row table of 1 << log2_slots entries, by the function the
    kernels run (ii2_explain_slot).  Needs no context and no GPU."""
    lib = _lib.load()
    slot = C.c_uint32(0)
    rc = lib.ii2_explain_slot(int(id), int(log2_slots), C.byref(slot))
    if rc:
        raise II2Error(rc, "ii2_explain_slot")
    return slot.value


def _edges(edges):
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.uint64).ravel())
    return e, max(int(e.size) - 1, 0)


def hist_bucket(edges, id: int) -> int:
    """The bucket of an id on a histogram axis, -1 outside it, by the function the histogram kernels run (ii2_hist_bucket): edges
    = n_buckets + 1 strictly ascending values <= 2^32, bucket b = [edges[b], edges[b + 1]).  Needs no context and no GPU."""
    e, nb = _edges(edges)
    b = C.c_int64(0)
    rc = _lib.load().ii2_hist_bucket(e.ctypes.data_as(_lib.u64p) if e.size else None, nb, int(id), C.byref(b))
    if rc:
        raise II2Error(rc, "ii2_hist_bucket")
    return b.value


def hist_block(edges, first_doc: int, up: int):
    """What a block with the doc bounds [first_doc, up] is to a histogram axis (ii2_hist_block): (kind, b_lo, b_hi), kind one of
    II2_HIST_SKIP / WHOLE / SPLIT / WIDE.  Needs no context and no GPU."""
    e, nb = _edges(edges)
    kind, lo, hi = C.c_int(-1), C.c_uint32(0), C.c_uint32(0)
    rc = _lib.load().ii2_hist_block(e.ctypes.data_as(_lib.u64p) if e.size else None, nb, int(first_doc), int(up), C.byref(kind), C.byref(lo), C.byref(hi))
    if rc:
        raise II2Error(rc, "ii2_hist_block")
    return kind.value, lo.value, hi.value


class DeviceArray:
    """A raw HBM buffer owned by a Context."""

    def __init__(self, ctx: "Context", count: int, dtype=np.uint32):
        self.ctx, self.count, self.dtype = ctx, int(count), np.dtype(dtype)
        p = C.c_void_p()
        ctx._ck(ctx.lib.ii2_dev_alloc(ctx.h, max(self.nbytes, 16), C.byref(p)))
        self.ptr = p.value

    @property
    def nbytes(self) -> int:
        return self.count * self.dtype.itemsize

    def data_ptr(self) -> int:
        return self.ptr

    def upload(self, host) -> "DeviceArray":
        a = _np(host, self.dtype)
        assert a.size <= self.count
        if a.size:
            self.ctx._ck(self.ctx.lib.ii2_copy_h2d(self.ctx.h, self.ptr, _ptr(a), a.nbytes))
        return self

    def download(self, count: Optional[int] = None) -> np.ndarray:
        n = self.count if count is None else int(count)
        out = np.empty(n, self.dtype)
        if n:
            self.ctx._ck(self.ctx.lib.ii2_copy_d2h(self.ctx.h, _ptr(out), self.ptr, out.nbytes))
        return out

    def free(self) -> None:
        if self.ptr:
            self.ctx.lib.ii2_dev_free(self.ctx.h, self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            if not sys.is_finalizing():      # at interpreter exit the HIP runtime may already be gone
                self.free()
        except Exception:
            pass


class Context:
    """One GPU + one HIP stream (ii2_ctx)."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = C.c_void_p()
        rc = self.lib.ii2_ctx_create(device, 0, C.byref(h))
        if rc:
            raise II2Error(rc, (self.lib.ii2_last_error(None) or b"").decode())
        self.h = h
        self.device = device
        # experiments: II2_OPTIONS="name=value,name=value" sets options on every context of the process (scripts, bench runs)
        for kv in filter(None, os.environ.get("II2_OPTIONS", "").split(",")):
            name, _, value = kv.partition("=")
            self.set_option(name.strip(), int(value))

    def _ck(self, rc: int) -> None:
        if rc:
            raise II2Error(rc, (self.lib.ii2_last_error(self.h) or b"").decode())

    def close(self) -> None:
        if self.h:
            self.lib.ii2_ctx_destroy(self.h)
            self.h = None

    def sync(self) -> None:
        self._ck(self.lib.ii2_ctx_sync(self.h))

    @property
    def stream(self) -> int:
        return self.lib.ii2_ctx_stream(self.h) or 0

    def set_option(self, name: str, value: int) -> None:
        self._ck(self.lib.ii2_set_option(self.h, name.encode(), int(value)))

    def counters(self):
        """(merges repeated on the packing path, look-back launches repeated on their second path, host waits inside the exchange
        entry points, stream waits the per-device order of look-back launches put in front of this context's) - see
        ii2_ctx_counters."""
        out = (C.c_uint64 * 4)()
        self._ck(self.lib.ii2_ctx_counters(self.h, out, 4))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def paths(self):
        """{path name: how often this context took that kernel path since it was created} (ii2_ctx_paths; the names come from
        ii2_path_name).  The difference between two reads is what the calls in between launched."""
        names = path_names()
        out = (C.c_uint64 * len(names))()
        n = self.lib.ii2_ctx_paths(self.h, out, len(names))
        if n != len(names):
            raise II2Error(-1, "ii2_ctx_paths: the library knows another number of paths than ii2_path_name")
        return {name: int(out[i]) for i, name in enumerate(names)}

    def merge_events(self):
        """{event name: how often the merge tile kernel left its ordinary path that way on this context since it was created}
        (ii2_merge_events; the names come from ii2_merge_event_name).  Counted on the device by every merge, the unions' merge
        passes included; the read waits for the context's stream.  The difference between two reads is what the calls in between
        met."""
        names = merge_event_names()
        out = (C.c_uint64 * len(names))()
        n = self.lib.ii2_merge_events(self.h, out, len(names))
        if n < 0:
            self._ck(n)
        if n != len(names):
            raise II2Error(-1, "ii2_merge_events: the library knows another number of events than ii2_merge_event_name")
        return {name: int(out[i]) for i, name in enumerate(names)}

    def lookback_check(self, n_wg: int, amount, spin: int, g_base: int = 0, seed_state=None, seed_value=None, delay=None):
        """The look-back protocol without a payload, on this context's records and epochs (ii2_lookback_check: a test and
        diagnostic facility).  amount: n_wg words; seed_state / seed_value: g_base + 2 * (g_base // 64) entries, the amounts of
        the workgroups before g_base and then {amount, inclusive prefix} of each group before it; delay: None or n_wg words.
        Returns a dict of arrays, one entry per launched workgroup: prefix (u64), state (0 or II2_LB_GAVE_UP_* bits), windows,
        dist (II2_LB_NO_PREFIX: none), polls; the raw records agg / grp of the launched workgroups and groups; and the words
        epoch, err (the error word afterwards) and cap (workgroups the records hold)."""
        n_wg, g_base = int(n_wg), int(g_base)
        n, n_grp = max(n_wg - g_base, 0), max((n_wg + 63) // 64 - g_base // 64, 0)
        amount = _np(amount, np.uint64)
        if amount.size != n_wg:
            raise ValueError("one amount per workgroup of the logical grid")
        n_seed = g_base + 2 * (g_base // 64)
        if g_base:
            seed_state, seed_value = _np(seed_state, np.uint8), _np(seed_value, np.uint64)
            if seed_state.size != n_seed or seed_value.size != n_seed:
                raise ValueError("g_base + 2 * (g_base // 64) seeds")
        else:
            seed_state = seed_value = None
        if delay is not None:
            delay = _np(delay, np.uint16)
            if delay.size != n_wg:
                raise ValueError("one delay per workgroup of the logical grid")
        prefix, agg, grp = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(2 * n_grp, np.uint64)
        state, walk, polls = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        info = np.zeros(4, np.uint64)
        self._ck(self.lib.ii2_lookback_check(self.h, n_wg, g_base, _ptr(amount), int(spin), _ptr(seed_state), _ptr(seed_value), _ptr(delay),
                                             _ptr(prefix), _ptr(state), _ptr(walk), _ptr(polls), _ptr(agg), _ptr(grp), _ptr(info)))
        return dict(prefix=prefix, state=state, windows=walk & 0xFFFFFF, dist=walk >> 24, polls=polls, agg=agg, grp=grp,
                    epoch=int(info[0]), err=int(info[1]), cap=int(info[2]))

    def profile_read(self):
        """(total device ms, launches) of the dominant kernel since the last read (option profile.events)."""
        ms, n = C.c_double(), C.c_uint64()
        self._ck(self.lib.ii2_profile_read(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_region(self, begin: bool) -> None:
        """Record the start (begin=True) / end event of a region on the ctx stream."""
        self._ck(self.lib.ii2_profile_region(self.h, 1 if begin else 0))

    def profile_region_ms(self) -> float:
        ms = C.c_double()
        self._ck(self.lib.ii2_profile_region_ms(self.h, C.byref(ms)))
        return ms.value

    def selftest(self) -> None:
        self._ck(self.lib.ii2_selftest(self.h))

    def empty(self, count: int, dtype=np.uint32) -> DeviceArray:
        return DeviceArray(self, count, dtype)

    # ---- segments -------------------------------------------------------------------------
    def encode(self, post_off, values, where: int = II2_HOST) -> "Segment":
        """Encode step (Writer.Append -> intcomp.CompressUint32, file/writer.go:32-59)."""
        if where == II2_HOST:
            post_off = _np(post_off, np.uint64)
            values = _np(values, np.uint32)
            n_lists = post_off.size - 1
        else:
            n_lists = post_off.count - 1
        s = C.c_void_p()
        self._ck(self.lib.ii2_seg_encode(self.h, n_lists, _ptr(post_off), _ptr(values), where, C.byref(s)))
        return Segment(self, s)

    def encode_lists(self, lists: Sequence) -> "Segment":
        arrs = [_np(l, np.uint32) for l in lists]
        po = np.zeros(len(arrs) + 1, np.uint64)
        if arrs:
            po[1:] = np.cumsum([a.size for a in arrs])
        flat = np.concatenate(arrs) if arrs else np.empty(0, np.uint32)
        return self.encode(po, flat)

    def build_segment(self, list_ids, values, n_lists: int, where: int = II2_HOST):
        """Build step (ii2_seg_build): one segment of n_lists lists from (list id, value) pairs in any order, repeats allowed -
        the bulk form of Shard.Put (shard.go:33-67) and the merges that fold its segments (shard.go:163-212).  numpy arrays
        with where == II2_HOST, DeviceArrays with II2_DEVICE.  Returns (Segment, BuildStats)."""
        if where == II2_HOST:
            list_ids = _np(list_ids, np.uint32)
            values = _np(values, np.uint32)
            n = list_ids.size
            if values.size != n:
                raise ValueError("build_segment: list_ids and values differ in length")
        else:
            n = list_ids.count
            if values.count != n:
                raise ValueError("build_segment: list_ids and values differ in length")
        s, st = C.c_void_p(), BuildStats()
        self._ck(self.lib.ii2_seg_build(self.h, int(n_lists), n, _ptr(list_ids) if n else None, _ptr(values) if n else None, where,
                                        C.byref(s), C.byref(st)))
        return Segment(self, s), st

    def import_dv1(self, n_postings: int, blk_off, skip, payload) -> "Segment":
        blk_off = _np(blk_off, np.uint32)
        skip = _np(skip, SKIP_DTYPE)
        payload = _np(payload, np.uint8)
        s = C.c_void_p()
        if blk_off.size < 1 or skip.size < 1:
            raise ValueError("import_dv1: blk_off and skip hold at least their closing entry")
        self._ck(self.lib.ii2_seg_import(self.h, blk_off.size - 1, n_postings, skip.size - 1, payload.size, _ptr(blk_off), _ptr(skip),
                                         _ptr(payload) if payload.size else None, II2_HOST, C.byref(s)))
        return Segment(self, s)

    def tombstones(self, removed, where: int = II2_HOST) -> "Tombstones":
        """RemovedLists.Values() as a device bitmap (removed_list.go:44-54, shard.go:183)."""
        if where == II2_HOST:
            removed = _np(removed, np.uint32)
            n = removed.size
        else:
            n = removed.count
        t = C.c_void_p()
        self._ck(self.lib.ii2_tomb_create(self.h, _ptr(removed), n, where, C.byref(t)))
        return Tombstones(self, t)

    # ---- term alignment on the device -------------------------------------------------------
    def align_terms(self, dictionaries) -> "Alignment":
        """k sorted, duplicate-free term dictionaries (lists of bytes) -> their union, on the device (the k-way term walk of
        makeIterator, shard.go:253-278, in bytes.Compare order)."""
        flat, blob, off, first = _flat_dicts(dictionaries)
        h = C.c_void_p()
        self._ck(self.lib.ii2_align_terms(self.h, len(dictionaries), _ptr(blob), _ptr(off), _ptr(first), C.byref(h)))
        return Alignment(self, h, flat)

    def align_terms_flat(self, term_bytes: np.ndarray, term_off: np.ndarray, seg_first: np.ndarray) -> "Alignment":
        """Same, from flat arrays (u8 bytes, u64 offsets [n_all + 1], u64 first term of each dictionary [k + 1])."""
        blob, off, first = _np(term_bytes, np.uint8), _np(term_off, np.uint64), _np(seg_first, np.uint64)
        h = C.c_void_p()
        self._ck(self.lib.ii2_align_terms(self.h, first.size - 1, _ptr(blob), _ptr(off), _ptr(first), C.byref(h)))
        return Alignment(self, h, None)

    def dictionary(self, terms) -> "Dictionary":
        """A segment's sorted, duplicate-free term dictionary (list of bytes), made resident in HBM (ii2_dict_create)."""
        terms = list(terms)
        return self.dictionary_flat(*_flat(terms), terms)

    def dictionary_flat(self, term_bytes, term_off, terms=None) -> "Dictionary":
        """Same, from flat arrays: u8 bytes and u64 offsets [n + 1] starting at 0."""
        blob, off = _np(term_bytes, np.uint8), _np(term_off, np.uint64)
        h = C.c_void_p()
        self._ck(self.lib.ii2_dict_create(self.h, _ptr(blob), _ptr(off), off.size - 1, II2_HOST, C.byref(h)))
        return Dictionary(self, h, terms)

    def build_dictionary(self, terms, term_off=None, where: int = II2_HOST, want_ids: bool = True):
        """Dictionary build step (ii2_dict_build): terms in any order, repeats allowed -> the resident dictionary of the sorted,
        duplicate-free terms and every input term's index in it, sorted and deduplicated on the device.  `terms` is a list of
        bytes, or - with term_off, u64 [n + 1] from 0 - the flat u8 bytes: numpy arrays with where == II2_HOST, DeviceArrays
        with II2_DEVICE.  Returns (Dictionary, term_id, DictBuildStats): term_id is a u32 numpy array, or with II2_DEVICE a
        DeviceArray that ii2_seg_build takes as its list_id (None with want_ids=False)."""
        if term_off is None:
            terms, term_off = _flat(list(terms))
            where = II2_HOST
        if where == II2_HOST:
            terms, term_off = _np(terms, np.uint8), _np(term_off, np.uint64)
            n = term_off.size - 1
            ids = np.zeros(max(n, 1), np.uint32) if want_ids else None
        else:
            n = term_off.count - 1
            ids = DeviceArray(self, max(n, 1), np.uint32) if want_ids else None
        h, st = C.c_void_p(), DictBuildStats()
        self._ck(self.lib.ii2_dict_build(self.h, n, _ptr(terms) if n else None, _ptr(term_off) if n else None, where, C.byref(h),
                                         _ptr(ids) if ids is not None else None, C.byref(st)))
        if where == II2_HOST and ids is not None:
            ids = ids[:n]
        return Dictionary(self, h), ids, st

    def dict_find(self, dicts, terms, prefix=False):
        """Term and prefix lookup on the device (ii2_dict_find): every term of `terms` (bytes) in every one of the k resident
        dictionaries.  prefix: one flag for all the probes or one per probe - False: the term itself, [j, j + 1) where it is
        list j and the empty [j, j) at its insertion point where it is absent; True: the run of the terms that start with it.
        Returns (list_first, list_end, n_found): u64 arrays of shape (len(terms), k) and the number of non-empty ranges.  Row p,
        flattened with the k segments repeated, is one group of the range entry points."""
        terms = list(terms)
        blob, off = _flat(terms)
        flags = _per_pattern(bool(prefix) if isinstance(prefix, (int, np.integer)) else prefix, len(terms), "dict_find", "prefix flag per term")
        first, end, found = self.dict_find_flat(dicts, blob, off, flags, II2_HOST)
        return first.reshape(len(terms), len(dicts)), end.reshape(len(terms), len(dicts)), found

    def dict_find_flat(self, dicts, probe_bytes, probe_off, probe_prefix=None, where: int = II2_HOST, list_first=None, list_end=None):
        """The same from flat arrays, as the ABI takes them: numpy arrays with where == II2_HOST, DeviceArrays (the outputs
        included: list_first / list_end of n_probes * k u64 each) with II2_DEVICE.  Returns (list_first, list_end, n_found)."""
        arr = (C.c_void_p * len(dicts))(*[d.h for d in dicts])
        if where == II2_HOST:
            probe_bytes, probe_off = _np(probe_bytes, np.uint8), _np(probe_off, np.uint64)
            n = probe_off.size - 1
            if probe_prefix is not None:
                probe_prefix = _np(probe_prefix, np.uint8)
            list_first = np.zeros(max(n * len(dicts), 1), np.uint64)
            list_end = np.zeros(max(n * len(dicts), 1), np.uint64)
        else:
            n = probe_off.count - 1
        found = C.c_uint64()
        self._ck(self.lib.ii2_dict_find(self.h, len(dicts), arr, n, _ptr(probe_bytes), _ptr(probe_off), _ptr(probe_prefix), where,
                                        _ptr(list_first), _ptr(list_end), C.byref(found)))
        if where == II2_HOST:
            list_first, list_end = list_first[: n * len(dicts)], list_end[: n * len(dicts)]
        return list_first, list_end, found.value

    def dict_match(self, dicts, patterns, kind=II2_MATCH_CONTAINS):
        """Substring, suffix and wildcard term search on the device (ii2_dict_match): every pattern of `patterns` (bytes, at
        most 64 of at most 64 bytes) in every one of the k resident dictionaries.  kind: II2_MATCH_CONTAINS / SUFFIX / GLOB,
        optionally | II2_MATCH_NOCASE and / or II2_MATCH_UTF8 (`?` and `*` take whole UTF-8 symbols of the term) - one for all the
        patterns or one per pattern.  Returns (run_off, run_first, run_end,
        run_dict, stats): pair (p, s) owns the runs run_off[p * k + s] .. run_off[p * k + s + 1] - 1, run j is the terms
        [run_first[j], run_end[j]) of dictionary run_dict[j]; the runs of pattern p, run_off[p * k] .. run_off[(p + 1) * k] - 1,
        are one group of the range entry points.  A result that outgrows the first buffer takes a second call of the exact size."""
        patterns = list(patterns)
        kinds = _per_pattern(kind, len(patterns), "dict_match", "kind per pattern")
        blob, off = _flat(patterns)
        return self._dict_runs(dicts, len(patterns), lambda *out: self.dict_match_flat(dicts, blob, off, kinds, *out))

    def _dict_runs(self, dicts, n_patterns, flat_call):
        """The two-call protocol of dict_match, dict_fuzzy and dict_regex: flat_call(run_off, run_first, run_end, run_dict, cap) -> (return
        code, stats) with a first buffer of 4096 runs, and where the result outgrows it once more with the exact size."""
        run_off = np.zeros(n_patterns * len(dicts) + 1, np.uint64)
        cap = 4096
        while True:
            first, end, which = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint32)
            rc, st = flat_call(run_off, first, end, which, cap)
            if rc != -4 or int(run_off[-1]) <= cap:      # II2_ECAPACITY: run_off is filled, the second call is exact
                self._ck(rc)
                n = int(run_off[-1])
                return run_off, first[:n], end[:n], which[:n], st
            cap = int(run_off[-1])

    def dict_match_flat(self, dicts, pat_bytes, pat_off, pat_kind, run_off, run_first, run_end, run_dict, cap: int, n_patterns=None):
        """The same from flat host arrays (numpy, of the ABI's element types), outputs included; any of them may be None to pass
        NULL.  n_patterns: len(pat_off) - 1 unless given.  Returns (return code, MatchStats) without raising, so that a caller
        can run the two-call protocol itself."""
        arr = (C.c_void_p * len(dicts))(*[d.h if d is not None else None for d in dicts])
        n = int(n_patterns) if n_patterns is not None else (0 if pat_off is None else pat_off.size - 1)
        st = MatchStats()
        rc = self.lib.ii2_dict_match(self.h, len(dicts), arr, max(n, 0), _ptr(pat_bytes), _ptr(pat_off), _ptr(pat_kind), _ptr(run_off),
                                     _ptr(run_first), _ptr(run_end), _ptr(run_dict), int(cap), C.byref(st))
        return rc, st

    def dict_fuzzy(self, dicts, patterns, max_dist, prefix=0, flags=0):
        """Typo-tolerant term search on the device (ii2_dict_fuzzy): every pattern of `patterns` (bytes, at most 16 of at most 64
        bytes) in every one of the k resident dictionaries.  A term matches when it shares the pattern's first `prefix` bytes and
        lies within `max_dist` edits (0 .. 255) of it; flags: 0, II2_FUZZY_TRANSPOSE, II2_MATCH_NOCASE and / or II2_MATCH_UTF8 (prefix,
        edits and the length filter count UTF-8 symbols; stats.n_utf8 = the patterns that carry it).  Each of the
        three is one value for all the patterns or one per pattern.  Returns (run_off, run_first, run_end, run_dict, stats), laid
        out as dict_match's: the runs of pattern p, run_off[p * k] .. run_off[(p + 1) * k] - 1, are one group of the range
        entry points.  A result that outgrows the first buffer takes a second call of the exact size."""
        patterns = list(patterns)
        dist, pre, fl = (_per_pattern(v, len(patterns), "dict_fuzzy", what + " per pattern")
                         for v, what in ((max_dist, "max_dist"), (prefix, "prefix"), (flags, "flags")))
        blob, off = _flat(patterns)
        return self._dict_runs(dicts, len(patterns), lambda *out: self.dict_fuzzy_flat(dicts, blob, off, dist, pre, fl, *out))

    def dict_fuzzy_flat(self, dicts, pat_bytes, pat_off, pat_dist, pat_prefix, pat_flags, run_off, run_first, run_end, run_dict, cap: int,
                        n_patterns=None):
        """The same from flat host arrays (numpy, of the ABI's element types), outputs included; any of them may be None to pass
        NULL.  n_patterns: len(pat_off) - 1 unless given.  Returns (return code, FuzzyStats) without raising, so that a caller
        can run the two-call protocol itself."""
        arr = (C.c_void_p * len(dicts))(*[d.h if d is not None else None for d in dicts])
        n = int(n_patterns) if n_patterns is not None else (0 if pat_off is None else pat_off.size - 1)
        st = FuzzyStats()
        rc = self.lib.ii2_dict_fuzzy(self.h, len(dicts), arr, max(n, 0), _ptr(pat_bytes), _ptr(pat_off), _ptr(pat_dist), _ptr(pat_prefix),
                                     _ptr(pat_flags), _ptr(run_off), _ptr(run_first), _ptr(run_end), _ptr(run_dict), int(cap), C.byref(st))
        return rc, st

    def dict_regex(self, dicts, patterns, flags=0):
        """Regular-expression term search on the device (ii2_dict_regex): every pattern of `patterns` (bytes, at most 8 of at most
        256 bytes and 64 positions; the syntax is in include/ii2.h) in every one of the k resident dictionaries.  A pattern
        matches a term when it matches the WHOLE term; flags: 0 or II2_MATCH_NOCASE, one value for all the patterns or one per
        pattern.  Returns (run_off, run_first, run_end, run_dict, stats), laid out as dict_match's: the runs of pattern p,
        run_off[p * k] .. run_off[(p + 1) * k] - 1, are one group of the range entry points.  A result that outgrows the first
        buffer takes a second call of the exact size."""
        patterns = list(patterns)
        fl = _per_pattern(flags, len(patterns), "dict_regex", "flags per pattern")
        blob, off = _flat(patterns)
        return self._dict_runs(dicts, len(patterns), lambda *out: self.dict_regex_flat(dicts, blob, off, fl, *out))

    def dict_regex_flat(self, dicts, pat_bytes, pat_off, pat_flags, run_off, run_first, run_end, run_dict, cap: int, n_patterns=None):
        """The same from flat host arrays (numpy, of the ABI's element types), outputs included; any of them may be None to pass
        NULL.  n_patterns: len(pat_off) - 1 unless given.  Returns (return code, RegexStats) without raising, so that a caller
        can run the two-call protocol itself."""
        arr = (C.c_void_p * len(dicts))(*[d.h if d is not None else None for d in dicts])
        n = int(n_patterns) if n_patterns is not None else (0 if pat_off is None else pat_off.size - 1)
        st = RegexStats()
        rc = self.lib.ii2_dict_regex(self.h, len(dicts), arr, max(n, 0), _ptr(pat_bytes), _ptr(pat_off), _ptr(pat_flags), _ptr(run_off),
                                     _ptr(run_first), _ptr(run_end), _ptr(run_dict), int(cap), C.byref(st))
        return rc, st

    def align_dicts(self, dicts) -> "Alignment":
        """The union of k resident dictionaries and every dictionary's place in it (ii2_align_dicts): no upload, no sort."""
        arr = (C.c_void_p * len(dicts))(*[d.h for d in dicts])
        h = C.c_void_p()
        self._ck(self.lib.ii2_align_dicts(self.h, len(dicts), arr, C.byref(h)))
        flat = None
        if all(d.terms is not None for d in dicts):
            flat = [t for d in dicts for t in d.terms]
        return Alignment(self, h, flat)

    def select_aligned(self, seg: "Segment", alignment: "Alignment", s: int, first_list: int = 0) -> "Segment":
        out = C.c_void_p()
        self._ck(self.lib.ii2_seg_select_aligned(self.h, seg.h, alignment.h, s, first_list, C.byref(out)))
        return Segment(self, out)

    def select_aligned_all(self, segs: Sequence["Segment"], alignment: "Alignment", first_list=None) -> List["Segment"]:
        """The aligned views of all the alignment's dictionaries in one call (ii2_seg_select_aligned_all)."""
        arr = (C.c_void_p * len(segs))(*[s.h for s in segs])
        outs = (C.c_void_p * len(segs))()
        fl = _np(first_list, np.uint64) if first_list is not None else None
        self._ck(self.lib.ii2_seg_select_aligned_all(self.h, arr, alignment.h, _ptr(fl) if fl is not None else None, outs))
        return [Segment(self, C.c_void_p(h)) for h in outs]

    def select(self, seg: "Segment", src_list) -> "Segment":
        src = _np(src_list, np.int64)
        out = C.c_void_p()
        self._ck(self.lib.ii2_seg_select(self.h, seg.h, src.size, _ptr(src), C.byref(out)))
        return Segment(self, out)

    # ---- operators ------------------------------------------------------------------------
    def _listargs(self, lists):
        segs = (C.c_void_p * len(lists))(*[s.h for s, _ in lists])
        idx = (C.c_uint64 * len(lists))(*[int(i) for _, i in lists])
        return segs, idx

    def intersect(self, lists, tomb: Optional["Tombstones"] = None, out: Optional[DeviceArray] = None,
                  cap: Optional[int] = None):
        """lists: [(Segment, list_index), ...].  Returns (DeviceArray ids, count)."""
        segs, idx = self._listargs(lists)
        if cap is None:
            cap = min(s.list_blocks(i, self) for s, i in lists) * 256 if out is None else out.count
        if out is None:
            out = self.empty(max(cap, 1))
        cnt = C.c_uint64()
        self._ck(self.lib.ii2_intersect(self.h, len(lists), segs, idx, tomb.h if tomb else None, _ptr(out), cap, C.byref(cnt)))
        return out, cnt.value

    def intersect_async(self, lists, tomb, out: DeviceArray, d_count: DeviceArray) -> None:
        segs, idx = self._listargs(lists)
        self._ck(self.lib.ii2_intersect_async(self.h, len(lists), segs, idx, tomb.h if tomb else None, _ptr(out), out.count,
                                              _ptr(d_count)))

    def union(self, lists, tomb: Optional["Tombstones"] = None, out: Optional[DeviceArray] = None):
        """PrefixSearch's append + sort + compact (inverted_index.go:274-292)."""
        segs, idx = self._listargs(lists)
        if out is None:
            out = self.empty(max(sum(s.list_blocks(i, self) for s, i in lists) * 256, 1))
        cnt = C.c_uint64()
        self._ck(self.lib.ii2_union(self.h, len(lists), segs, idx, tomb.h if tomb else None, _ptr(out), out.count, C.byref(cnt)))
        return out, cnt.value

    def union_ranges(self, ranges, tomb: Optional["Tombstones"] = None, out: Optional[DeviceArray] = None):
        """PrefixSearch's union over any number of lists (ii2_union_ranges): ranges = [(Segment, first, end), ...], every list
        [first, end) of the segment.  Returns (DeviceArray ids, count); the default `out` holds 256 ids per block of the lists."""
        ranges = [(s, int(a), int(b)) for s, a, b in ranges]
        n = len(ranges)
        segs = (C.c_void_p * max(n, 1))(*[s.h for s, _, _ in ranges])
        first = (C.c_uint64 * max(n, 1))(*[a for _, a, _ in ranges])
        end = (C.c_uint64 * max(n, 1))(*[b for _, _, b in ranges])
        if out is None:
            out = self.empty(max(sum(s.range_blocks(a, b, self) for s, a, b in ranges) * 256, 1))
        cnt = C.c_uint64()
        self._ck(self.lib.ii2_union_ranges(self.h, n, segs, first, end, tomb.h if tomb else None, _ptr(out), out.count, C.byref(cnt)))
        return out, cnt.value

    def intersect_ranges(self, groups, tomb: Optional["Tombstones"] = None, out: Optional[DeviceArray] = None):
        """AND of ORs over list ranges (ii2_intersect_ranges): groups = [[(Segment, first, end), ...], ...]; the ids found in at
        least one list of every group.  Returns (DeviceArray ids, count); the default `out` holds 256 ids per block of the group
        with the fewest blocks."""
        groups = [[(s, int(a), int(b)) for s, a, b in g] for g in groups]
        ranges = [r for g in groups for r in g]
        n = len(ranges)
        gf = np.zeros(len(groups) + 1, np.uint64)
        gf[1:] = np.cumsum([len(g) for g in groups], dtype=np.uint64) if groups else []
        group_first = (C.c_uint64 * len(gf))(*[int(x) for x in gf])
        segs = (C.c_void_p * max(n, 1))(*[s.h for s, _, _ in ranges])
        first = (C.c_uint64 * max(n, 1))(*[a for _, a, _ in ranges])
        end = (C.c_uint64 * max(n, 1))(*[b for _, _, b in ranges])
        if out is None:
            blocks = [sum(s.range_blocks(a, b, self) for s, a, b in g) for g in groups]
            out = self.empty(max(min(blocks, default=0) * 256, 1))
        cnt = C.c_uint64()
        self._ck(self.lib.ii2_intersect_ranges(self.h, len(groups), group_first, segs, first, end, tomb.h if tomb else None, _ptr(out),
                                               out.count, C.byref(cnt)))
        return out, cnt.value

    def andnot_ranges(self, groups, exclude, tomb: Optional["Tombstones"] = None, out: Optional[DeviceArray] = None):
        """AND of ORs minus excluded groups (ii2_andnot_ranges): groups and exclude are lists of groups as intersect_ranges takes
        them; the ids found in at least one list of every group of `groups` and in no list of any group of `exclude`.  Returns
        (DeviceArray ids, count); the default `out` holds 256 ids per block of the required group with the fewest blocks."""
        group_first, group_not, gsegs, first, end = pack_andnot(groups, exclude)
        n = len(gsegs)
        segs = (C.c_void_p * max(n, 1))(*[s.h for s in gsegs])
        if out is None:
            blocks = [sum(s.range_blocks(int(a), int(b), self) for s, a, b in g) for g in groups]
            out = self.empty(max(min(blocks, default=0) * 256, 1))
        cnt = C.c_uint64()
        self._ck(self.lib.ii2_andnot_ranges(self.h, len(group_not), group_first.ctypes.data_as(_lib.u64p), group_not.ctypes.data_as(_lib.u8p),
                                            segs, first.ctypes.data_as(_lib.u64p), end.ctypes.data_as(_lib.u64p), tomb.h if tomb else None,
                                            _ptr(out), out.count, C.byref(cnt)))
        return out, cnt.value

    def atleast_ranges(self, groups, min_match: int, exclude=(), tomb: Optional["Tombstones"] = None, out: Optional[DeviceArray] = None,
                       stats: bool = False):
        """Threshold query (ii2_atleast_ranges): groups and exclude are lists of groups as andnot_ranges takes them; the ids found
        in at least one list of at least `min_match` groups of `groups` and in no list of any group of `exclude`.  A group without
        postings matches no doc.  Returns (DeviceArray ids, count), with stats=True (DeviceArray ids, count, AtleastStats); the
        default `out` holds 256 ids per block of the n' - min_match + 1 groups with the fewest blocks, n' the groups that have blocks."""
        groups = [list(g) for g in groups]
        group_first, group_not, gsegs, first, end = pack_andnot(groups, exclude)
        n = len(gsegs)
        segs = (C.c_void_p * max(n, 1))(*[s.h for s in gsegs])
        if out is None:
            blocks = sorted(b for b in (sum(s.range_blocks(int(a), int(b), self) for s, a, b in g) for g in groups) if b)
            out = self.empty(max(sum(blocks[:max(len(blocks) - int(min_match) + 1, 0)]) * 256, 1))
        cnt = C.c_uint64()
        st = AtleastStats()
        self._ck(self.lib.ii2_atleast_ranges(self.h, len(group_not), group_first.ctypes.data_as(_lib.u64p), group_not.ctypes.data_as(_lib.u8p),
                                             int(min_match), segs, first.ctypes.data_as(_lib.u64p), end.ctypes.data_as(_lib.u64p),
                                             tomb.h if tomb else None, _ptr(out), out.count, C.byref(cnt), C.byref(st)))
        return (out, cnt.value, st) if stats else (out, cnt.value)

    def topk_ranges(self, groups, k: int, min_match: int = 1, exclude=(), tomb: Optional["Tombstones"] = None, stats: bool = False,
                    out: Optional[tuple] = None):
        """Ranked query (ii2_topk_ranges): groups and exclude as atleast_ranges takes them; the `k` docs that lie in the most groups
        of `groups` - at least `min_match` of them, in no list of any group of `exclude`, not in `tomb` - ordered by score
        descending, then id ascending.  Returns (DeviceArray ids, DeviceArray scores, count), with stats=True also the score
        histogram (ndarray[256]: eligible docs per score) and TopkStats.  k = 0: the histogram and stats only.  `out`: (ids, scores)
        DeviceArrays of at least k entries to write into instead of fresh ones."""
        groups = [list(g) for g in groups]
        group_first, group_not, gsegs, first, end = pack_andnot(groups, exclude)
        n = len(gsegs)
        segs = (C.c_void_p * max(n, 1))(*[s.h for s in gsegs])
        ids, scores = out if out is not None else (self.empty(max(int(k), 1)), self.empty(max(int(k), 1)))
        if ids.count < int(k) or scores.count < int(k):
            raise ValueError("topk_ranges: out holds fewer than k entries")
        cnt = C.c_uint64()
        st = TopkStats()
        hist = np.zeros(256, np.uint64)
        self._ck(self.lib.ii2_topk_ranges(self.h, len(group_not), group_first.ctypes.data_as(_lib.u64p), group_not.ctypes.data_as(_lib.u8p),
                                          int(min_match), int(k), segs, first.ctypes.data_as(_lib.u64p), end.ctypes.data_as(_lib.u64p),
                                          tomb.h if tomb else None, _ptr(ids), _ptr(scores), C.byref(cnt), hist.ctypes.data_as(_lib.u64p), C.byref(st)))
        return (ids, scores, cnt.value, hist, st) if stats else (ids, scores, cnt.value)

    def topk_weighted_ranges(self, groups, weights, k: int, min_score: int = 1, exclude=(), tomb: Optional["Tombstones"] = None,
                             stats: bool = False, out: Optional[tuple] = None):
        """Ranked query with a weight per group (ii2_topk_weighted_ranges): groups, exclude, k, tomb and out as topk_ranges takes
        them; `weights` holds one integer 1 .. 255 per group of `groups` (None: every weight is 1) and a doc's score is the sum of
        the weights of the groups it lies in - at least `min_score`, at most 255.  Returns (DeviceArray ids, DeviceArray scores,
        count), with stats=True also the score histogram (ndarray[256]) and TopkwStats."""
        groups = [list(g) for g in groups]
        group_first, group_not, gsegs, first, end = pack_andnot(groups, exclude)
        n = len(gsegs)
        segs = (C.c_void_p * max(n, 1))(*[s.h for s in gsegs])
        c_weights = None
        if weights is not None:
            if len(weights) != len(groups):
                raise ValueError("topk_weighted_ranges: one weight per group")
            c_weights = (C.c_uint32 * max(len(group_not), 1))(*[int(w) for w in weights])      # (an excluded group's entry is ignored)
        ids, scores = out if out is not None else (self.empty(max(int(k), 1)), self.empty(max(int(k), 1)))
        if ids.count < int(k) or scores.count < int(k):
            raise ValueError("topk_weighted_ranges: out holds fewer than k entries")
        cnt = C.c_uint64()
        st = TopkwStats()
        hist = np.zeros(256, np.uint64)
        self._ck(self.lib.ii2_topk_weighted_ranges(self.h, len(group_not), group_first.ctypes.data_as(_lib.u64p), group_not.ctypes.data_as(_lib.u8p),
                                                   c_weights, int(min_score), int(k), segs, first.ctypes.data_as(_lib.u64p),
                                                   end.ctypes.data_as(_lib.u64p), tomb.h if tomb else None, _ptr(ids), _ptr(scores), C.byref(cnt),
                                                   hist.ctypes.data_as(_lib.u64p), C.byref(st)))
        return (ids, scores, cnt.value, hist, st) if stats else (ids, scores, cnt.value)

    def query_batch(self, queries, tomb: Optional["Tombstones"] = None, out: Optional[DeviceArray] = None):
        """Many AND / OR queries in one call (ii2_query_batch): queries = [("and" | "or", [(Segment, first, end), ...]), ...] -
        an "or" is the union of every list in its ranges, an "and" takes every list in its ranges as one operand.  Returns
        (DeviceArray ids, offsets): result q is ids[offsets[q] : offsets[q + 1]].  The default `out` holds 256 ids per block
        of each query's bound (and: its operand with the fewest blocks; or: every block of its ranges)."""
        op, query_first, qsegs, first, end = pack_batch(queries)
        n = len(qsegs)
        segs = (C.c_void_p * max(n, 1))(*[s.h for s in qsegs])
        if out is None:
            blocks = 0
            for q, (_, ranges) in enumerate(queries):
                if op[q] == II2_OP_OR:
                    blocks += sum(s.range_blocks(int(a), int(b), self) for s, a, b in ranges)
                elif sum(max(min(int(b), s.info.n_lists) - int(a), 0) for s, a, b in ranges) <= 64:      # (more: the library rejects it)
                    blocks += min((s.list_blocks(j, self) for s, a, b in ranges
                                   for j in range(int(a), min(int(b), s.info.n_lists))), default=0)
            out = self.empty(max(blocks * 256, 1))
        off = np.zeros(len(queries) + 1, np.uint64)
        self._ck(self.lib.ii2_query_batch(self.h, len(queries), op.ctypes.data_as(_lib.u8p), query_first.ctypes.data_as(_lib.u64p), segs,
                                          first.ctypes.data_as(_lib.u64p), end.ctypes.data_as(_lib.u64p), tomb.h if tomb else None,
                                          _ptr(out), out.count, off.ctypes.data_as(_lib.u64p)))
        return out, off

    def query_batch_groups(self, queries, tomb: Optional["Tombstones"] = None, out: Optional[DeviceArray] = None):
        """Many AND-of-ORs / NOT queries in one call (ii2_query_batch_groups): queries = [(groups, exclude), ...], each pair as
        andnot_ranges takes it - the ids found in at least one list of every group of `groups` and in no list of any group of
        `exclude`; one group and no exclusion is a union.  Returns (DeviceArray ids, offsets): result q is ids[offsets[q] :
        offsets[q + 1]].  The default `out` holds 256 ids per block of each query's required group with the fewest blocks."""
        query_first, group_first, group_not, qsegs, first, end = pack_group_batch(queries)
        n = len(qsegs)
        segs = (C.c_void_p * max(n, 1))(*[s.h for s in qsegs])
        if out is None:
            blocks = 0
            for groups, _ in queries:
                blocks += min((sum(s.range_blocks(int(a), int(b), self) for s, a, b in g) for g in groups), default=0)
            out = self.empty(max(blocks * 256, 1))
        off = np.zeros(len(queries) + 1, np.uint64)
        self._ck(self.lib.ii2_query_batch_groups(self.h, len(queries), query_first.ctypes.data_as(_lib.u64p), group_first.ctypes.data_as(_lib.u64p),
                                                 group_not.ctypes.data_as(_lib.u8p), segs, first.ctypes.data_as(_lib.u64p),
                                                 end.ctypes.data_as(_lib.u64p), tomb.h if tomb else None, _ptr(out), out.count,
                                                 off.ctypes.data_as(_lib.u64p)))
        return out, off

    def topk_batch(self, queries, tomb: Optional["Tombstones"] = None, stats: bool = False, out: Optional[tuple] = None):
        """Many ranked queries in one call (ii2_topk_batch): queries = [(groups, weights | None, k, min_score, exclude), ...], each
        as topk_weighted_ranges takes it.  Returns (DeviceArray ids, DeviceArray scores, offsets, eligible), with stats=True also
        TopkBatchStats: result q is ids / scores[offsets[q] : offsets[q + 1]], eligible[q] its number of eligible docs.  The default
        `out` holds sum(k) entries each; `out` = (ids, scores) DeviceArrays to write into instead, scores may be None."""
        query_first, group_first, group_not, qsegs, first, end, weight, min_score, k = pack_topk_batch(queries)
        n = len(qsegs)
        segs = (C.c_void_p * max(n, 1))(*[s.h for s in qsegs])
        if out is None:
            cap = max(int(k.sum(dtype=np.uint64)), 1)
            out = (self.empty(cap), self.empty(cap))
        ids, scores = out
        if scores is not None and scores.count < ids.count:
            raise ValueError("topk_batch: scores holds fewer entries than ids")
        off = np.zeros(len(queries) + 1, np.uint64)
        eligible = np.zeros(len(queries), np.uint64)
        st = TopkBatchStats()
        self._ck(self.lib.ii2_topk_batch(self.h, len(queries), query_first.ctypes.data_as(_lib.u64p), group_first.ctypes.data_as(_lib.u64p),
                                         group_not.ctypes.data_as(_lib.u8p), None if weight is None else weight.ctypes.data_as(_lib.u32p),
                                         min_score.ctypes.data_as(_lib.u32p), k.ctypes.data_as(_lib.u32p), segs, first.ctypes.data_as(_lib.u64p),
                                         end.ctypes.data_as(_lib.u64p), tomb.h if tomb else None, _ptr(ids), _ptr(scores), ids.count,
                                         off.ctypes.data_as(_lib.u64p), eligible.ctypes.data_as(_lib.u64p), C.byref(st)))
        return (ids, scores, off, eligible, st) if stats else (ids, scores, off, eligible)

    def count_ranges(self, ranges, dset: Optional[DeviceArray] = None, n_set: Optional[int] = None,
                     tomb: Optional["Tombstones"] = None):
        """Hits per list against a doc set (ii2_count_ranges: facet counts): ranges = [(Segment, first, end), ...] as union_ranges
        takes them; dset is a DeviceArray of ascending, duplicate-free ids - what every query returns - of which the first n_set
        count (default: all of it), or None for "every doc".  Returns (uint64 counts, one per list named in range order: its ids
        that lie in the set and not in tomb; CountStats)."""
        ranges = [(s, int(a), int(b)) for s, a, b in ranges]
        n = len(ranges)
        segs = (C.c_void_p * max(n, 1))(*[s.h for s, _, _ in ranges])
        first = (C.c_uint64 * max(n, 1))(*[a for _, a, _ in ranges])
        end = (C.c_uint64 * max(n, 1))(*[b for _, _, b in ranges])
        if dset is None:
            n_set = 0
        elif n_set is None:
            n_set = dset.count
        counts = np.zeros(sum(max(b - a, 0) for _, a, b in ranges), np.uint64)
        st = CountStats()
        self._ck(self.lib.ii2_count_ranges(self.h, n, segs, first, end, _ptr(dset), int(n_set), tomb.h if tomb else None,
                                           counts.ctypes.data_as(_lib.u64p), counts.size, C.byref(st)))
        return counts, st

    def histogram_ranges(self, ranges, edges, dset: Optional[DeviceArray] = None, n_set: Optional[int] = None,
                         tomb: Optional["Tombstones"] = None):
        """Hits per list and value bucket (ii2_histogram_ranges): ranges, dset, n_set and tomb as count_ranges takes them; edges =
        n_buckets + 1 strictly ascending values <= 2^32, bucket b = the ids edges[b] <= id < edges[b + 1].  Returns (uint64 counts
        of shape (lists named, n_buckets); HistStats)."""
        ranges = [(s, int(a), int(b)) for s, a, b in ranges]
        n = len(ranges)
        segs = (C.c_void_p * max(n, 1))(*[s.h for s, _, _ in ranges])
        first = (C.c_uint64 * max(n, 1))(*[a for _, a, _ in ranges])
        end = (C.c_uint64 * max(n, 1))(*[b for _, _, b in ranges])
        if dset is None:
            n_set = 0
        elif n_set is None:
            n_set = dset.count
        e, nb = _edges(edges)
        n_named = sum(max(b - a, 0) for _, a, b in ranges)
        counts = np.zeros((n_named, nb), np.uint64)
        st = HistStats()
        self._ck(self.lib.ii2_histogram_ranges(self.h, n, segs, first, end, _ptr(dset), int(n_set), tomb.h if tomb else None, nb,
                                               e.ctypes.data_as(_lib.u64p), counts.ctypes.data_as(_lib.u64p), counts.size, C.byref(st)))
        return counts, st

    def histogram_ids(self, dset: DeviceArray, n_set: Optional[int], edges, tomb: Optional["Tombstones"] = None):
        """The bucket counts of an ascending, duplicate-free device set (ii2_histogram_ids): uint64 [n_buckets], the first n_set ids
        of dset (None: all of it) per bucket of `edges`, minus tomb."""
        if n_set is None:
            n_set = dset.count
        e, nb = _edges(edges)
        counts = np.zeros(nb, np.uint64)
        self._ck(self.lib.ii2_histogram_ids(self.h, _ptr(dset), int(n_set), tomb.h if tomb else None, nb, e.ctypes.data_as(_lib.u64p),
                                            counts.ctypes.data_as(_lib.u64p), counts.size))
        return counts

    def explain_ranges(self, groups, ids: DeviceArray, n_ids: Optional[int] = None, stats: bool = False, out: Optional[DeviceArray] = None):
        """Which groups each doc lies in (ii2_explain_ranges): groups = [[(Segment, first, end), ...], ...] as intersect_ranges
        takes them; ids is a DeviceArray of doc ids IN ANY ORDER - a query's ascending result or a ranked page - of which the first
        n_ids count (default: all of it).  Returns a uint64 DeviceArray of n_ids * n_words mask words, doc-major, n_words =
        ceil(len(groups) / 64), its `shape` attribute (n_ids, n_words): bit g & 63 of word i * n_words + (g >> 6) says ids[i] lies
        in a list of group g; a repeated id has its mask in its first row and zeros after.  With stats=True (masks, ExplainStats).
        `out`: a uint64 DeviceArray of at least n_ids * n_words words to write into instead of a fresh one."""
        groups = [[(s, int(a), int(b)) for s, a, b in g] for g in groups]
        ranges = [r for g in groups for r in g]
        n = len(ranges)
        gf = np.zeros(len(groups) + 1, np.uint64)
        gf[1:] = np.cumsum([len(g) for g in groups], dtype=np.uint64) if groups else []
        segs = (C.c_void_p * max(n, 1))(*[s.h for s, _, _ in ranges])
        first = np.array([a for _, a, _ in ranges] or [0], np.uint64)
        end = np.array([b for _, _, b in ranges] or [0], np.uint64)
        n_ids = ids.count if n_ids is None else int(n_ids)
        n_words = (len(groups) + 63) // 64
        if out is None:
            out = self.empty(max(n_ids * n_words, 1), np.uint64)
        if out.dtype != np.uint64:
            raise ValueError("explain_ranges: out is not a uint64 array")
        st = ExplainStats()
        self._ck(self.lib.ii2_explain_ranges(self.h, len(groups), gf.ctypes.data_as(_lib.u64p), segs, first.ctypes.data_as(_lib.u64p),
                                             end.ctypes.data_as(_lib.u64p), _ptr(ids), n_ids, _ptr(out), out.count, C.byref(st)))
        out.shape = (n_ids, n_words)
        return (out, st) if stats else out

    def explain_batch(self, queries, ids: DeviceArray, ids_off, stats: bool = False, out: Optional[DeviceArray] = None):
        """Many explains in one call (ii2_explain_batch): queries = [groups, ...], each as explain_ranges takes it; query q explains
        ids[ids_off[q] : ids_off[q + 1]] - the ids / offsets topk_batch and query_batch_groups return fit as they are.  Returns
        (uint64 DeviceArray of the packed masks, mask_off): query q's rows, (ids_off[q + 1] - ids_off[q]) x ceil(len(queries[q]) / 64)
        words, start at word mask_off[q] and are what explain_ranges writes for it alone.  With stats=True also ExplainBatchStats.
        `out`: a uint64 DeviceArray of at least mask_off[-1] words to write into instead of a fresh one."""
        queries = [list(groups) for groups in queries]
        query_first, group_first, qsegs, first, end = pack_explain_batch(queries)
        ids_off = np.ascontiguousarray(ids_off, np.uint64)
        if ids_off.size != len(queries) + 1:
            raise ValueError("explain_batch: ids_off holds len(queries) + 1 offsets")
        n = len(qsegs)
        segs = (C.c_void_p * max(n, 1))(*[s.h for s in qsegs])
        if out is None:
            words = sum(int(ids_off[q + 1] - ids_off[q]) * ((len(g) + 63) // 64) for q, g in enumerate(queries) if ids_off[q + 1] > ids_off[q])
            out = self.empty(max(words, 1), np.uint64)
        if out.dtype != np.uint64:
            raise ValueError("explain_batch: out is not a uint64 array")
        mask_off = np.zeros(len(queries) + 1, np.uint64)
        st = ExplainBatchStats()
        self._ck(self.lib.ii2_explain_batch(self.h, len(queries), query_first.ctypes.data_as(_lib.u64p), group_first.ctypes.data_as(_lib.u64p), segs,
                                            first.ctypes.data_as(_lib.u64p), end.ctypes.data_as(_lib.u64p), _ptr(ids), ids_off.ctypes.data_as(_lib.u64p),
                                            _ptr(out), out.count, mask_off.ctypes.data_as(_lib.u64p), C.byref(st)))
        return (out, mask_off, st) if stats else (out, mask_off)

    def merge(self, segs: Sequence["Segment"], tomb: Optional["Tombstones"] = None,
              out_off: Optional[DeviceArray] = None, out_values: Optional[DeviceArray] = None):
        """Shard.Merge's loop body (shard.go:163-212).  Returns (out_off u64[T+1], out_values, MergeStats)."""
        T = segs[0].info.n_lists
        if out_off is None:
            out_off = self.empty(T + 1, np.uint64)
        if out_values is None:
            out_values = self.empty(max(sum(s.info.n_postings for s in segs), 1))
        arr = (C.c_void_p * len(segs))(*[s.h for s in segs])
        st = MergeStats()
        self._ck(self.lib.ii2_merge_segments(self.h, len(segs), arr, tomb.h if tomb else None, _ptr(out_off), _ptr(out_values),
                                             out_values.count, C.byref(st)))
        return out_off, out_values, st

    def merge_to_segment(self, segs: Sequence["Segment"], tomb: Optional["Tombstones"] = None):
        arr = (C.c_void_p * len(segs))(*[s.h for s in segs])
        st = MergeStats()
        out = C.c_void_p()
        self._ck(self.lib.ii2_merge_segments_to_seg(self.h, len(segs), arr, tomb.h if tomb else None, C.byref(out), C.byref(st)))
        return (Segment(self, out) if out.value else None), st

    # ---- host-buffer calls (what the cgo binding uses) ---------------------------------------
    def merge_small(self, segs: Sequence["Segment"], dictionaries, removed=()):
        """The common Shard.Merge in one launch (ii2_merge_small): k small segments with their term dictionaries (lists of
        bytes, segs[s] holding one list per term of dictionaries[s]) and RemovedLists.Values().  Returns (merged Segment or
        None, its terms, MergeStats)."""
        flat, blob, off, first = _flat_dicts(dictionaries)
        rem = _np(removed, np.uint32)
        arr = (C.c_void_p * len(segs))(*[s.h for s in segs])
        out = C.c_void_p()
        kept = np.zeros(max(len(flat), 1), np.uint64)
        n_kept = C.c_uint64()
        st = MergeStats()
        self._ck(self.lib.ii2_merge_small(self.h, len(segs), arr, _ptr(blob), _ptr(off), _ptr(first), _ptr(rem) if rem.size else None, rem.size,
                                          C.byref(out), kept.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n_kept), C.byref(st)))
        terms = [flat[int(g)] for g in kept[: n_kept.value]]
        return (Segment(self, out) if out.value else None), terms, st

    def read_small(self, segs: Sequence["Segment"], dictionaries, list_first=None):
        """The small Shard.Read in one launch (ii2_read_small): the merged lists of k small segments (dictionaries[s] names the
        lists list_first[s] .. of segs[s]) on the host.  Returns (terms, post_off, values)."""
        flat, blob, off, first = _flat_dicts(dictionaries)
        lf = _np(list_first, np.uint64) if list_first is not None else None
        arr = (C.c_void_p * len(segs))(*[s.h for s in segs])
        cap = int(sum(s.info.n_postings for s in segs))
        rep = np.zeros(max(len(flat), 1), np.uint64)
        post_off = np.zeros(len(flat) + 1, np.uint64)
        values = np.zeros(max(cap, 1), np.uint32)
        n_union = C.c_uint64()
        self._ck(self.lib.ii2_read_small(self.h, len(segs), arr, _ptr(blob), _ptr(off), _ptr(first), _ptr(lf) if lf is not None else None,
                                         rep.ctypes.data_as(C.POINTER(C.c_uint64)), post_off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         _ptr(values), cap, C.byref(n_union)))
        nu = n_union.value
        return [flat[int(g)] for g in rep[:nu]], post_off[: nu + 1].copy(), values[: int(post_off[nu])].copy()

    def merge_host(self, seg_offs, seg_vals, removed=()):
        k = len(seg_offs)
        offs = [_np(o, np.uint64) for o in seg_offs]
        vals = [_np(v, np.uint32) for v in seg_vals]
        T = offs[0].size - 1
        flat_off = np.concatenate(offs) if k else np.zeros(0, np.uint64)
        base = np.zeros(k + 1, np.uint64)
        base[1:] = np.cumsum([v.size for v in vals])
        flat = np.concatenate(vals) if k else np.empty(0, np.uint32)
        rem = _np(removed, np.uint32)
        out_off = np.zeros(T + 1, np.uint64)
        out_vals = np.empty(max(flat.size, 1), np.uint32)
        st = MergeStats()
        self._ck(self.lib.ii2_merge_host(self.h, k, T, _ptr(flat_off), _ptr(base), _ptr(flat), _ptr(rem) if rem.size else None,
                                         rem.size, _ptr(out_off), _ptr(out_vals), out_vals.size, C.byref(st)))
        return out_off, out_vals[: int(out_off[-1])].copy(), st

    def _flat_lists(self, lists):
        arrs = [_np(l, np.uint32) for l in lists]
        off = np.zeros(len(arrs) + 1, np.uint64)
        if arrs:
            off[1:] = np.cumsum([a.size for a in arrs])
        flat = np.concatenate(arrs) if arrs else np.empty(0, np.uint32)
        return off, _np(flat, np.uint32)

    def intersect_host(self, lists, removed=()) -> np.ndarray:
        off, flat = self._flat_lists(lists)
        rem = _np(removed, np.uint32)
        cap = max(min((int(off[i + 1] - off[i]) for i in range(len(lists))), default=0), 1)
        out = np.empty(cap, np.uint32)
        cnt = C.c_uint64()
        self._ck(self.lib.ii2_intersect_host(self.h, len(lists), _ptr(off), _ptr(flat), _ptr(rem) if rem.size else None, rem.size,
                                             _ptr(out), cap, C.byref(cnt)))
        return out[: cnt.value].copy()

    def union_host(self, lists, removed=()) -> np.ndarray:
        off, flat = self._flat_lists(lists)
        rem = _np(removed, np.uint32)
        out = np.empty(max(flat.size, 1), np.uint32)
        cnt = C.c_uint64()
        self._ck(self.lib.ii2_union_host(self.h, len(lists), _ptr(off), _ptr(flat), _ptr(rem) if rem.size else None, rem.size,
                                         _ptr(out), out.size, C.byref(cnt)))
        return out[: cnt.value].copy()

    # ---- multi-GPU ---------------------------------------------------------------------------
    def comm_init(self, world: int, rank: int, unique_id: bytes) -> None:
        buf = C.create_string_buffer(unique_id, _lib.II2_UNIQUE_ID_BYTES)
        self._ck(self.lib.ii2_comm_init(self.h, world, rank, buf))

    def allgatherv(self, local: DeviceArray, n_local: int, out: DeviceArray, world: int):
        counts = (C.c_uint64 * max(world, 1))()
        self._ck(self.lib.ii2_allgatherv(self.h, _ptr(local), n_local, _ptr(out), out.count, counts))
        return [int(c) for c in counts]

    def allgatherv_bytes(self, local, n_bytes: int, out: DeviceArray, world: int):
        """Rank-order concatenation of byte arrays (any device buffers); returns the ranks' byte counts."""
        counts = (C.c_uint64 * max(world, 1))()
        self._ck(self.lib.ii2_allgatherv_bytes(self.h, _ptr(local), n_bytes, _ptr(out), out.nbytes, counts))
        return [int(c) for c in counts]

    def seg_concat(self, segs: Sequence["Segment"]) -> "Segment":
        """The lists of segs[0], then segs[1], ... as one segment on this device (ii2_seg_concat)."""
        arr = (C.c_void_p * len(segs))(*[s.h for s in segs])
        h = C.c_void_p()
        self._ck(self.lib.ii2_seg_concat(self.h, len(segs), arr, C.byref(h)))
        return Segment(self, h)

    def seg_allgather(self, local: "Segment") -> "Segment":
        """Every rank's merged segment, concatenated in rank order into one segment (the postings travel DV1-encoded)."""
        h = C.c_void_p()
        self._ck(self.lib.ii2_seg_allgather(self.h, local.h, C.byref(h)))
        return Segment(self, h)


def seg_gather_plan(shapes):
    """Host arithmetic of seg_allgather: shapes = [(n_lists, n_blocks, n_bytes)] per rank -> (rc, list_off, block_off, byte_off)."""
    world = len(shapes)
    flat = (C.c_uint64 * (3 * max(world, 1)))(*[int(x) for sh in shapes for x in sh])
    lo, bo, qo = ((C.c_uint64 * (world + 1))() for _ in range(3))
    rc = _lib.load().ii2_seg_gather_plan(flat, world, lo, bo, qo)
    return rc, list(lo), list(bo), list(qo)


def align_plan(dictionaries) -> _lib.AlignPlan:
    """Host arithmetic of the alignment (ii2_align_plan, no GPU): the brackets the ranking kernel would bisect for these k sorted,
    duplicate-free dictionaries (lists of bytes) - how many in LDS, in global memory and empty - and its constants."""
    _, blob, off, first = _flat_dicts(dictionaries)
    plan = _lib.AlignPlan()
    rc = _lib.load().ii2_align_plan(len(dictionaries), _ptr(blob), _ptr(off), _ptr(first), C.byref(plan))
    if rc:
        raise II2Error(rc, "ii2_align_plan refused the dictionaries")
    return plan


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(_lib.II2_UNIQUE_ID_BYTES)
    rc = _lib.load().ii2_comm_unique_id(buf)
    if rc:
        raise II2Error(rc, "ncclGetUniqueId failed")
    return buf.raw


class Segment:
    """Device-resident DV1 segment (ii2_seg)."""

    def __init__(self, ctx: Context, h: C.c_void_p):
        self.ctx, self.h = ctx, h
        info = SegInfo()
        ctx.lib.ii2_seg_get_info(h, C.byref(info))
        self.info = info
        self._blk_off = None

    def list_blocks(self, i: int, ctx: Optional["Context"] = None) -> int:
        """Blocks of list i.  A segment belongs to its device, not to the context that made it: any live context works."""
        if self._blk_off is None:
            c = ctx if ctx is not None and ctx.h else self.ctx
            blk = np.zeros(self.info.n_lists + 1, np.uint32)
            c._ck(c.lib.ii2_seg_export(c.h, self.h, _ptr(blk), None, None))
            self._blk_off = blk
        return int(self._blk_off[i + 1] - self._blk_off[i])

    def range_blocks(self, first: int, end: int, ctx: Optional["Context"] = None) -> int:
        """Blocks of the lists [first, end) (0 for an empty or out-of-range span; the library checks the range)."""
        if not 0 <= first < end <= self.info.n_lists:
            return 0
        self.list_blocks(first, ctx)
        return max(int(self._blk_off[end]) - int(self._blk_off[first]), 0)

    def decode(self):
        """Decode step (Reader.Next -> intcomp.UncompressUint32, file/reader.go:79-100)."""
        po = np.zeros(self.info.n_lists + 1, np.uint64)
        vals = np.empty(max(self.info.n_postings, 1), np.uint32)
        self.ctx._ck(self.ctx.lib.ii2_seg_decode(self.ctx.h, self.h, _ptr(po), _ptr(vals), II2_HOST))
        return po, vals[: self.info.n_postings]

    def export(self):
        blk = np.zeros(self.info.n_lists + 1, np.uint32)
        skip = np.zeros(self.info.n_blocks + 1, SKIP_DTYPE)
        payload = np.zeros(max(self.info.n_bytes, 1), np.uint8)
        self.ctx._ck(self.ctx.lib.ii2_seg_export(self.ctx.h, self.h, _ptr(blk), _ptr(skip), _ptr(payload)))
        return blk, skip, payload[: self.info.n_bytes]

    def meta(self, ctx: Optional["Context"] = None):
        """The arrays the library derives when the segment is made (ii2_seg_export_meta), as a dict: cnt, last_doc (u32
        [n_lists]), blk_list (u32 [n_blocks + 1], a view's n_blocks being its store's), spans (u32 [n_lists, 3]: the host mirror
        the path choice reads, None when the segment has none), and is_view, spans_mirrored, merge_blocks, merge_bytes,
        n_postings."""
        c = ctx if ctx is not None and ctx.h else self.ctx
        nl, nb = self.info.n_lists, self.info.n_blocks
        cnt, last = np.zeros(max(nl, 1), np.uint32), np.zeros(max(nl, 1), np.uint32)
        blk_list = np.zeros(nb + 1, np.uint32)
        spans = np.zeros(max(3 * nl, 1), np.uint32)
        info = _lib.SegMetaInfo()
        c._ck(c.lib.ii2_seg_export_meta(c.h, self.h, _ptr(cnt), _ptr(last), _ptr(blk_list), _ptr(spans), C.byref(info)))
        return {"cnt": cnt[:nl], "last_doc": last[:nl], "blk_list": blk_list,
                "spans": spans[: 3 * nl].reshape(nl, 3) if info.spans_mirrored else None,
                "is_view": bool(info.is_view), "spans_mirrored": bool(info.spans_mirrored), "merge_blocks": int(info.merge_blocks),
                "merge_bytes": int(info.merge_bytes), "n_postings": int(info.n_postings)}

    def dense_form(self, i: int, ctx: Optional["Context"] = None, words: bool = True):
        """The dense form a two-list AND has cached for list i (ii2_seg_dense_form), or None: a dict of origin, n_words, the
        words (u32 [n_words]; None with words=False) and store_bytes, the bytes of all forms of this segment's store.  Builds
        nothing."""
        c = ctx if ctx is not None and ctx.h else self.ctx
        info = np.zeros(4, np.uint64)
        c._ck(c.lib.ii2_seg_dense_form(c.h, self.h, int(i), _ptr(info), None, 0))
        if not info[0]:
            return None
        w = None
        if words:
            w = np.zeros(int(info[2]), np.uint32)
            c._ck(c.lib.ii2_seg_dense_form(c.h, self.h, int(i), _ptr(info), _ptr(w), len(w)))
        return {"origin": int(info[1]), "n_words": int(info[2]), "words": w, "store_bytes": int(info[3])}

    def dense_form_bytes(self, ctx: Optional["Context"] = None) -> int:
        """Bytes held by the dense forms of this segment's store."""
        c = ctx if ctx is not None and ctx.h else self.ctx
        info = np.zeros(4, np.uint64)
        c._ck(c.lib.ii2_seg_dense_form(c.h, self.h, 0, _ptr(info), None, 0))
        return int(info[3])

    def free(self) -> None:
        if self.h:
            self.ctx.lib.ii2_seg_free(self.h)      # needs no context: the segment knows its device
            self.h = None

    def __del__(self):
        try:
            if not sys.is_finalizing():      # at interpreter exit the HIP runtime may already be gone
                self.free()
        except Exception:
            pass


class Dictionary:
    """A term dictionary resident in HBM (ii2_dict)."""

    def __init__(self, ctx: Context, h: C.c_void_p, terms=None):
        self.ctx, self.h, self.terms = ctx, h, terms

    def find(self, terms, prefix=False):
        """(list_first, list_end) u64 [len(terms)] of every term of `terms` in this dictionary (Context.dict_find with k = 1)."""
        first, end, _ = self.ctx.dict_find([self], terms, prefix)
        return first[:, 0].copy(), end[:, 0].copy()

    def match(self, patterns, kind=II2_MATCH_CONTAINS):
        """(run_off, run_first, run_end, stats) of every pattern of `patterns` in this dictionary (Context.dict_match with k = 1):
        pattern p matches the terms [run_first[j], run_end[j]) for j in run_off[p] .. run_off[p + 1] - 1."""
        run_off, first, end, _, st = self.ctx.dict_match([self], patterns, kind)
        return run_off, first, end, st

    def fuzzy(self, patterns, max_dist, prefix=0, flags=0):
        """(run_off, run_first, run_end, stats) of every pattern of `patterns` in this dictionary (Context.dict_fuzzy with k = 1):
        the terms within `max_dist` edits of pattern p are [run_first[j], run_end[j]) for j in run_off[p] .. run_off[p + 1] - 1."""
        run_off, first, end, _, st = self.ctx.dict_fuzzy([self], patterns, max_dist, prefix, flags)
        return run_off, first, end, st

    def regex(self, patterns, flags=0):
        """(run_off, run_first, run_end, stats) of every pattern of `patterns` in this dictionary (Context.dict_regex with k = 1):
        the terms that regular expression p matches are [run_first[j], run_end[j]) for j in run_off[p] .. run_off[p + 1] - 1."""
        run_off, first, end, _, st = self.ctx.dict_regex([self], patterns, flags)
        return run_off, first, end, st

    def info(self):
        """(number of terms, bytes of the terms) - ii2_dict_info"""
        n, b = C.c_uint64(), C.c_uint64()
        self.ctx._ck(self.ctx.lib.ii2_dict_info(self.h, C.byref(n), C.byref(b)))
        return n.value, b.value

    def export_flat(self):
        """(u8 bytes [n_bytes], u64 offsets [n + 1]) copied to the host - ii2_dict_export"""
        n, nb = self.info()
        blob, off = np.zeros(max(nb, 1), np.uint8), np.zeros(n + 1, np.uint64)
        self.ctx._ck(self.ctx.lib.ii2_dict_export(self.ctx.h, self.h, _ptr(blob), _ptr(off)))
        return blob[:nb], off

    def export(self):
        """the terms as a list of bytes, in the dictionary's order"""
        blob, off = self.export_flat()
        raw = blob.tobytes()
        return [raw[int(off[i]):int(off[i + 1])] for i in range(off.size - 1)]

    def free(self) -> None:
        if self.h:
            self.ctx.lib.ii2_dict_free(self.h)
            self.h = None

    def __del__(self):
        try:
            if not sys.is_finalizing():
                self.free()
        except Exception:
            pass


class Alignment:
    """Device-resident result of Context.align_terms / align_dicts (ii2_align)."""

    def __init__(self, ctx: Context, h: C.c_void_p, flat_terms):
        self.ctx, self.h, self._flat = ctx, h, flat_terms
        n, k = C.c_uint64(), C.c_uint32()
        ctx.lib.ii2_align_info(h, C.byref(n), C.byref(k))
        self.n_union, self.k = n.value, k.value

    def export(self):
        """(union terms as bytes, src_list int64 [k][n_union])."""
        rep = np.zeros(max(self.n_union, 1), np.uint64)
        src = np.zeros(max(self.k * self.n_union, 1), np.int64)
        self.ctx._ck(self.ctx.lib.ii2_align_export(self.ctx.h, self.h, _ptr(rep), _ptr(src)))
        terms = [self._flat[int(g)] for g in rep[: self.n_union]] if self._flat is not None else rep[: self.n_union].copy()
        return terms, src[: self.k * self.n_union].reshape(self.k, self.n_union)

    def free(self) -> None:
        if self.h:
            self.ctx.lib.ii2_align_free(self.h)
            self.h = None

    def __del__(self):
        try:
            if not sys.is_finalizing():
                self.free()
        except Exception:
            pass


class Tombstones:
    def __init__(self, ctx: Context, h: C.c_void_p):
        self.ctx, self.h = ctx, h

    def free(self) -> None:
        if self.h:
            self.ctx.lib.ii2_tomb_free(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.ctx.h and not sys.is_finalizing():
                self.free()
        except Exception:
            pass
