"""Python face of the C++ host mirror (host/host_index.cpp, libii2_host.so): the reference's Shard and
InvertedIndex operations — Put / Read / Merge / Remove (PutRemoved) / PrefixSearch, plus the
additive Intersect — with every posting operation executed on the GPU through the C ABI.
Segments stay in HBM; terms are byte strings.  Errors surface as HostError with the
reference-style "s: merge: …" prefix."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib
from .engine import Context, _flat

vp = C.c_void_p
u64p = C.POINTER(C.c_uint64)


class HostError(RuntimeError):
    pass


_typed = False


_host = None
HOST_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libii2_host.so")
# (sanitizer runs of the CPU-only file-layer tests load an instrumented build instead: make -C csrc host_asan / host_tsan)
HOST_LIB_PATH = os.environ.get("II2_HOST_LIB", HOST_LIB_PATH)


def _lib_typed():
    global _typed, _host
    if _host is None:
        _lib.load()                      # libii2_hip.so first: the host library links against it
        if not os.path.exists(HOST_LIB_PATH):
            raise RuntimeError(f"{HOST_LIB_PATH} is missing: build it with __graft_entry__.build()")
        _host = C.CDLL(HOST_LIB_PATH)
    lib = _host
    if not _typed:
        lib.ii2h_create.restype = vp
        lib.ii2h_create.argtypes = [vp, C.c_int]
        lib.ii2h_attach.restype = vp
        lib.ii2h_attach.argtypes = [vp]
        lib.ii2h_open.restype = vp
        lib.ii2h_open.argtypes = [vp, C.c_int, C.c_char_p, C.c_char_p, C.c_uint64]
        lib.ii2h_file_write.argtypes = [vp, vp, C.c_char_p, C.c_int, vp, vp, C.c_uint64, vp, vp, C.c_char_p]
        lib.ii2h_file_read.argtypes = [vp, vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_int, C.c_char_p, C.c_uint64, C.c_int, u64p]
        lib.ii2h_remove_segment.argtypes = [vp, C.c_char_p, C.c_char_p]
        lib.ii2h_terms_read.argtypes = [vp, C.c_char_p, C.c_char_p, C.POINTER(C.c_int), u64p]
        lib.ii2h_removed_write.argtypes = [vp, C.c_char_p, C.c_uint64, vp, vp, vp]
        lib.ii2h_removed_read.argtypes = [vp, C.c_char_p, u64p, u64p]
        lib.ii2h_destroy.argtypes = [vp]
        lib.ii2h_last_error.restype = C.c_char_p
        lib.ii2h_last_error.argtypes = [vp]
        lib.ii2h_put.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32]
        lib.ii2h_put_batch.argtypes = [vp, vp, vp, vp, vp, C.c_uint64]
        lib.ii2h_remove.argtypes = [vp, vp, C.c_uint64]
        lib.ii2h_merge.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]
        lib.ii2h_read.argtypes = [vp, C.c_char_p, C.c_uint64, C.c_int, C.c_char_p, C.c_uint64, C.c_int, u64p]
        lib.ii2h_prefix_search.argtypes = [vp, vp, vp, C.c_uint64, u64p]
        lib.ii2h_match_search.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, u64p]
        lib.ii2h_match_terms.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint64, u64p]
        lib.ii2h_fuzzy_search.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, u64p]
        lib.ii2h_fuzzy_terms.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, u64p]
        lib.ii2h_regex_search.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, u64p]
        lib.ii2h_regex_terms.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint64, u64p]
        lib.ii2h_intersect.argtypes = [vp, vp, vp, C.c_uint64, u64p]
        lib.ii2h_intersect_except.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, C.c_uint64, u64p]
        lib.ii2h_intersect_at_least.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64, u64p]
        lib.ii2h_intersect_top.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64, u64p]
        lib.ii2h_matched_terms.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64, u64p]
        lib.ii2h_masks_copy.argtypes = [vp, vp]
        lib.ii2h_matched_terms_batch.argtypes = [vp, vp, vp, vp, vp, vp, C.c_uint64, vp]
        lib.ii2h_masks_batch_copy.argtypes = [vp, vp]
        lib.ii2h_intersect_top_weighted.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64, u64p]
        lib.ii2h_set_resolve.argtypes = [vp, C.c_int]
        lib.ii2h_set_build.argtypes = [vp, C.c_int]
        lib.ii2h_set_first_cap.argtypes = [vp, C.c_uint64]
        lib.ii2h_second_calls.restype = C.c_uint64
        lib.ii2h_second_calls.argtypes = [vp]
        lib.ii2h_union_bound.restype = C.c_uint64
        lib.ii2h_union_bound.argtypes = [vp, C.c_uint64, vp]
        lib.ii2h_intersect_batch.argtypes = [vp, vp, vp, vp, vp, C.c_uint64, u64p]
        lib.ii2h_intersect_top_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, u64p]
        lib.ii2h_removed_values.argtypes = [vp, u64p]
        lib.ii2h_term_counts.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, C.c_uint64, u64p]
        lib.ii2h_count_term_len.restype = C.c_uint64
        lib.ii2h_count_term_len.argtypes = [vp, C.c_uint64]
        lib.ii2h_count_copy.argtypes = [vp, C.c_uint64, vp, u64p]
        lib.ii2h_histogram.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, C.c_uint64, u64p]
        lib.ii2h_hist_copy.argtypes = [vp, vp]
        lib.ii2h_term_histogram.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, C.c_uint64, u64p]
        lib.ii2h_term_hist_term_len.restype = C.c_uint64
        lib.ii2h_term_hist_term_len.argtypes = [vp, C.c_uint64]
        lib.ii2h_term_hist_copy.argtypes = [vp, C.c_uint64, vp, vp]
        for f in ("ii2h_result_term_len", "ii2h_result_values_len"):
            getattr(lib, f).restype = C.c_uint64
            getattr(lib, f).argtypes = [vp, C.c_uint64]
        lib.ii2h_result_copy.argtypes = [vp, C.c_uint64, vp, vp]
        lib.ii2h_ids_copy.argtypes = [vp, vp]
        lib.ii2h_scores_copy.argtypes = [vp, vp]
        for f in ("ii2h_segment_count", "ii2h_index_segment_count", "ii2h_shard_count"):
            getattr(lib, f).restype = C.c_uint64
            getattr(lib, f).argtypes = [vp]
        _typed = True
    return lib


def union_bound(range_seg, seg_postings) -> int:
    """For the tests, no device: the output bound prefix_search and match_search give one name whose range i lies in segment
    `range_seg[i]`, segment s holding `seg_postings[s]` postings - every distinct segment counted once, however many ranges."""
    seg = np.ascontiguousarray(list(range_seg) + [0], np.uint64)
    posts = np.ascontiguousarray(list(seg_postings) + [0], np.uint64)
    return _lib_typed().ii2h_union_bound(seg.ctypes.data, len(range_seg), posts.ctypes.data)


class _Target:
    def __init__(self, ctx: Context, is_index: bool, basedir: Optional[str] = None):
        self.lib = _lib_typed()
        self.ctx = ctx
        self.basedir = basedir
        if basedir is None:
            self.h = self.lib.ii2h_create(ctx.h if ctx is not None else None, 1 if is_index else 0)
        else:               # NewShard(basedir) / NewInvertedIndex(basedir): what the directory holds is loaded
            err = C.create_string_buffer(512)
            self.h = self.lib.ii2h_open(ctx.h, 1 if is_index else 0, os.fsencode(basedir), err, len(err))
            if not self.h:
                raise HostError(err.value.decode())

    def _ck(self, rc: int) -> None:
        if rc:
            raise HostError((self.lib.ii2h_last_error(self.h) or b"").decode())

    def session(self):
        """Another handle on the same shard / index for use from another thread: the operations are thread-safe (like the
        reference's goroutine-safe methods), a handle's result buffers are per handle."""
        other = object.__new__(type(self))
        other.lib, other.ctx, other.basedir = self.lib, self.ctx, self.basedir
        other.h = self.lib.ii2h_attach(self.h)
        return other

    def close(self) -> None:
        if self.h:
            self.lib.ii2h_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.ctx is None or self.ctx.h:
                self.close()
        except Exception:
            pass

    def put(self, terms: List[bytes], val: int) -> None:
        blob, off = _flat(list(terms))
        self._ck(self.lib.ii2h_put(self.h, blob.ctypes.data, off.ctypes.data, len(terms), val))

    def set_build(self, mode: int) -> None:
        """Where put_batch sorts, deduplicates and looks up its terms (SetBuild): 0 on the host, 1 on the device (ii2_dict_build;
        the built dictionary stays resident with the segment), -1 (the default) decides by the batch's size.  A batch with a term
        above 256 bytes takes the host route under every mode.  The segment and its files are the same either way."""
        self._ck(self.lib.ii2h_set_build(self.h, int(mode)))

    def put_batch(self, docs: List[Tuple[List[bytes], int]]) -> None:
        """Many puts at once, docs = [(terms, val), ...]: one merged-quality segment per shard that receives a term (PutBatch:
        one ii2_seg_build call each) instead of one direct segment per put."""
        docs = [(list(terms), int(val)) for terms, val in docs]
        blob, off = _flat([t for terms, _ in docs for t in terms])
        doc_first = np.zeros(len(docs) + 1, np.uint64)
        if docs:
            doc_first[1:] = np.cumsum([len(terms) for terms, _ in docs])
        vals = np.array([val for _, val in docs] + [0], np.uint32)
        self._ck(self.lib.ii2h_put_batch(self.h, blob.ctypes.data, off.ctypes.data, doc_first.ctypes.data, vals.ctypes.data, len(docs)))

    def _results(self, n: int) -> List[Tuple[bytes, List[int]]]:
        out = []
        for i in range(n):
            tl = self.lib.ii2h_result_term_len(self.h, i)
            vl = self.lib.ii2h_result_values_len(self.h, i)
            tb = np.zeros(max(tl, 1), np.uint8)
            vb = np.zeros(max(vl, 1), np.uint32)
            self.lib.ii2h_result_copy(self.h, i, tb.ctypes.data, vb.ctypes.data)
            out.append((tb[:tl].tobytes(), vb[:vl].tolist()))
        return out

    def read(self, lo: Optional[bytes] = None, hi: Optional[bytes] = None):
        n = C.c_uint64()
        self._ck(self.lib.ii2h_read(self.h, lo or b"", len(lo or b""), lo is not None, hi or b"", len(hi or b""), hi is not None,
                                    C.byref(n)))
        return self._results(n.value)

    def _merge(self, req: int, m: int, conc: int) -> int:
        out = C.c_int64()
        self._ck(self.lib.ii2h_merge(self.h, req, m, conc, C.byref(out)))
        return out.value

    def _remove(self, values) -> None:
        v = np.ascontiguousarray(values, dtype=np.uint32)
        self._ck(self.lib.ii2h_remove(self.h, v.ctypes.data, v.size))

    def match_search(self, patterns: List[bytes], kind: int = 0) -> Dict[bytes, List[int]]:
        """Substring, suffix and wildcard search (MatchSearch): {pattern: ids under any term it matches}, over every segment (of
        every shard); a pattern that matches no term has no entry.  kind: II2_MATCH_CONTAINS (0) / SUFFIX (1) / GLOB (2),
        optionally | II2_MATCH_NOCASE (0x80) and / or II2_MATCH_UTF8 (0x08: `?` and `*` take whole UTF-8 symbols), for all the
        patterns; any number of patterns (the device call takes 64 at a time).  Like read, no tombstone filter."""
        blob, off = _flat(list(patterns))
        n = C.c_uint64()
        self._ck(self.lib.ii2h_match_search(self.h, blob.ctypes.data, off.ctypes.data, len(patterns), int(kind), C.byref(n)))
        return dict(self._results(n.value))

    def match_terms(self, pattern: bytes, kind: int = 0, limit: int = 1 << 62) -> List[bytes]:
        """The distinct terms the pattern matches (MatchTerms), in byte order, at most `limit`."""
        pat = np.frombuffer(bytes(pattern) + b"\0", np.uint8).copy()
        n = C.c_uint64()
        self._ck(self.lib.ii2h_match_terms(self.h, pat.ctypes.data, len(pattern), int(kind), int(limit), C.byref(n)))
        return [t for t, _ in self._results(n.value)]

    def fuzzy_search(self, terms: List[bytes], max_dist: int, prefix: int = 0, flags: int = 0) -> Dict[bytes, List[int]]:
        """Typo-tolerant search (FuzzySearch): {query term: ids under any term within `max_dist` edits of it}, over every segment
        (of every shard); a query term that matches nothing has no entry.  prefix: leading bytes a term must share with the query
        term (a shorter query term is compared as a whole); flags: II2_FUZZY_TRANSPOSE (1), II2_MATCH_NOCASE (0x80) and / or II2_MATCH_UTF8
        (0x08: edits, prefix and the clamp of a shorter query term count UTF-8 symbols, not bytes); any
        number of query terms (the device call takes 16 at a time).  Like read, no tombstone filter."""
        blob, off = _flat(list(terms))
        n = C.c_uint64()
        self._ck(self.lib.ii2h_fuzzy_search(self.h, blob.ctypes.data, off.ctypes.data, len(terms), int(max_dist), int(prefix), int(flags), C.byref(n)))
        return dict(self._results(n.value))

    def fuzzy_terms(self, pattern: bytes, max_dist: int, prefix: int = 0, flags: int = 0, limit: int = 1 << 62) -> List[Tuple[bytes, int]]:
        """The distinct terms within `max_dist` edits of the pattern with their distances (FuzzyTerms): [(term, distance), ...],
        distance ascending, then in byte order, at most `limit`."""
        pat = np.frombuffer(bytes(pattern) + b"\0", np.uint8).copy()
        n = C.c_uint64()
        self._ck(self.lib.ii2h_fuzzy_terms(self.h, pat.ctypes.data, len(pattern), int(max_dist), int(prefix), int(flags), int(limit), C.byref(n)))
        return [(t, v[0]) for t, v in self._results(n.value)]

    def regex_search(self, patterns: List[bytes], flags: int = 0) -> Dict[bytes, List[int]]:
        """Regular-expression search (RegexSearch): {pattern: ids under any term the pattern matches as a whole}, over every
        segment (of every shard); a pattern that matches no term has no entry.  The syntax is include/ii2.h's (a subset of
        Python's `re` on bytes with re.DOTALL; at most 256 bytes and 64 positions a pattern); flags: 0 or II2_MATCH_NOCASE (0x80)
        for all the patterns; any number of patterns (the device call takes 8 at a time).  A pattern that does not parse fails
        the whole call, before any search runs.  Like read, no tombstone filter."""
        blob, off = _flat(list(patterns))
        n = C.c_uint64()
        self._ck(self.lib.ii2h_regex_search(self.h, blob.ctypes.data, off.ctypes.data, len(patterns), int(flags), C.byref(n)))
        return dict(self._results(n.value))

    def regex_terms(self, pattern: bytes, flags: int = 0, limit: int = 1 << 62) -> List[bytes]:
        """The distinct terms the regular expression matches (RegexTerms), in byte order, at most `limit`."""
        pat = np.frombuffer(bytes(pattern) + b"\0", np.uint8).copy()
        n = C.c_uint64()
        self._ck(self.lib.ii2h_regex_terms(self.h, pat.ctypes.data, len(pattern), int(flags), int(limit), C.byref(n)))
        return [t for t, _ in self._results(n.value)]

    def removed_values(self) -> List[int]:
        n = C.c_uint64()
        self._ck(self.lib.ii2h_removed_values(self.h, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint32)
        self.lib.ii2h_ids_copy(self.h, out.ctypes.data)
        return out[: n.value].tolist()


class Shard(_Target):
    """shard.go: Put / Read / Remove / Merge.  With `basedir` the shard lives in that directory (segment files and
    removed.list, host/segment_file.h) and a new Shard on the same directory picks the state up (shard.go:300-358)."""

    def __init__(self, ctx: Context, basedir: Optional[str] = None):
        super().__init__(ctx, False, basedir)

    def merge(self, req_count: int, m_count: int) -> int:
        return self._merge(req_count, m_count, 1)

    def remove(self, values) -> None:
        self._remove(values)

    @property
    def n_segments(self) -> int:
        return self.lib.ii2h_segment_count(self.h)


class InvertedIndex(_Target):
    """inverted_index.go: Put / Read / Merge / PutRemoved / PrefixSearch (+ Intersect, IntersectExcept, IntersectAtLeast, IntersectTop, IntersectTopWeighted, IntersectTopBatch, IntersectMany, TermCounts, Histogram, TermHistogram, MatchedTerms, MatchedTermsBatch)."""

    def __init__(self, ctx: Context, basedir: Optional[str] = None):
        super().__init__(ctx, True, basedir)

    def merge(self, req_count: int, m_count: int, concurrency: int = 1) -> int:
        return self._merge(req_count, m_count, concurrency)

    def put_removed(self, values) -> None:
        self._remove(values)

    def set_resolve(self, mode: int) -> None:
        """How intersect_many, intersect_top_batch and matched_terms_batch turn their terms into lists (SetResolve): 0 bisects the host dictionaries,
        1 probes resident dictionaries on the device (ii2_dict_find), -1 (the default) decides by the call's size.  The results
        are the same in every mode."""
        self._ck(self.lib.ii2h_set_resolve(self.h, int(mode)))

    def set_first_cap(self, ids: int) -> None:
        """For the tests: the first buffer of every call that may need a second one holds at most `ids` ids (SetFirstCap: 1 to
        2**22, the default), so that a small index reaches the second call."""
        self._ck(self.lib.ii2h_set_first_cap(self.h, int(ids)))

    @property
    def second_calls(self) -> int:
        """How many calls on this index have been made a second time because the first buffer was too small."""
        return self.lib.ii2h_second_calls(self.h)

    def prefix_search(self, prefixes: List[bytes]) -> Dict[bytes, List[int]]:
        blob, off = _flat(list(prefixes))
        n = C.c_uint64()
        self._ck(self.lib.ii2h_prefix_search(self.h, blob.ctypes.data, off.ctypes.data, len(prefixes), C.byref(n)))
        return dict(self._results(n.value))

    def intersect(self, terms: List[bytes]) -> List[int]:
        blob, off = _flat(list(terms))
        n = C.c_uint64()
        self._ck(self.lib.ii2h_intersect(self.h, blob.ctypes.data, off.ctypes.data, len(terms), C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint32)
        self.lib.ii2h_ids_copy(self.h, out.ctypes.data)
        return out[: n.value].tolist()

    def intersect_except(self, terms: List[bytes], exclude: List[bytes]) -> List[int]:
        """ids under every term of `terms` and under no term of `exclude` (IntersectExcept: one ii2_andnot_ranges call)."""
        blob, off = _flat(list(terms))
        x_blob, x_off = _flat(list(exclude))
        n = C.c_uint64()
        self._ck(self.lib.ii2h_intersect_except(self.h, blob.ctypes.data, off.ctypes.data, len(terms), x_blob.ctypes.data, x_off.ctypes.data,
                                                len(exclude), C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint32)
        self.lib.ii2h_ids_copy(self.h, out.ctypes.data)
        return out[: n.value].tolist()

    def intersect_at_least(self, terms: List[bytes], min_match: int, exclude: List[bytes] = ()) -> List[int]:
        """ids under at least `min_match` of `terms` and under no term of `exclude` (IntersectAtLeast: one ii2_atleast_ranges call);
        a term found in no segment matches no doc."""
        blob, off = _flat(list(terms))
        x_blob, x_off = _flat(list(exclude))
        n = C.c_uint64()
        self._ck(self.lib.ii2h_intersect_at_least(self.h, blob.ctypes.data, off.ctypes.data, len(terms), int(min_match), x_blob.ctypes.data,
                                                  x_off.ctypes.data, len(exclude), C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint32)
        self.lib.ii2h_ids_copy(self.h, out.ctypes.data)
        return out[: n.value].tolist()

    def intersect_top(self, terms: List[bytes], k: int, min_match: int = 1, exclude: List[bytes] = ()) -> List[Tuple[int, int]]:
        """the `k` ids under the most of `terms` - at least `min_match` of them, under no term of `exclude` - as (id, score) pairs,
        score descending, then id ascending (IntersectTop: one ii2_topk_ranges call); a term found in no segment matches no doc."""
        blob, off = _flat(list(terms))
        x_blob, x_off = _flat(list(exclude))
        n = C.c_uint64()
        self._ck(self.lib.ii2h_intersect_top(self.h, blob.ctypes.data, off.ctypes.data, len(terms), int(k), int(min_match), x_blob.ctypes.data,
                                             x_off.ctypes.data, len(exclude), C.byref(n)))
        ids, scores = np.zeros(max(n.value, 1), np.uint32), np.zeros(max(n.value, 1), np.uint32)
        self.lib.ii2h_ids_copy(self.h, ids.ctypes.data)
        self.lib.ii2h_scores_copy(self.h, scores.ctypes.data)
        return list(zip(ids[: n.value].tolist(), scores[: n.value].tolist()))

    def matched_terms(self, ids, terms: List[bytes]) -> np.ndarray:
        """which of `terms` each of `ids` lies under (MatchedTerms: one ii2_explain_ranges call): a uint64 array of shape (len(ids),
        ceil(len(terms) / 64)), bit j & 63 of word [i, j >> 6] set when ids[i] lies under terms[j].  ids in any order - an ascending
        result or intersect_top's ranked page; an id given twice has its bits in its first row and zeros after; a term found in no
        segment never has its bit set."""
        ids = np.ascontiguousarray(ids, np.uint32)
        blob, off = _flat(list(terms))
        nw = C.c_uint64()
        self._ck(self.lib.ii2h_matched_terms(self.h, ids.ctypes.data, ids.size, blob.ctypes.data, off.ctypes.data, len(terms), C.byref(nw)))
        out = np.zeros(max(ids.size * nw.value, 1), np.uint64)
        self.lib.ii2h_masks_copy(self.h, out.ctypes.data)
        return out[: ids.size * nw.value].reshape(ids.size, nw.value)

    def matched_terms_batch(self, pages) -> List[np.ndarray]:
        """matched_terms for many pages = [(ids, terms), ...] in one device call (MatchedTermsBatch: one upload of all ids, ONE
        ii2_explain_batch call, one download): result p equals matched_terms(*pages[p])."""
        pages = [(np.ascontiguousarray(ids, np.uint32), list(terms)) for ids, terms in pages]
        ids = np.concatenate([i for i, _ in pages] + [np.zeros(1, np.uint32)])              # (never an empty array)
        ids_off = np.cumsum([0] + [i.size for i, _ in pages]).astype(np.uint64)
        blob, off = _flat([t for _, terms in pages for t in terms])
        term_first = np.cumsum([0] + [len(terms) for _, terms in pages]).astype(np.uint64)
        words_off = np.zeros(len(pages) + 1, np.uint64)
        self._ck(self.lib.ii2h_matched_terms_batch(self.h, ids.ctypes.data, ids_off.ctypes.data, blob.ctypes.data, off.ctypes.data,
                                                   term_first.ctypes.data, len(pages), words_off.ctypes.data))
        out = np.zeros(max(int(words_off[-1]), 1), np.uint64)
        self.lib.ii2h_masks_batch_copy(self.h, out.ctypes.data)
        return [out[int(words_off[p]): int(words_off[p + 1])].reshape(i.size, (len(terms) + 63) // 64) for p, (i, terms) in enumerate(pages)]

    def intersect_top_weighted(self, terms: List[bytes], weights: List[int], k: int, min_score: int = 1,
                               exclude: List[bytes] = ()) -> List[Tuple[int, int]]:
        """intersect_top with a weight per term: a doc's score is the sum of `weights[i]` (1 .. 255 each, at most 255 together) over
        the `terms[i]` it lies under, at least `min_score` (IntersectTopWeighted: one ii2_topk_weighted_ranges call); a term found
        in no segment keeps its slot and matches no doc."""
        if len(weights) != len(terms):
            raise ValueError("intersect_top_weighted: one weight per term")
        blob, off = _flat(list(terms))
        x_blob, x_off = _flat(list(exclude))
        w = np.asarray(list(weights) + [0], np.uint32)
        n = C.c_uint64()
        self._ck(self.lib.ii2h_intersect_top_weighted(self.h, blob.ctypes.data, off.ctypes.data, len(terms), w.ctypes.data, int(k), int(min_score),
                                                      x_blob.ctypes.data, x_off.ctypes.data, len(exclude), C.byref(n)))
        ids, scores = np.zeros(max(n.value, 1), np.uint32), np.zeros(max(n.value, 1), np.uint32)
        self.lib.ii2h_ids_copy(self.h, ids.ctypes.data)
        self.lib.ii2h_scores_copy(self.h, scores.ctypes.data)
        return list(zip(ids[: n.value].tolist(), scores[: n.value].tolist()))

    def intersect_batch(self, queries) -> List[List[int]]:
        """Many intersect_except queries, queries = [(terms, exclude), ...], in one device call (IntersectMany: one
        ii2_query_batch_groups call - a second one when the results exceed its first buffer - and one download); result q is
        that of intersect_except(*queries[q])."""
        queries = [(list(t), list(x)) for t, x in queries]
        blob, off = _flat([term for t, x in queries for term in t + x])
        q_first = np.zeros(len(queries) + 1, np.uint64)
        q_first[1:] = np.cumsum([len(t) + len(x) for t, x in queries], dtype=np.uint64) if queries else []
        q_req = np.array([len(t) for t, _ in queries], np.uint64)
        n = C.c_uint64()
        self._ck(self.lib.ii2h_intersect_batch(self.h, blob.ctypes.data, off.ctypes.data, q_first.ctypes.data, q_req.ctypes.data, len(queries),
                                               C.byref(n)))
        return [vals for _, vals in self._results(n.value)]

    def intersect_top_batch(self, queries) -> List[List[Tuple[int, int]]]:
        """Many intersect_top_weighted queries, queries = [(terms, weights, k, min_score, exclude), ...], in one device call
        (IntersectTopBatch: one ii2_topk_batch call - a second one when the results exceed its first buffer - and one download);
        result q is that of intersect_top_weighted(*queries[q])."""
        queries = [(list(t), list(w), int(k), int(m), list(x)) for t, w, k, m, x in queries]
        for q, (t, w, _, _, _) in enumerate(queries):
            if len(w) != len(t):
                raise ValueError(f"intersect_top_batch: query {q}: one weight per term")
        blob, off = _flat([term for t, _, _, _, x in queries for term in t + x])
        q_first = np.zeros(len(queries) + 1, np.uint64)
        q_first[1:] = np.cumsum([len(t) + len(x) for t, _, _, _, x in queries], dtype=np.uint64) if queries else []
        q_req = np.array([len(t) for t, _, _, _, _ in queries], np.uint64)
        w = np.asarray([x for _, ws, _, _, _ in queries for x in ws] + [0], np.uint32)
        k = np.asarray([k for _, _, k, _, _ in queries] + [0], np.uint64)
        m = np.asarray([m for _, _, _, m, _ in queries] + [0], np.uint32)
        n = C.c_uint64()
        self._ck(self.lib.ii2h_intersect_top_batch(self.h, blob.ctypes.data, off.ctypes.data, q_first.ctypes.data, q_req.ctypes.data, w.ctypes.data,
                                                   k.ctypes.data, m.ctypes.data, len(queries), C.byref(n)))
        ids = [vals for _, vals in self._results(n.value)]
        scores = np.zeros(max(sum(len(v) for v in ids), 1), np.uint32)
        self.lib.ii2h_scores_copy(self.h, scores.ctypes.data)
        out, at = [], 0
        for v in ids:
            out.append(list(zip(v, scores[at:at + len(v)].tolist())))
            at += len(v)
        return out

    def term_counts(self, prefix: bytes, terms: List[bytes] = (), exclude: List[bytes] = ()) -> Dict[bytes, int]:
        """Facet counts (TermCounts: the filter stays on the device, one ii2_count_ranges call over the prefix's run of every
        segment): for every term that starts with `prefix`, the number of distinct docs under it among
        intersect_except(terms, exclude); terms with count 0 are left out.  Without `terms` the doc set is every doc: the
        document frequency of each term under the prefix."""
        blob, off = _flat(list(terms))
        x_blob, x_off = _flat(list(exclude))
        pre = np.frombuffer(bytes(prefix) + b"\0", dtype=np.uint8).copy()
        n = C.c_uint64()
        self._ck(self.lib.ii2h_term_counts(self.h, pre.ctypes.data, len(prefix), blob.ctypes.data, off.ctypes.data, len(terms), x_blob.ctypes.data,
                                           x_off.ctypes.data, len(exclude), C.byref(n)))
        out = {}
        for i in range(n.value):
            tl = self.lib.ii2h_count_term_len(self.h, i)
            tb = np.zeros(max(tl, 1), np.uint8)
            c = C.c_uint64()
            self.lib.ii2h_count_copy(self.h, i, tb.ctypes.data, C.byref(c))
            out[tb[:tl].tobytes()] = c.value
        return out

    def histogram(self, terms: List[bytes], edges, exclude: List[bytes] = ()) -> np.ndarray:
        """The date histogram of a query (Histogram: the result stays on the device, one ii2_histogram_ids call): uint64
        [n_buckets], how many ids of intersect_except(terms, exclude) fall into each bucket edges[b] <= id < edges[b + 1] of the
        n_buckets + 1 strictly ascending `edges` (each <= 2^32); ids outside the axis are counted nowhere."""
        blob, off = _flat(list(terms))
        x_blob, x_off = _flat(list(exclude))
        e = np.ascontiguousarray(np.asarray(edges, dtype=np.uint64).ravel())
        n = C.c_uint64()
        self._ck(self.lib.ii2h_histogram(self.h, blob.ctypes.data, off.ctypes.data, len(terms), x_blob.ctypes.data, x_off.ctypes.data, len(exclude),
                                         e.ctypes.data, e.size, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint64)
        self.lib.ii2h_hist_copy(self.h, out.ctypes.data)
        return out[: n.value]

    def term_histogram(self, prefix: bytes, edges, terms: List[bytes] = (), exclude: List[bytes] = ()) -> Dict[bytes, np.ndarray]:
        """Terms over time (TermHistogram: one ii2_histogram_ranges call over the prefix's run of every segment): term_counts per
        bucket of `edges` - for every term that starts with `prefix` a uint64 [n_buckets] row, the distinct docs under it among
        intersect_except(terms, exclude) per bucket; terms with an all-zero row are left out.  Without `terms` the doc set is
        every doc: each term's frequency over the value axis."""
        blob, off = _flat(list(terms))
        x_blob, x_off = _flat(list(exclude))
        pre = np.frombuffer(bytes(prefix) + b"\0", dtype=np.uint8).copy()
        e = np.ascontiguousarray(np.asarray(edges, dtype=np.uint64).ravel())
        n = C.c_uint64()
        self._ck(self.lib.ii2h_term_histogram(self.h, pre.ctypes.data, len(prefix), blob.ctypes.data, off.ctypes.data, len(terms), x_blob.ctypes.data,
                                              x_off.ctypes.data, len(exclude), e.ctypes.data, e.size, C.byref(n)))
        out = {}
        for i in range(n.value):
            tl = self.lib.ii2h_term_hist_term_len(self.h, i)
            tb = np.zeros(max(tl, 1), np.uint8)
            row = np.zeros(max(e.size - 1, 1), np.uint64)
            self.lib.ii2h_term_hist_copy(self.h, i, tb.ctypes.data, row.ctypes.data)
            out[tb[:tl].tobytes()] = row[: e.size - 1]
        return out

    @property
    def n_shards(self) -> int:
        return self.lib.ii2h_shard_count(self.h)

    @property
    def n_segments(self) -> int:
        """Segments of all shards together (a shard exists once it has received a term)."""
        return self.lib.ii2h_index_segment_count(self.h)


class SegmentFiles(_Target):
    """file.Writer / file.Reader / file.RemoveSegment (file/writer.go, file/reader.go) over host/segment_file.h: the
    encode and decode steps run on the device."""

    def __init__(self, ctx: Context):
        super().__init__(ctx, False)

    def write(self, directory: str, term_values: List[Tuple[bytes, List[int]]], direct: bool = False) -> str:
        """NewWriter / NewDirectWriter + Append for every (term, values) + Close; returns GetKey()."""
        blob, off = _flat([t for t, _ in term_values])
        po = np.zeros(len(term_values) + 1, np.uint64)
        if term_values:
            po[1:] = np.cumsum([len(v) for _, v in term_values])
        flat = np.ascontiguousarray([x for _, v in term_values for x in v] + [0], dtype=np.uint32)
        key = C.create_string_buffer(32)
        if self.ctx is None and not direct:
            raise HostError("writer: the encode step needs a device context")
        self._ck(self.lib.ii2h_file_write(self.h, self.ctx.h if self.ctx is not None else None, os.fsencode(directory), 1 if direct else 0,
                                          blob.ctypes.data, off.ctypes.data, len(term_values), po.ctypes.data, flat.ctypes.data, key))
        return key.value.decode()

    def write_arrays(self, directory: str, term_blob: np.ndarray, term_off: np.ndarray, post_off: np.ndarray, values: np.ndarray) -> str:
        """write() for callers that already hold flat arrays (terms: bytes + u64 offsets; lists: u64 offsets + u32 ids)."""
        key = C.create_string_buffer(32)
        term_blob = np.ascontiguousarray(term_blob, np.uint8)
        term_off = np.ascontiguousarray(term_off, np.uint64)
        post_off = np.ascontiguousarray(post_off, np.uint64)
        values = np.ascontiguousarray(values, np.uint32)
        self._ck(self.lib.ii2h_file_write(self.h, self.ctx.h, os.fsencode(directory), 0, term_blob.ctypes.data, term_off.ctypes.data,
                                          term_off.size - 1, post_off.ctypes.data, values.ctypes.data, key))
        return key.value.decode()

    def read_count(self, directory: str, key: str) -> Tuple[int, int]:
        """Reads and decodes a whole segment; returns (terms, postings) without copying the lists into Python."""
        n = C.c_uint64()
        self._ck(self.lib.ii2h_file_read(self.h, self.ctx.h, os.fsencode(directory), key.encode(), b"", 0, 0, b"", 0, 0, C.byref(n)))
        return n.value, sum(self.lib.ii2h_result_values_len(self.h, i) for i in range(0, n.value, max(n.value // 1000, 1)))

    def read(self, directory: str, key: str, lo: Optional[bytes] = None, hi: Optional[bytes] = None):
        """NewReader(dir, key, min, max) drained with Next(); None when the segment has nothing in range."""
        n = C.c_uint64()
        rc = self.lib.ii2h_file_read(self.h, self.ctx.h, os.fsencode(directory), key.encode(), lo or b"", len(lo or b""), lo is not None,
                                     hi or b"", len(hi or b""), hi is not None, C.byref(n))
        if rc == 1:
            return None
        self._ck(rc)
        return self._results(n.value)

    def remove(self, directory: str, key: str) -> None:
        self._ck(self.lib.ii2h_remove_segment(self.h, os.fsencode(directory), key.encode()))

    # ---- the parts of the file layer that involve no device (usable with ctx = None) ----
    def read_terms(self, directory: str, key: str):
        """The term dictionary file alone: (direct, [(term, [value] if direct else [])])."""
        n, direct = C.c_uint64(), C.c_int()
        self._ck(self.lib.ii2h_terms_read(self.h, os.fsencode(directory), key.encode(), C.byref(direct), C.byref(n)))
        return bool(direct.value), self._results(n.value)

    def write_removed(self, directory: str, batches: Dict[int, List[int]]) -> None:
        ts = np.ascontiguousarray(sorted(batches), dtype=np.int64)
        off = np.zeros(ts.size + 1, np.uint64)
        off[1:] = np.cumsum([len(batches[int(t)]) for t in ts])
        vals = np.ascontiguousarray([v for t in ts for v in batches[int(t)]] + [0], dtype=np.uint32)
        self._ck(self.lib.ii2h_removed_write(self.h, os.fsencode(directory), ts.size, ts.ctypes.data, off.ctypes.data, vals.ctypes.data))

    def read_removed(self, directory: str) -> Tuple[int, List[int]]:
        """(batches, RemovedLists.Values()) of the directory's removed.list; (0, []) when there is none."""
        nb, n = C.c_uint64(), C.c_uint64()
        self._ck(self.lib.ii2h_removed_read(self.h, os.fsencode(directory), C.byref(nb), C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint32)
        self.lib.ii2h_ids_copy(self.h, out.ctypes.data)
        return nb.value, out[: n.value].tolist()
