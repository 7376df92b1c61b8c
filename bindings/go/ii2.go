// Package gpu binds the posting-list hot path of lezhnev74/inverted_index_2 to libii2_hip.so
// (include/ii2.h) through cgo.  It replaces bodies, not signatures: the reference's exported
// API (inverted_index.go, shard.go) keeps its shape; see index.go for the drop-in methods.
//
// This image has no Go toolchain, so the package has never been compiled here; the same
// entry points are exercised through ctypes by the repository's -m gpu tests.
//
// cgo rules honoured: only flat slices cross (no Go pointer to Go pointer), buffers are pinned
// for the duration of one call, the library retains nothing.
package gpu

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../inverted_index_2_amd -lii2_hip -Wl,-rpath,${SRCDIR}/../../inverted_index_2_amd
#include "ii2.h"
*/
import "C"

import (
	"fmt"
	"unsafe"
)

// Ctx is one GPU + one HIP stream.  Calls on a Ctx are serialised by the library; give every
// worker goroutine of InvertedIndex.Merge its own Ctx (inverted_index.go:83-103).  Segments and
// tombstone bitmaps belong to the device and may be shared by all Ctx of that device.
type Ctx struct{ h *C.ii2_ctx }

func NewCtx(device int) (*Ctx, error) {
	var h *C.ii2_ctx
	if rc := C.ii2_ctx_create(C.int(device), 0, &h); rc != 0 {
		return nil, fmt.Errorf("gpu: ctx: %s (%d)", C.GoString(C.ii2_last_error(nil)), int(rc))
	}
	return &Ctx{h}, nil
}

func (c *Ctx) Close()      { C.ii2_ctx_destroy(c.h) }
func (c *Ctx) Device() int { return int(C.ii2_ctx_device(c.h)) }

// Counters reports how often this context repeated a call on its second path because a bounded wait between workgroups of
// one launch ran out (merges on the packing path; two-list ANDs / segment encodes without a look-back).  Results are identical
// either way; a non-zero count on production hardware is worth a bug report.
func (c *Ctx) Counters() (mergeRepeats, lookbackRepeats uint64) {
	var out [2]C.uint64_t
	C.ii2_ctx_counters(c.h, &out[0], 2)
	return uint64(out[0]), uint64(out[1])
}

func (c *Ctx) err(what string, rc C.int) error {
	return fmt.Errorf("gpu: %s: %s (%d)", what, C.GoString(C.ii2_last_error(c.h)), int(rc))
}

func u32ptr(s []uint32) *C.uint32_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint32_t)(unsafe.Pointer(&s[0]))
}
func u64ptr(s []uint64) *C.uint64_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint64_t)(unsafe.Pointer(&s[0]))
}

// Segment is a device-resident DV1 segment (the encode step, file/writer.go:32-59).
type Segment struct{ h *C.ii2_seg }

// Encode uploads nLists posting lists given CSR-style (postOff[nLists+1] into values).
func (c *Ctx) Encode(postOff []uint64, values []uint32) (*Segment, error) {
	var s *C.ii2_seg
	if rc := C.ii2_seg_encode(c.h, C.uint64_t(len(postOff)-1), u64ptr(postOff), u32ptr(values), C.II2_HOST, &s); rc != 0 {
		return nil, c.err("encode", rc)
	}
	return &Segment{s}, nil
}

// BuildStats mirrors ii2_build_stats.
type BuildStats struct {
	Pairs, Postings, NonEmpty uint64
	Passes                    uint32
}

// SegBuild is the build step (ii2_seg_build): ONE segment of nLists lists from (list, value) pairs in any order, repeats
// allowed - list t ends up holding, ascending and duplicate-free, every values[i] with listID[i] == t.  It replaces N calls of
// Shard.Put (shard.go:33-67) and the merges that fold their direct segments (shard.go:163-212); no tombstone filter, as in Put.
// A listID >= nLists is an error and leaves nothing allocated.
func (c *Ctx) SegBuild(nLists uint64, listID, values []uint32) (*Segment, BuildStats, error) {
	if len(listID) != len(values) {
		return nil, BuildStats{}, fmt.Errorf("gpu: build: %d list ids for %d values", len(listID), len(values))
	}
	var s *C.ii2_seg
	var st C.ii2_build_stats
	if rc := C.ii2_seg_build(c.h, C.uint64_t(nLists), C.uint64_t(len(listID)), u32ptr(listID), u32ptr(values), C.II2_HOST, &s, &st); rc != 0 {
		return nil, BuildStats{}, c.err("build", rc)
	}
	return &Segment{s}, BuildStats{uint64(st.n_pairs), uint64(st.n_postings), uint64(st.n_nonempty), uint32(st.n_passes)}, nil
}

// Decode is the decode step (file/reader.go:79-100).
func (c *Ctx) Decode(s *Segment) (postOff []uint64, values []uint32, err error) {
	var info C.ii2_seg_info
	C.ii2_seg_get_info(s.h, &info)
	postOff = make([]uint64, uint64(info.n_lists)+1)
	values = make([]uint32, uint64(info.n_postings))
	if rc := C.ii2_seg_decode(c.h, s.h, u64ptr(postOff), u32ptr(values), C.II2_HOST); rc != 0 {
		return nil, nil, c.err("decode", rc)
	}
	return postOff, values, nil
}

// SegMeta holds the arrays the library derives when a segment is made (ii2_seg_export_meta): postings and last doc per list,
// the owner of every block (0xFFFFFFFF: none of a view's lists, and the entry past the last block) and - when the segment has
// the host mirror - {first doc, first doc of the last block, last doc} per list as the path choice reads it.
type SegMeta struct {
	Cnt, LastDoc, BlkList, Spans []uint32 // Spans is nil when SpansMirrored is false
	IsView, SpansMirrored        bool
	MergeBlocks, MergeBytes      uint64
	Postings                     uint64
}

// Meta copies a segment's derived arrays to the host (one wait, no kernel).
func (c *Ctx) Meta(s *Segment) (*SegMeta, error) {
	var info C.ii2_seg_info
	C.ii2_seg_get_info(s.h, &info)
	m := &SegMeta{Cnt: make([]uint32, uint64(info.n_lists)), LastDoc: make([]uint32, uint64(info.n_lists)),
		BlkList: make([]uint32, uint64(info.n_blocks)+1), Spans: make([]uint32, 3*uint64(info.n_lists))}
	var mi C.ii2_seg_meta_info
	if rc := C.ii2_seg_export_meta(c.h, s.h, u32ptr(m.Cnt), u32ptr(m.LastDoc), u32ptr(m.BlkList), u32ptr(m.Spans), &mi); rc != 0 {
		return nil, c.err("export meta", rc)
	}
	m.IsView, m.SpansMirrored = mi.is_view != 0, mi.spans_mirrored != 0
	m.MergeBlocks, m.MergeBytes, m.Postings = uint64(mi.merge_blocks), uint64(mi.merge_bytes), uint64(mi.n_postings)
	if !m.SpansMirrored {
		m.Spans = nil
	}
	return m, nil
}

// DenseForm reports the bitmap a two-list AND has cached for list i (ii2_seg_dense_form): present, its origin and word count,
// and the bytes held by all forms of the segment's store.  It builds nothing.
func (c *Ctx) DenseForm(s *Segment, i uint64) (present bool, origin, nWords, storeBytes uint64, err error) {
	var info [4]C.uint64_t
	if rc := C.ii2_seg_dense_form(c.h, s.h, C.uint64_t(i), &info[0], nil, 0); rc != 0 {
		return false, 0, 0, 0, c.err("dense form", rc)
	}
	return info[0] != 0, uint64(info[1]), uint64(info[2]), uint64(info[3]), nil
}

func (s *Segment) Free() { C.ii2_seg_free(s.h); s.h = nil }

// MergeAligned replaces the loop of Shard.Merge (shard.go:163-212) for k term-aligned segments
// held in host memory.  segOff: k*(nTerms+1) offsets (per segment, into that segment's slice of
// values); segBase: k+1 starts of the segments' slices in values; removed: RemovedLists.Values().
// A term with outOff[t+1]==outOff[t] has no survivors and is dropped by the caller
// (shard.go:192-194); termsOut == 0 means "write no segment" (shard.go:219-225).
func (c *Ctx) MergeAligned(k int, nTerms uint64, segOff, segBase []uint64, values, removed []uint32) (outOff []uint64, outVals []uint32, termsOut uint64, err error) {
	outOff = make([]uint64, nTerms+1)
	outVals = make([]uint32, len(values)+1)
	var st C.ii2_merge_stats
	rc := C.ii2_merge_host(c.h, C.uint32_t(k), C.uint64_t(nTerms), u64ptr(segOff), u64ptr(segBase), u32ptr(values),
		u32ptr(removed), C.uint64_t(len(removed)), u64ptr(outOff), u32ptr(outVals), C.uint64_t(len(outVals)), &st)
	if rc != 0 {
		return nil, nil, 0, c.err("merge", rc)
	}
	return outOff, outVals[:st.n_out], uint64(st.n_terms_out), nil
}

// Alignment is the device-resident result of AlignTerms.
type Alignment struct {
	h      *C.ii2_align
	NUnion uint64
	K      int
}

// AlignTerms replaces the k-way term-dictionary walk of makeIterator (shard.go:253-278,
// bytes.Compare order of file/types.go:24-26) with one call: the k sorted dictionaries are
// given flat (termBytes, termOff[nAll+1], segFirst[k+1] = index in termOff of each
// dictionary's first term); the union dictionary and the per-segment mapping stay on the GPU.
func (c *Ctx) AlignTerms(termBytes []byte, termOff []uint64, segFirst []uint64) (*Alignment, error) {
	var tb *C.uint8_t
	if len(termBytes) > 0 {
		tb = (*C.uint8_t)(unsafe.Pointer(&termBytes[0]))
	}
	var a *C.ii2_align
	if rc := C.ii2_align_terms(c.h, C.uint32_t(len(segFirst)-1), tb, u64ptr(termOff), u64ptr(segFirst), &a); rc != 0 {
		return nil, c.err("align", rc)
	}
	var n C.uint64_t
	var k C.uint32_t
	C.ii2_align_info(a, &n, &k)
	return &Alignment{h: a, NUnion: uint64(n), K: int(k)}, nil
}

// Export copies the alignment out: rep[u] = index (into termOff) of one input term equal to union
// term u; srcList[s*NUnion+u] = index inside dictionary s of the term equal to union term u, or -1.
func (c *Ctx) Export(a *Alignment) (rep []uint64, srcList []int64, err error) {
	rep = make([]uint64, a.NUnion)
	srcList = make([]int64, uint64(a.K)*a.NUnion)
	var sl *C.int64_t
	if len(srcList) > 0 {
		sl = (*C.int64_t)(unsafe.Pointer(&srcList[0]))
	}
	if rc := C.ii2_align_export(c.h, a.h, u64ptr(rep), sl); rc != 0 {
		return nil, nil, c.err("align export", rc)
	}
	return rep, srcList, nil
}

// SelectAligned builds, on the GPU, the term-aligned view of a resident segment for dictionary s
// of the alignment (firstList = list of seg that corresponds to the dictionary's first term).
func (c *Ctx) SelectAligned(seg *Segment, a *Alignment, s int, firstList uint64) (*Segment, error) {
	var v *C.ii2_seg
	if rc := C.ii2_seg_select_aligned(c.h, seg.h, a.h, C.uint32_t(s), C.uint64_t(firstList), &v); rc != 0 {
		return nil, c.err("select", rc)
	}
	return &Segment{v}, nil
}

// SelectAlignedAll builds the views of all the alignment's dictionaries in one call (one wait instead of one per view).
func (c *Ctx) SelectAlignedAll(segs []*Segment, a *Alignment, firstList []uint64) ([]*Segment, error) {
	// the C side writes a.K views: the slices must be exactly that long
	if len(segs) == 0 || len(segs) != a.K || (len(firstList) != 0 && len(firstList) != a.K) {
		return nil, fmt.Errorf("select: %d segments / %d first lists for an alignment of %d dictionaries", len(segs), len(firstList), a.K)
	}
	hs := make([]*C.ii2_seg, len(segs))
	for i, s := range segs {
		hs[i] = s.h
	}
	outs := make([]*C.ii2_seg, len(segs))
	if rc := C.ii2_seg_select_aligned_all(c.h, (**C.ii2_seg)(unsafe.Pointer(&hs[0])), a.h, u64ptr(firstList), (**C.ii2_seg)(unsafe.Pointer(&outs[0]))); rc != 0 {
		return nil, c.err("select", rc)
	}
	vs := make([]*Segment, len(outs))
	for i, h := range outs {
		vs[i] = &Segment{h}
	}
	return vs, nil
}

func (a *Alignment) Free() { C.ii2_align_free(a.h); a.h = nil }

// Dictionary is a segment's sorted, duplicate-free term dictionary resident in HBM (ii2_dict): made once, when the
// segment is written or loaded, so that alignments read it in place (no upload per merge).
type Dictionary struct{ h *C.ii2_dict }

// NewDictionary uploads a dictionary given flat (termBytes, termOff[n+1], termOff[0] == 0).  Terms that do not ascend
// strictly in bytes.Compare order are an error (II2_EINVAL).
func (c *Ctx) NewDictionary(termBytes []byte, termOff []uint64) (*Dictionary, error) {
	var tb *C.uint8_t
	if len(termBytes) > 0 {
		tb = (*C.uint8_t)(unsafe.Pointer(&termBytes[0]))
	}
	var d *C.ii2_dict
	if rc := C.ii2_dict_create(c.h, tb, u64ptr(termOff), C.uint64_t(len(termOff)-1), C.II2_HOST, &d); rc != 0 {
		return nil, c.err("dictionary", rc)
	}
	return &Dictionary{d}, nil
}

func (d *Dictionary) Free() { C.ii2_dict_free(d.h); d.h = nil }

// DictBuildStats mirrors ii2_dict_build_stats.
type DictBuildStats struct {
	Terms, Unique, Bytes uint64
	MinLen, MaxLen       uint32
	Passes               uint32
}

// DictBuild sorts and deduplicates terms on the device (ii2_dict_build): terms in any order, repeats allowed, at most 256 bytes
// each.  The dictionary holds the sorted distinct terms (bytes.Compare order, file/types.go:24-26) and termID[i] is the index of
// terms[i] in it - the listID of SegBuild for the occurrences' values.
func (c *Ctx) DictBuild(terms [][]byte) (*Dictionary, []uint32, DictBuildStats, error) {
	off := make([]uint64, len(terms)+1)
	var blob []byte
	for i, t := range terms {
		blob = append(blob, t...)
		off[i+1] = uint64(len(blob))
	}
	blob = append(blob, 0) // never an empty array
	ids := make([]uint32, len(terms)+1)
	var d *C.ii2_dict
	var st C.ii2_dict_build_stats
	if rc := C.ii2_dict_build(c.h, C.uint64_t(len(terms)), (*C.uint8_t)(unsafe.Pointer(&blob[0])), u64ptr(off), C.II2_HOST, &d,
		(*C.uint32_t)(unsafe.Pointer(&ids[0])), &st); rc != 0 {
		return nil, nil, DictBuildStats{}, c.err("dict build", rc)
	}
	return &Dictionary{d}, ids[:len(terms)], DictBuildStats{uint64(st.n_terms), uint64(st.n_unique), uint64(st.n_bytes), uint32(st.min_len),
		uint32(st.max_len), uint32(st.n_passes)}, nil
}

// DictInfo returns the number of terms of a dictionary and the bytes they take (ii2_dict_info).
func (d *Dictionary) DictInfo() (nTerms, nBytes uint64) {
	var n, b C.uint64_t
	C.ii2_dict_info(d.h, &n, &b)
	return uint64(n), uint64(b)
}

// DictExport copies a dictionary's terms to the host, in its order (ii2_dict_export).
func (c *Ctx) DictExport(d *Dictionary) ([][]byte, error) {
	n, nb := d.DictInfo()
	blob := make([]byte, nb+1)
	off := make([]uint64, n+1)
	if rc := C.ii2_dict_export(c.h, d.h, (*C.uint8_t)(unsafe.Pointer(&blob[0])), u64ptr(off)); rc != 0 {
		return nil, c.err("dict export", rc)
	}
	terms := make([][]byte, n)
	for i := range terms {
		terms[i] = blob[off[i]:off[i+1]]
	}
	return terms, nil
}

// DictFind looks terms up in k resident dictionaries on the device (ii2_dict_find): the step from a query's terms to the list
// ranges every range call takes.  prefix == nil: every probe is a term - [j, j+1) where dictionary s holds it as list j, the
// empty [j, j) at its insertion point where it does not; prefix[p] == 1: the run of the terms that start with probe p
// (PrefixSearch, inverted_index.go:274-292).  Entry p*k + s of first / end answers probe p in dicts[s]: the k ranges of one probe
// are one group of the range calls, with the k segments repeated.  found is the number of non-empty ranges.
func (c *Ctx) DictFind(dicts []*Dictionary, probes [][]byte, prefix []uint8) (first, end []uint64, found uint64, err error) {
	if len(dicts) == 0 {
		return nil, nil, 0, fmt.Errorf("dict find: no dictionaries")
	}
	if prefix != nil && len(prefix) != len(probes) {
		return nil, nil, 0, fmt.Errorf("dict find: one prefix flag per probe")
	}
	hs := make([]*C.ii2_dict, len(dicts))
	for i, d := range dicts {
		hs[i] = d.h
	}
	off := make([]uint64, len(probes)+1)
	var blob []byte
	for i, p := range probes {
		blob = append(blob, p...)
		off[i+1] = uint64(len(blob))
	}
	blob = append(blob, 0) // never an empty array
	first = make([]uint64, len(probes)*len(dicts)+1)
	end = make([]uint64, len(probes)*len(dicts)+1)
	var pf *C.uint8_t
	if len(prefix) > 0 {
		pf = (*C.uint8_t)(unsafe.Pointer(&prefix[0]))
	}
	var n C.uint64_t
	if rc := C.ii2_dict_find(c.h, C.uint32_t(len(hs)), (**C.ii2_dict)(unsafe.Pointer(&hs[0])), C.uint64_t(len(probes)),
		(*C.uint8_t)(unsafe.Pointer(&blob[0])), u64ptr(off), pf, C.II2_HOST, u64ptr(first), u64ptr(end), &n); rc != 0 {
		return nil, nil, 0, c.err("dict find", rc)
	}
	return first[:len(probes)*len(dicts)], end[:len(probes)*len(dicts)], uint64(n), nil
}

// Kinds of DictMatch (II2_MATCH_*); MatchNoCase is OR-ed into a kind: ASCII A-Z and a-z compare equal, no other byte folds.
// MatchUtf8 (II2_MATCH_UTF8) is OR-ed into a kind or into DictFuzzy's flags: positions are UTF-8 symbols - a code point per
// well-formed sequence, one symbol per ill-formed byte of a term - instead of bytes, and the pattern must be well-formed UTF-8.
const (
	MatchContains uint8 = 0
	MatchSuffix   uint8 = 1
	MatchGlob     uint8 = 2
	MatchUtf8     uint8 = 0x08
	MatchNoCase   uint8 = 0x80
)

// MatchStats mirrors ii2_match_stats.
type MatchStats struct {
	Terms, Matched, Runs uint64
	Staged, Global       uint32
}

// DictMatch is the substring, suffix and wildcard term search in k resident dictionaries (ii2_dict_match): what neither DictFind
// nor the FST can answer, because both walk a term from its front.  At most 64 patterns of at most 64 bytes per call (callers
// chunk); kinds[p] is MatchContains / MatchSuffix / MatchGlob (`*`, `?`, `\x`; the whole term), optionally | MatchNoCase, | MatchUtf8.  Pair
// (p, s) - pattern p in dicts[s] - owns the runs runOff[p*k+s] .. runOff[p*k+s+1]-1; run j is the terms [first[j], end[j]) of
// dictionary dict[j].  The runs of pattern p, runOff[p*k] .. runOff[(p+1)*k]-1, are one group of the range calls, with
// segs[j] the segment of dicts[dict[j]].  A result above the first buffer of 4096 runs takes the second call the library asks
// for, with the exact size.
func (c *Ctx) DictMatch(dicts []*Dictionary, patterns [][]byte, kinds []uint8) (runOff, first, end []uint64, dict []uint32, st MatchStats, err error) {
	if len(dicts) == 0 {
		return nil, nil, nil, nil, st, fmt.Errorf("dict match: no dictionaries")
	}
	if len(kinds) != len(patterns) {
		return nil, nil, nil, nil, st, fmt.Errorf("dict match: one kind per pattern")
	}
	hs := make([]*C.ii2_dict, len(dicts))
	for i, d := range dicts {
		hs[i] = d.h
	}
	off := make([]uint64, len(patterns)+1)
	var blob []byte
	for i, p := range patterns {
		blob = append(blob, p...)
		off[i+1] = uint64(len(blob))
	}
	blob = append(blob, 0) // never an empty array
	kd := append([]uint8{}, kinds...)
	kd = append(kd, 0)
	runOff = make([]uint64, len(patterns)*len(dicts)+1)
	capRuns := uint64(4096)
	var cs C.ii2_match_stats
	for attempt := 0; ; attempt++ {
		first, end, dict = make([]uint64, capRuns+1), make([]uint64, capRuns+1), make([]uint32, capRuns+1)
		rc := C.ii2_dict_match(c.h, C.uint32_t(len(hs)), (**C.ii2_dict)(unsafe.Pointer(&hs[0])), C.uint32_t(len(patterns)),
			(*C.uint8_t)(unsafe.Pointer(&blob[0])), u64ptr(off), (*C.uint8_t)(unsafe.Pointer(&kd[0])), u64ptr(runOff), u64ptr(first), u64ptr(end),
			(*C.uint32_t)(unsafe.Pointer(&dict[0])), C.uint64_t(capRuns), &cs)
		if rc == C.II2_ECAPACITY && attempt == 0 {
			capRuns = runOff[len(runOff)-1]
			continue
		}
		if rc != 0 {
			return nil, nil, nil, nil, st, c.err("dict match", rc)
		}
		break
	}
	n := runOff[len(runOff)-1]
	st = MatchStats{uint64(cs.n_terms), uint64(cs.n_matched), uint64(cs.n_runs), uint32(cs.n_staged), uint32(cs.n_global)}
	return runOff, first[:n], end[:n], dict[:n], st, nil
}

// Utf8Decode is the symbols of a byte string by the decoder the kernels run under MatchUtf8 (ii2_utf8_decode): a well-formed
// sequence is its code point, any other byte b alone is 0xDC00 + b; wellFormed says that every byte belongs to a sequence - what a
// pattern must be.  Needs no GPU.
func Utf8Decode(data []byte) (symbols []uint32, wellFormed bool, err error) {
	b := append(append([]byte{}, data...), 0)
	symbols = make([]uint32, len(data)+1)
	var n C.uint64_t
	var ok C.int
	if rc := C.ii2_utf8_decode((*C.uint8_t)(unsafe.Pointer(&b[0])), C.uint64_t(len(data)), (*C.uint32_t)(unsafe.Pointer(&symbols[0])),
		C.uint64_t(len(data)), &n, &ok); rc != 0 {
		return nil, false, fmt.Errorf("utf8 decode: error %d", int(rc))
	}
	return symbols[:n], ok != 0, nil
}

// TermMatch is one pattern against one term by the functions DictMatch's kernel runs (ii2_term_match); needs no GPU.
func TermMatch(kind uint8, pattern, term []byte) (bool, error) {
	p, t := append(append([]byte{}, pattern...), 0), append(append([]byte{}, term...), 0)
	var m C.int
	if rc := C.ii2_term_match(C.uint32_t(kind), (*C.uint8_t)(unsafe.Pointer(&p[0])), C.uint64_t(len(pattern)), (*C.uint8_t)(unsafe.Pointer(&t[0])),
		C.uint64_t(len(term)), &m); rc != 0 {
		return false, fmt.Errorf("term match: error %d", int(rc))
	}
	return m != 0, nil
}

// FuzzyTranspose is a flag of DictFuzzy (II2_FUZZY_TRANSPOSE): an adjacent transposition costs 1 (optimal string alignment).
// MatchNoCase and MatchUtf8 (distance, prefix and length filter count UTF-8 symbols) are the only other flags.
const FuzzyTranspose uint8 = 0x01

// FuzzyStats mirrors ii2_fuzzy_stats.
type FuzzyStats struct {
	Terms, Matched, Runs, Tested uint64
	Staged, Global, WordBits     uint32
	Utf8                         uint32 // patterns that carried MatchUtf8; 0: the byte instances ran
}

// DictFuzzy is the typo-tolerant term search in k resident dictionaries (ii2_dict_fuzzy): every term within dist[p] edits of
// pattern p that shares its first prefix[p] bytes.  At most 16 patterns of at most 64 bytes per call (callers chunk); flags[p] is
// 0, FuzzyTranspose, MatchNoCase and / or MatchUtf8 (edits and prefix in symbols); prefix and flags may be nil (all 0).  The answer is laid out as DictMatch's: pair
// (p, s) owns the runs runOff[p*k+s] .. runOff[p*k+s+1]-1, run j is the terms [first[j], end[j]) of dictionary dict[j], and the
// runs of pattern p are one group of the range calls.  The runs carry no distance: send a pattern with distances 0, 1 and 2 for
// tiers - the groups nest, so their weights add up in TopKWeightedRanges.  A result above the first buffer of 4096 runs takes the
// second call the library asks for, with the exact size.
func (c *Ctx) DictFuzzy(dicts []*Dictionary, patterns [][]byte, dist, prefix, flags []uint8) (runOff, first, end []uint64, dict []uint32, st FuzzyStats, err error) {
	if len(dicts) == 0 {
		return nil, nil, nil, nil, st, fmt.Errorf("dict fuzzy: no dictionaries")
	}
	if len(dist) != len(patterns) || (prefix != nil && len(prefix) != len(patterns)) || (flags != nil && len(flags) != len(patterns)) {
		return nil, nil, nil, nil, st, fmt.Errorf("dict fuzzy: one distance, prefix and flag byte per pattern")
	}
	hs := make([]*C.ii2_dict, len(dicts))
	for i, d := range dicts {
		hs[i] = d.h
	}
	off := make([]uint64, len(patterns)+1)
	var blob []byte
	for i, p := range patterns {
		blob = append(blob, p...)
		off[i+1] = uint64(len(blob))
	}
	blob = append(blob, 0) // never an empty array
	ds := append(append([]uint8{}, dist...), 0)
	var pp, fp *C.uint8_t
	if prefix != nil {
		pre := append(append([]uint8{}, prefix...), 0)
		pp = (*C.uint8_t)(unsafe.Pointer(&pre[0]))
	}
	if flags != nil {
		fl := append(append([]uint8{}, flags...), 0)
		fp = (*C.uint8_t)(unsafe.Pointer(&fl[0]))
	}
	runOff = make([]uint64, len(patterns)*len(dicts)+1)
	capRuns := uint64(4096)
	var cs C.ii2_fuzzy_stats
	for attempt := 0; ; attempt++ {
		first, end, dict = make([]uint64, capRuns+1), make([]uint64, capRuns+1), make([]uint32, capRuns+1)
		rc := C.ii2_dict_fuzzy(c.h, C.uint32_t(len(hs)), (**C.ii2_dict)(unsafe.Pointer(&hs[0])), C.uint32_t(len(patterns)),
			(*C.uint8_t)(unsafe.Pointer(&blob[0])), u64ptr(off), (*C.uint8_t)(unsafe.Pointer(&ds[0])), pp, fp, u64ptr(runOff), u64ptr(first), u64ptr(end),
			(*C.uint32_t)(unsafe.Pointer(&dict[0])), C.uint64_t(capRuns), &cs)
		if rc == C.II2_ECAPACITY && attempt == 0 {
			capRuns = runOff[len(runOff)-1]
			continue
		}
		if rc != 0 {
			return nil, nil, nil, nil, st, c.err("dict fuzzy", rc)
		}
		break
	}
	n := runOff[len(runOff)-1]
	st = FuzzyStats{uint64(cs.n_terms), uint64(cs.n_matched), uint64(cs.n_runs), uint64(cs.n_tested), uint32(cs.n_staged), uint32(cs.n_global),
		uint32(cs.word_bits), uint32(cs.n_utf8)}
	return runOff, first[:n], end[:n], dict[:n], st, nil
}

// TermFuzzy is one pattern against one term by the functions DictFuzzy's kernel runs (ii2_term_fuzzy): whether the term matches,
// and the exact distance under flags whatever prefix and maxDist are; needs no GPU.
func TermFuzzy(pattern, term []byte, maxDist, prefix uint32, flags uint8) (bool, uint32, error) {
	p, t := append(append([]byte{}, pattern...), 0), append(append([]byte{}, term...), 0)
	var m C.int
	var d C.uint32_t
	if rc := C.ii2_term_fuzzy(C.uint32_t(flags), (*C.uint8_t)(unsafe.Pointer(&p[0])), C.uint64_t(len(pattern)), C.uint32_t(prefix), C.uint32_t(maxDist),
		(*C.uint8_t)(unsafe.Pointer(&t[0])), C.uint64_t(len(term)), &m, &d); rc != 0 {
		return false, 0, fmt.Errorf("term fuzzy: error %d", int(rc))
	}
	return m != 0, uint32(d), nil
}

// RegexStats mirrors ii2_regex_stats.
type RegexStats struct {
	Terms, Matched, Runs, Tested uint64
	Staged, Global, MaxPositions uint32
}

// DictRegex is the regular-expression term search in k resident dictionaries (ii2_dict_regex): every term that pattern p
// matches as a WHOLE (write `.*foo.*` for "contains").  The syntax is the subset of Python's re on bytes that include/ii2.h
// lists - classes, alternation, groups, counted repetition, no anchors, `.` matches any byte.  At most 8 patterns of at most 256
// bytes and 64 positions per call (callers chunk); flags[p] is 0 or MatchNoCase; flags may be nil (all 0).  The answer is laid
// out as DictMatch's: pair (p, s) owns the runs runOff[p*k+s] .. runOff[p*k+s+1]-1, run j is the terms [first[j], end[j]) of
// dictionary dict[j], and the runs of pattern p are one group of the range calls.  A result above the first buffer of 4096 runs
// takes the second call the library asks for, with the exact size.
func (c *Ctx) DictRegex(dicts []*Dictionary, patterns [][]byte, flags []uint8) (runOff, first, end []uint64, dict []uint32, st RegexStats, err error) {
	if len(dicts) == 0 {
		return nil, nil, nil, nil, st, fmt.Errorf("dict regex: no dictionaries")
	}
	if flags != nil && len(flags) != len(patterns) {
		return nil, nil, nil, nil, st, fmt.Errorf("dict regex: one flag byte per pattern")
	}
	hs := make([]*C.ii2_dict, len(dicts))
	for i, d := range dicts {
		hs[i] = d.h
	}
	off := make([]uint64, len(patterns)+1)
	var blob []byte
	for i, p := range patterns {
		blob = append(blob, p...)
		off[i+1] = uint64(len(blob))
	}
	blob = append(blob, 0) // never an empty array
	var fp *C.uint8_t
	if flags != nil {
		fl := append(append([]uint8{}, flags...), 0)
		fp = (*C.uint8_t)(unsafe.Pointer(&fl[0]))
	}
	runOff = make([]uint64, len(patterns)*len(dicts)+1)
	capRuns := uint64(4096)
	var cs C.ii2_regex_stats
	for attempt := 0; ; attempt++ {
		first, end, dict = make([]uint64, capRuns+1), make([]uint64, capRuns+1), make([]uint32, capRuns+1)
		rc := C.ii2_dict_regex(c.h, C.uint32_t(len(hs)), (**C.ii2_dict)(unsafe.Pointer(&hs[0])), C.uint32_t(len(patterns)),
			(*C.uint8_t)(unsafe.Pointer(&blob[0])), u64ptr(off), fp, u64ptr(runOff), u64ptr(first), u64ptr(end),
			(*C.uint32_t)(unsafe.Pointer(&dict[0])), C.uint64_t(capRuns), &cs)
		if rc == C.II2_ECAPACITY && attempt == 0 {
			capRuns = runOff[len(runOff)-1]
			continue
		}
		if rc != 0 {
			return nil, nil, nil, nil, st, c.err("dict regex", rc)
		}
		break
	}
	n := runOff[len(runOff)-1]
	st = RegexStats{uint64(cs.n_terms), uint64(cs.n_matched), uint64(cs.n_runs), uint64(cs.n_tested), uint32(cs.n_staged), uint32(cs.n_global),
		uint32(cs.max_positions)}
	return runOff, first[:n], end[:n], dict[:n], st, nil
}

// TermRegex is one pattern against one term by the functions DictRegex's kernel runs (ii2_term_regex): whether the pattern
// matches the whole term, and the positions of its automaton - also set when they are too many (the error then is II2_ERANGE);
// needs no GPU.
func TermRegex(pattern, term []byte, flags uint8) (bool, uint32, error) {
	p, t := append(append([]byte{}, pattern...), 0), append(append([]byte{}, term...), 0)
	var m C.int
	var n C.uint32_t
	if rc := C.ii2_term_regex(C.uint32_t(flags), (*C.uint8_t)(unsafe.Pointer(&p[0])), C.uint64_t(len(pattern)), (*C.uint8_t)(unsafe.Pointer(&t[0])),
		C.uint64_t(len(term)), &m, &n); rc != 0 {
		return false, uint32(n), fmt.Errorf("term regex: error %d", int(rc))
	}
	return m != 0, uint32(n), nil
}

// AlignDicts is AlignTerms on resident dictionaries (ii2_align_dicts): nothing is uploaded, nothing is sorted.
func (c *Ctx) AlignDicts(dicts []*Dictionary) (*Alignment, error) {
	hs := make([]*C.ii2_dict, len(dicts))
	for i, d := range dicts {
		hs[i] = d.h
	}
	var a *C.ii2_align
	if len(hs) == 0 {
		return nil, fmt.Errorf("align: no dictionaries")
	}
	if rc := C.ii2_align_dicts(c.h, C.uint32_t(len(hs)), (**C.ii2_dict)(unsafe.Pointer(&hs[0])), &a); rc != 0 {
		return nil, c.err("align", rc)
	}
	var n C.uint64_t
	var k C.uint32_t
	C.ii2_align_info(a, &n, &k)
	return &Alignment{h: a, NUnion: uint64(n), K: int(k)}, nil
}

// MergeSmall is the common Shard.Merge in one launch (ii2_merge_small): a few small resident segments (what Shard.Put
// writes, shard.go:33-67), their dictionaries flat as for AlignTerms, RemovedLists.Values().  It returns the merged
// segment (nil when no term survives, shard.go:219-225) and, per output list, the index into termOff of an input term
// equal to its term.  ErrTooLarge (II2_ERANGE) means: take AlignTerms + MergeSegmentsToSeg instead.
func (c *Ctx) MergeSmall(segs []*Segment, termBytes []byte, termOff, segFirst []uint64, removed []uint32) (*Segment, []uint64, error) {
	hs := make([]*C.ii2_seg, len(segs))
	for i, s := range segs {
		hs[i] = s.h
	}
	var tb *C.uint8_t
	if len(termBytes) > 0 {
		tb = (*C.uint8_t)(unsafe.Pointer(&termBytes[0]))
	}
	kept := make([]uint64, len(termOff))
	var nKept C.uint64_t
	var out *C.ii2_seg
	var st C.ii2_merge_stats
	if len(hs) == 0 {
		return nil, nil, fmt.Errorf("merge: no segments")
	}
	rc := C.ii2_merge_small(c.h, C.uint32_t(len(hs)), (**C.ii2_seg)(unsafe.Pointer(&hs[0])), tb, u64ptr(termOff), u64ptr(segFirst),
		u32ptr(removed), C.uint64_t(len(removed)), &out, u64ptr(kept), &nKept, &st)
	if rc == C.II2_ERANGE {
		return nil, nil, ErrTooLarge
	}
	if rc != 0 {
		return nil, nil, c.err("merge", rc)
	}
	if out == nil {
		return nil, nil, nil
	}
	return &Segment{out}, kept[:nKept], nil
}

// ReadSmall is the small Shard.Read in one launch (ii2_read_small): the merged lists of a few small resident segments —
// dictionary s names the lists listFirst[s].. of segs[s] (nil: from list 0) — on the host.  rep[j] indexes termOff: an
// input term equal to merged term j; the ids of term j are values[postOff[j]:postOff[j+1]].  ErrTooLarge as for MergeSmall.
func (c *Ctx) ReadSmall(segs []*Segment, termBytes []byte, termOff, segFirst, listFirst []uint64, capValues int) (rep, postOff []uint64, values []uint32, err error) {
	hs := make([]*C.ii2_seg, len(segs))
	for i, s := range segs {
		hs[i] = s.h
	}
	var tb *C.uint8_t
	if len(termBytes) > 0 {
		tb = (*C.uint8_t)(unsafe.Pointer(&termBytes[0]))
	}
	rep = make([]uint64, len(termOff))
	postOff = make([]uint64, len(termOff)+1)
	values = make([]uint32, capValues+1)
	var nUnion C.uint64_t
	if len(hs) == 0 {
		return nil, nil, nil, fmt.Errorf("read: no segments")
	}
	rc := C.ii2_read_small(c.h, C.uint32_t(len(hs)), (**C.ii2_seg)(unsafe.Pointer(&hs[0])), tb, u64ptr(termOff), u64ptr(segFirst),
		u64ptr(listFirst), u64ptr(rep), u64ptr(postOff), u32ptr(values), C.uint64_t(capValues), &nUnion)
	if rc == C.II2_ERANGE {
		return nil, nil, nil, ErrTooLarge
	}
	if rc != 0 {
		return nil, nil, nil, c.err("read", rc)
	}
	return rep[:nUnion], postOff[:nUnion+1], values[:postOff[nUnion]], nil
}

// ErrTooLarge: the inputs exceed the one-launch merge's limits (II2_SMALL_MERGE_*).
var ErrTooLarge = fmt.Errorf("gpu: too large for the one-launch merge")

// SegAllGather concatenates every rank's merged segment in rank order into one segment on every rank; the postings
// travel DV1-encoded (ii2_seg_allgather; one process per GPU, the communicator set up with ii2_comm_init).
func (c *Ctx) SegAllGather(local *Segment) (*Segment, error) {
	var out *C.ii2_seg
	if rc := C.ii2_seg_allgather(c.h, local.h, &out); rc != 0 {
		return nil, c.err("segment all-gather", rc)
	}
	return &Segment{out}, nil
}

// SegConcat is the same concatenation on one device: the lists of segs[0], then segs[1], ... as one segment.
func (c *Ctx) SegConcat(segs []*Segment) (*Segment, error) {
	if len(segs) == 0 {
		return nil, fmt.Errorf("concat: no segments")
	}
	hs := make([]*C.ii2_seg, len(segs))
	for i, s := range segs {
		hs[i] = s.h
	}
	var out *C.ii2_seg
	if rc := C.ii2_seg_concat(c.h, C.uint32_t(len(hs)), (**C.ii2_seg)(unsafe.Pointer(&hs[0])), &out); rc != 0 {
		return nil, c.err("concat", rc)
	}
	return &Segment{out}, nil
}

// MergeSegmentsToSeg merges k term-aligned resident segments (views from SelectAligned / SelectAlignedAll) into a new
// resident segment, minus RemovedLists.Values() (ii2_tomb_create + ii2_merge_segments_to_seg): the general path behind
// MergeSmall.  It returns nil when no posting survives (shard.go:219-225); the caller drops the emptied term slots.
func (c *Ctx) MergeSegmentsToSeg(segs []*Segment, removed []uint32) (*Segment, error) {
	hs := make([]*C.ii2_seg, len(segs))
	for i, s := range segs {
		hs[i] = s.h
	}
	var tomb *C.ii2_tomb
	if len(removed) > 0 {
		if rc := C.ii2_tomb_create(c.h, u32ptr(removed), C.uint64_t(len(removed)), C.II2_HOST, &tomb); rc != 0 {
			return nil, c.err("merge", rc)
		}
		defer C.ii2_tomb_free(tomb)
	}
	var out *C.ii2_seg
	var st C.ii2_merge_stats
	if len(hs) == 0 {
		return nil, fmt.Errorf("merge: no segments")
	}
	if rc := C.ii2_merge_segments_to_seg(c.h, C.uint32_t(len(hs)), (**C.ii2_seg)(unsafe.Pointer(&hs[0])), tomb, &out, &st); rc != 0 {
		return nil, c.err("merge", rc)
	}
	if out == nil {
		return nil, nil
	}
	return &Segment{out}, nil
}

// Query ops of QueryBatch (II2_OP_AND / II2_OP_OR).
const (
	OpAnd uint8 = 0
	OpOr  uint8 = 1
)

// ErrCapacity: the packed results of a QueryBatch did not fit `out`; the returned offsets hold the sizes needed.
var ErrCapacity = fmt.Errorf("gpu: results do not fit the output buffer")

// QueryBatch answers MANY AND / OR queries over resident segments in one call (ii2_query_batch): a number of launches
// and one wait that do not depend on len(op).  Query q owns the ranges queryFirst[q] .. queryFirst[q+1]-1; a range is lists
// [listFirst[i], listEnd[i]) of segs[i].  OpOr: the union of every list in the query's ranges (one query per prefix replaces
// PrefixSearch's per-prefix append + slices.Sort + slices.Compact, inverted_index.go:274-292); OpAnd: every list in the
// ranges is one operand.  The results are packed back to back into the device buffer out (capacity capIDs ids) in query
// order; the returned offsets (len(op)+1) delimit them.  All-or-nothing: on ErrCapacity nothing was written and
// offsets[len(op)] is the capacity to call again with.
func (c *Ctx) QueryBatch(op []uint8, queryFirst []uint64, segs []*Segment, listFirst, listEnd []uint64, out unsafe.Pointer, capIDs uint64) ([]uint64, error) {
	if len(queryFirst) != len(op)+1 || len(listFirst) != len(segs) || len(listEnd) != len(segs) {
		return nil, fmt.Errorf("query batch: array lengths disagree")
	}
	offsets := make([]uint64, len(op)+1)
	if len(op) == 0 {
		return offsets, nil
	}
	hs := make([]*C.ii2_seg, len(segs)+1)
	for i, s := range segs {
		hs[i] = s.h
	}
	rc := C.ii2_query_batch(c.h, C.uint64_t(len(op)), (*C.uint8_t)(unsafe.Pointer(&op[0])), u64ptr(queryFirst),
		(**C.ii2_seg)(unsafe.Pointer(&hs[0])), u64ptr(listFirst), u64ptr(listEnd), nil, (*C.uint32_t)(out), C.uint64_t(capIDs), u64ptr(offsets))
	if rc == C.II2_ECAPACITY {
		return offsets, ErrCapacity
	}
	if rc != 0 {
		return nil, c.err("query batch", rc)
	}
	return offsets, nil
}

// QueryBatchHost is QueryBatch with the results in host memory: a device buffer of firstCap ids, a second call with the size the
// first one reported when the results did not fit (nothing was written then), one download.  Returns the packed ids and the
// offsets that delimit the queries' results.
func (c *Ctx) QueryBatchHost(op []uint8, queryFirst []uint64, segs []*Segment, listFirst, listEnd []uint64, firstCap uint64) ([]uint32, []uint64, error) {
	capIDs := firstCap
	for attempt := 0; ; attempt++ {
		var d unsafe.Pointer
		if rc := C.ii2_dev_alloc(c.h, C.size_t((capIDs+1)*4), &d); rc != 0 {
			return nil, nil, c.err("query batch", rc)
		}
		offs, err := c.QueryBatch(op, queryFirst, segs, listFirst, listEnd, d, capIDs+1)
		if err == ErrCapacity && attempt == 0 {
			C.ii2_dev_free(c.h, d)
			capIDs = offs[len(offs)-1]
			continue
		}
		if err != nil {
			C.ii2_dev_free(c.h, d)
			return nil, nil, err
		}
		n := offs[len(offs)-1]
		ids := make([]uint32, n)
		var rc C.int
		if n > 0 {
			rc = C.ii2_copy_d2h(c.h, unsafe.Pointer(&ids[0]), d, C.size_t(n*4))
		}
		C.ii2_dev_free(c.h, d)
		if rc != 0 {
			return nil, nil, c.err("query batch", rc)
		}
		return ids, offs, nil
	}
}

// QueryBatchGroups answers MANY AND-of-ORs / NOT queries over resident segments in one call (ii2_query_batch_groups): QueryBatch
// for an index that is not fully merged, where a term is a group - one short list per Put segment that holds it.  Query q owns
// the groups queryFirst[q] .. queryFirst[q+1]-1; groupFirst, groupNot and the range arrays are those of AndNotRanges over all
// groups of the batch (groupNot == nil: every group is required), and result q is what AndNotRanges returns for query q's
// groups: one required group is a union, several an AND of ORs, excluded groups a NOT.  A query without groups, or with a
// required group without postings, gives an empty result; a query with groups but no required one is an error that names the
// query.  Replaces a loop over Intersect / IntersectExcept (index.go) by a number of launches and one wait that do not depend
// on the number of queries.  The results are packed back to back into the device buffer out (capacity capIDs ids; the sum over
// the queries of the postings of their smallest required group is always enough) in query order; the returned offsets
// (len(queryFirst)) delimit them.  All-or-nothing: on ErrCapacity nothing was written and the last offset is the capacity to
// call again with.
func (c *Ctx) QueryBatchGroups(queryFirst, groupFirst []uint64, groupNot []uint8, segs []*Segment, listFirst, listEnd []uint64, out unsafe.Pointer, capIDs uint64) ([]uint64, error) {
	nQueries := len(queryFirst) - 1
	if nQueries < 0 || len(groupFirst) == 0 || (groupNot != nil && len(groupNot) != len(groupFirst)-1) || len(listFirst) != len(segs) || len(listEnd) != len(segs) {
		return nil, fmt.Errorf("query batch groups: array lengths disagree")
	}
	// the C side reads groupFirst[0 .. queryFirst[nQueries]] and the range arrays up to groupFirst's last element
	if queryFirst[nQueries] != uint64(len(groupFirst)-1) || groupFirst[len(groupFirst)-1] != uint64(len(segs)) {
		return nil, fmt.Errorf("query batch groups: queryFirst / groupFirst do not end at the lengths of the arrays they index")
	}
	offsets := make([]uint64, nQueries+1)
	if nQueries == 0 {
		return offsets, nil
	}
	hs := make([]*C.ii2_seg, len(segs)+1)
	for i, s := range segs {
		hs[i] = s.h
	}
	var flags *C.uint8_t
	if len(groupNot) != 0 {
		flags = (*C.uint8_t)(unsafe.Pointer(&groupNot[0]))
	}
	rc := C.ii2_query_batch_groups(c.h, C.uint64_t(nQueries), u64ptr(queryFirst), u64ptr(groupFirst), flags,
		(**C.ii2_seg)(unsafe.Pointer(&hs[0])), u64ptr(listFirst), u64ptr(listEnd), nil, (*C.uint32_t)(out), C.uint64_t(capIDs), u64ptr(offsets))
	if rc == C.II2_ECAPACITY {
		return offsets, ErrCapacity
	}
	if rc != 0 {
		return nil, c.err("query batch groups", rc)
	}
	return offsets, nil
}

// AndNotRanges answers one boolean query with excluded (NOT) groups over resident segments (ii2_andnot_ranges): the ids that
// lie in at least one list of EVERY required group and in NO list of ANY excluded group.  Group g owns the ranges
// groupFirst[g] .. groupFirst[g+1]-1, a range being lists [listFirst[i], listEnd[i]) of segs[i]; groupNot[g] is 0 for a
// required group and 1 for an excluded one (at least one group must be required; groupNot == nil: every group is required,
// the call is ii2_intersect_ranges).  The ids go to the device buffer out (capacity capIDs ids; the postings of the smallest
// required group are always enough) and their number is returned.  All-or-nothing: on ErrCapacity nothing was written and
// the returned count is the capacity to call again with.
func (c *Ctx) AndNotRanges(groupFirst []uint64, groupNot []uint8, segs []*Segment, listFirst, listEnd []uint64, out unsafe.Pointer, capIDs uint64) (uint64, error) {
	nGroups := len(groupFirst) - 1
	if nGroups < 0 || (groupNot != nil && len(groupNot) != nGroups) || len(listFirst) != len(segs) || len(listEnd) != len(segs) {
		return 0, fmt.Errorf("andnot ranges: array lengths disagree")
	}
	if groupFirst[nGroups] != uint64(len(segs)) { // the C side reads the range arrays up to groupFirst's last element
		return 0, fmt.Errorf("andnot ranges: groupFirst does not end at the number of ranges")
	}
	if nGroups == 0 {
		return 0, nil
	}
	hs := make([]*C.ii2_seg, len(segs)+1)
	for i, s := range segs {
		hs[i] = s.h
	}
	var flags *C.uint8_t
	if groupNot != nil {
		flags = (*C.uint8_t)(unsafe.Pointer(&groupNot[0]))
	}
	var n C.uint64_t
	rc := C.ii2_andnot_ranges(c.h, C.uint64_t(nGroups), u64ptr(groupFirst), flags, (**C.ii2_seg)(unsafe.Pointer(&hs[0])),
		u64ptr(listFirst), u64ptr(listEnd), nil, (*C.uint32_t)(out), C.uint64_t(capIDs), &n)
	if rc == C.II2_ECAPACITY {
		return uint64(n), ErrCapacity
	}
	if rc != 0 {
		return 0, c.err("andnot ranges", rc)
	}
	return uint64(n), nil
}

// AndNotRangesHost is AndNotRanges with the result in host memory: a device buffer of firstCap ids (the caller's bound of the
// smallest required group, or less), a second call with the size the first one reported when the result did not fit (nothing
// was written then), one download.
func (c *Ctx) AndNotRangesHost(groupFirst []uint64, groupNot []uint8, segs []*Segment, listFirst, listEnd []uint64, firstCap uint64) ([]uint32, error) {
	capIDs := firstCap
	for attempt := 0; ; attempt++ {
		var d unsafe.Pointer
		if rc := C.ii2_dev_alloc(c.h, C.size_t((capIDs+1)*4), &d); rc != 0 {
			return nil, c.err("andnot ranges", rc)
		}
		n, err := c.AndNotRanges(groupFirst, groupNot, segs, listFirst, listEnd, d, capIDs+1)
		if err == ErrCapacity && attempt == 0 {
			C.ii2_dev_free(c.h, d)
			capIDs = n
			continue
		}
		if err != nil {
			C.ii2_dev_free(c.h, d)
			return nil, err
		}
		ids := make([]uint32, n)
		var rc C.int
		if n > 0 {
			rc = C.ii2_copy_d2h(c.h, unsafe.Pointer(&ids[0]), d, C.size_t(n*4))
		}
		C.ii2_dev_free(c.h, d)
		if rc != 0 {
			return nil, c.err("andnot ranges", rc)
		}
		return ids, nil
	}
}

// AtLeastStats mirrors ii2_atleast_stats.
type AtLeastStats struct {
	Counted, Bound                uint64
	Form, Planes, Windows, NLate uint32
}

// The forms of AtLeastRanges (II2_ATLEAST_*).
const (
	AtLeastNone  = uint32(C.II2_ATLEAST_NONE)
	AtLeastSmall = uint32(C.II2_ATLEAST_SMALL)
	AtLeastCount = uint32(C.II2_ATLEAST_COUNT)
	AtLeastAnd   = uint32(C.II2_ATLEAST_AND)
	AtLeastOr    = uint32(C.II2_ATLEAST_OR)
)

// AtLeastRanges answers one threshold query over resident segments (ii2_atleast_ranges): the ids that lie in at least one list
// of AT LEAST minMatch required groups and in NO list of ANY excluded group.  Groups, ranges and groupNot are those of
// AndNotRanges; a required group without postings matches no doc.  The ids go to the device buffer out (capacity capIDs ids;
// the postings of the n' - minMatch + 1 smallest required groups are always enough) and their number is returned.
// All-or-nothing: on ErrCapacity nothing was written and the returned count is the capacity to call again with.
func (c *Ctx) AtLeastRanges(groupFirst []uint64, groupNot []uint8, minMatch uint32, segs []*Segment, listFirst, listEnd []uint64, out unsafe.Pointer, capIDs uint64) (uint64, AtLeastStats, error) {
	nGroups := len(groupFirst) - 1
	if nGroups < 0 || (groupNot != nil && len(groupNot) != nGroups) || len(listFirst) != len(segs) || len(listEnd) != len(segs) {
		return 0, AtLeastStats{}, fmt.Errorf("atleast ranges: array lengths disagree")
	}
	if groupFirst[nGroups] != uint64(len(segs)) { // the C side reads the range arrays up to groupFirst's last element
		return 0, AtLeastStats{}, fmt.Errorf("atleast ranges: groupFirst does not end at the number of ranges")
	}
	hs := make([]*C.ii2_seg, len(segs)+1)
	for i, s := range segs {
		hs[i] = s.h
	}
	var flags *C.uint8_t
	if groupNot != nil && nGroups > 0 {
		flags = (*C.uint8_t)(unsafe.Pointer(&groupNot[0]))
	}
	var n C.uint64_t
	var st C.ii2_atleast_stats
	rc := C.ii2_atleast_ranges(c.h, C.uint64_t(nGroups), u64ptr(groupFirst), flags, C.uint32_t(minMatch), (**C.ii2_seg)(unsafe.Pointer(&hs[0])),
		u64ptr(listFirst), u64ptr(listEnd), nil, (*C.uint32_t)(out), C.uint64_t(capIDs), &n, &st)
	stats := AtLeastStats{uint64(st.n_counted), uint64(st.bound), uint32(st.form), uint32(st.n_planes), uint32(st.n_windows), uint32(st.n_late)}
	if rc == C.II2_ECAPACITY {
		return uint64(n), stats, ErrCapacity
	}
	if rc != 0 {
		return 0, AtLeastStats{}, c.err("atleast ranges", rc)
	}
	return uint64(n), stats, nil
}

// AtLeastRangesHost is AtLeastRanges with the result in host memory, in the shape of AndNotRangesHost: a device buffer of firstCap
// ids, a second call with the size the first one reported when the result did not fit, one download.
func (c *Ctx) AtLeastRangesHost(groupFirst []uint64, groupNot []uint8, minMatch uint32, segs []*Segment, listFirst, listEnd []uint64, firstCap uint64) ([]uint32, error) {
	capIDs := firstCap
	for attempt := 0; ; attempt++ {
		var d unsafe.Pointer
		if rc := C.ii2_dev_alloc(c.h, C.size_t((capIDs+1)*4), &d); rc != 0 {
			return nil, c.err("atleast ranges", rc)
		}
		n, _, err := c.AtLeastRanges(groupFirst, groupNot, minMatch, segs, listFirst, listEnd, d, capIDs+1)
		if err == ErrCapacity && attempt == 0 {
			C.ii2_dev_free(c.h, d)
			capIDs = n
			continue
		}
		if err != nil {
			C.ii2_dev_free(c.h, d)
			return nil, err
		}
		ids := make([]uint32, n)
		var rc C.int
		if n > 0 {
			rc = C.ii2_copy_d2h(c.h, unsafe.Pointer(&ids[0]), d, C.size_t(n*4))
		}
		C.ii2_dev_free(c.h, d)
		if rc != 0 {
			return nil, c.err("atleast ranges", rc)
		}
		return ids, nil
	}
}

// TopKStats mirrors ii2_topk_stats.
type TopKStats struct {
	Counted, Eligible, NCut                       uint64
	MaxScore, CutScore, Planes, Windows, NMarks uint32
}

// TopKMax is the largest k of TopKRanges (II2_TOPK_MAX).
const TopKMax = uint64(C.II2_TOPK_MAX)

// TopKRanges answers one ranked query over resident segments (ii2_topk_ranges): the k docs that lie in the most required groups - at
// least minMatch of them, in NO list of ANY excluded group - ordered by score descending, then id ascending.  Groups, ranges and
// groupNot are those of AtLeastRanges; a required group without postings matches no doc.  The ids go to the device buffer ids and
// their scores to scores (k entries each; scores may be nil); the number written, min(k, eligible docs), is returned together with
// the score histogram (eligible docs per score).  k == 0 returns the histogram and stats only.  There is no ErrCapacity.
func (c *Ctx) TopKRanges(groupFirst []uint64, groupNot []uint8, minMatch uint32, k uint64, segs []*Segment, listFirst, listEnd []uint64, ids, scores unsafe.Pointer) (uint64, [256]uint64, TopKStats, error) {
	var hist [256]uint64
	nGroups := len(groupFirst) - 1
	if nGroups < 0 || (groupNot != nil && len(groupNot) != nGroups) || len(listFirst) != len(segs) || len(listEnd) != len(segs) {
		return 0, hist, TopKStats{}, fmt.Errorf("topk ranges: array lengths disagree")
	}
	if groupFirst[nGroups] != uint64(len(segs)) { // the C side reads the range arrays up to groupFirst's last element
		return 0, hist, TopKStats{}, fmt.Errorf("topk ranges: groupFirst does not end at the number of ranges")
	}
	hs := make([]*C.ii2_seg, len(segs)+1)
	for i, s := range segs {
		hs[i] = s.h
	}
	var flags *C.uint8_t
	if groupNot != nil && nGroups > 0 {
		flags = (*C.uint8_t)(unsafe.Pointer(&groupNot[0]))
	}
	var n C.uint64_t
	var st C.ii2_topk_stats
	rc := C.ii2_topk_ranges(c.h, C.uint64_t(nGroups), u64ptr(groupFirst), flags, C.uint32_t(minMatch), C.uint64_t(k), (**C.ii2_seg)(unsafe.Pointer(&hs[0])),
		u64ptr(listFirst), u64ptr(listEnd), nil, (*C.uint32_t)(ids), (*C.uint32_t)(scores), &n, (*C.uint64_t)(unsafe.Pointer(&hist[0])), &st)
	if rc != 0 {
		return 0, hist, TopKStats{}, c.err("topk ranges", rc)
	}
	stats := TopKStats{uint64(st.n_counted), uint64(st.n_eligible), uint64(st.n_cut), uint32(st.max_score), uint32(st.cut_score), uint32(st.n_planes),
		uint32(st.n_windows), uint32(st.n_marks)}
	return uint64(n), hist, stats, nil
}

// Scored is one entry of a ranked result: a doc id and its score - the number of groups it lies in, or the sum of their weights.
type Scored struct {
	ID, Score uint32
}

// TopKRangesHost is TopKRanges with the result in host memory: one device buffer of 2k words (the ids, then the scores), one call,
// one download.
func (c *Ctx) TopKRangesHost(groupFirst []uint64, groupNot []uint8, minMatch uint32, k uint64, segs []*Segment, listFirst, listEnd []uint64) ([]Scored, error) {
	if k == 0 {
		return nil, nil
	}
	var d unsafe.Pointer
	if rc := C.ii2_dev_alloc(c.h, C.size_t(2*k*4), &d); rc != 0 {
		return nil, c.err("topk ranges", rc)
	}
	defer C.ii2_dev_free(c.h, d)
	n, _, _, err := c.TopKRanges(groupFirst, groupNot, minMatch, k, segs, listFirst, listEnd, d, unsafe.Add(d, int(k*4)))
	if err != nil || n == 0 {
		return nil, err
	}
	raw := make([]uint32, k+n)
	if rc := C.ii2_copy_d2h(c.h, unsafe.Pointer(&raw[0]), d, C.size_t((k+n)*4)); rc != 0 {
		return nil, c.err("topk ranges", rc)
	}
	out := make([]Scored, n)
	for i := range out {
		out[i] = Scored{raw[i], raw[k+uint64(i)]}
	}
	return out, nil
}

// TopKWStats mirrors ii2_topkw_stats.
type TopKWStats struct {
	Counted, Eligible, NCut                                         uint64
	TotalWeight, MaxScore, CutScore, Planes, Windows, NMarks, NLate uint32
}

// TopKWeightedRanges is TopKRanges with a weight per group (ii2_topk_weighted_ranges): a doc's score is the sum of groupWeight[g]
// over the required groups g it lies in - weights 1 .. 255 that sum to at most 255 over the groups with postings - and it is
// eligible from minScore up.  groupWeight holds one entry per group (an excluded group's is ignored); nil: every weight is 1.
// Everything else - groups, ranges, groupNot, the order, the buffers, k == 0 - is TopKRanges'.
func (c *Ctx) TopKWeightedRanges(groupFirst []uint64, groupNot []uint8, groupWeight []uint32, minScore uint32, k uint64, segs []*Segment, listFirst, listEnd []uint64, ids, scores unsafe.Pointer) (uint64, [256]uint64, TopKWStats, error) {
	var hist [256]uint64
	nGroups := len(groupFirst) - 1
	if nGroups < 0 || (groupNot != nil && len(groupNot) != nGroups) || (groupWeight != nil && len(groupWeight) != nGroups) || len(listFirst) != len(segs) || len(listEnd) != len(segs) {
		return 0, hist, TopKWStats{}, fmt.Errorf("topk weighted ranges: array lengths disagree")
	}
	if groupFirst[nGroups] != uint64(len(segs)) { // the C side reads the range arrays up to groupFirst's last element
		return 0, hist, TopKWStats{}, fmt.Errorf("topk weighted ranges: groupFirst does not end at the number of ranges")
	}
	hs := make([]*C.ii2_seg, len(segs)+1)
	for i, s := range segs {
		hs[i] = s.h
	}
	var flags *C.uint8_t
	if groupNot != nil && nGroups > 0 {
		flags = (*C.uint8_t)(unsafe.Pointer(&groupNot[0]))
	}
	var weights *C.uint32_t
	if groupWeight != nil && nGroups > 0 {
		weights = (*C.uint32_t)(unsafe.Pointer(&groupWeight[0]))
	}
	var n C.uint64_t
	var st C.ii2_topkw_stats
	rc := C.ii2_topk_weighted_ranges(c.h, C.uint64_t(nGroups), u64ptr(groupFirst), flags, weights, C.uint32_t(minScore), C.uint64_t(k),
		(**C.ii2_seg)(unsafe.Pointer(&hs[0])), u64ptr(listFirst), u64ptr(listEnd), nil, (*C.uint32_t)(ids), (*C.uint32_t)(scores), &n,
		(*C.uint64_t)(unsafe.Pointer(&hist[0])), &st)
	if rc != 0 {
		return 0, hist, TopKWStats{}, c.err("topk weighted ranges", rc)
	}
	stats := TopKWStats{uint64(st.n_counted), uint64(st.n_eligible), uint64(st.n_cut), uint32(st.total_weight), uint32(st.max_score), uint32(st.cut_score),
		uint32(st.n_planes), uint32(st.n_windows), uint32(st.n_marks), uint32(st.n_late)}
	return uint64(n), hist, stats, nil
}

// TopKWeightedRangesHost is TopKWeightedRanges with the result in host memory, as TopKRangesHost is TopKRanges'.
func (c *Ctx) TopKWeightedRangesHost(groupFirst []uint64, groupNot []uint8, groupWeight []uint32, minScore uint32, k uint64, segs []*Segment, listFirst, listEnd []uint64) ([]Scored, error) {
	if k == 0 {
		return nil, nil
	}
	var d unsafe.Pointer
	if rc := C.ii2_dev_alloc(c.h, C.size_t(2*k*4), &d); rc != 0 {
		return nil, c.err("topk weighted ranges", rc)
	}
	defer C.ii2_dev_free(c.h, d)
	n, _, _, err := c.TopKWeightedRanges(groupFirst, groupNot, groupWeight, minScore, k, segs, listFirst, listEnd, d, unsafe.Add(d, int(k*4)))
	if err != nil || n == 0 {
		return nil, err
	}
	raw := make([]uint32, k+n)
	if rc := C.ii2_copy_d2h(c.h, unsafe.Pointer(&raw[0]), d, C.size_t((k+n)*4)); rc != 0 {
		return nil, c.err("topk weighted ranges", rc)
	}
	out := make([]Scored, n)
	for i := range out {
		out[i] = Scored{raw[i], raw[k+uint64(i)]}
	}
	return out, nil
}

// TopKBatchStats mirrors ii2_topk_batch_stats.
type TopKBatchStats struct {
	Tiny, Small, Single, Empty uint32
	Staged                     uint64
}

// TopKBatch answers MANY ranked queries over resident segments in one call (ii2_topk_batch): query q owns the groups
// queryFirst[q] .. queryFirst[q+1]-1 - groupFirst, groupNot and the range arrays are those of QueryBatchGroups, groupWeight holds
// one entry per group of the batch (nil: every weight is 1) - and its result is what TopKWeightedRanges returns for those groups
// with minScore[q] (nil: every one is 1) and k[q]: the same ids in the same order, the same scores.  The results are packed back
// to back in query order into the device buffers ids and scores (capEntries entries each; scores may be nil; the sum of the k[q]
// is always enough); the returned offsets (len(queryFirst)) delimit them and eligible[q] is query q's number of eligible docs.
// All-or-nothing: on ErrCapacity nothing was written and the last offset is the capacity to call again with.
func (c *Ctx) TopKBatch(queryFirst, groupFirst []uint64, groupNot []uint8, groupWeight, minScore, k []uint32, segs []*Segment, listFirst, listEnd []uint64, ids, scores unsafe.Pointer, capEntries uint64) ([]uint64, []uint64, TopKBatchStats, error) {
	nQueries := len(queryFirst) - 1
	nGroups := len(groupFirst) - 1
	if nQueries < 0 || nGroups < 0 || (groupNot != nil && len(groupNot) != nGroups) || (groupWeight != nil && len(groupWeight) != nGroups) ||
		(minScore != nil && len(minScore) != nQueries) || len(k) != nQueries || len(listFirst) != len(segs) || len(listEnd) != len(segs) {
		return nil, nil, TopKBatchStats{}, fmt.Errorf("topk batch: array lengths disagree")
	}
	// the C side reads groupFirst[0 .. queryFirst[nQueries]] and the range arrays up to groupFirst's last element
	if queryFirst[nQueries] != uint64(nGroups) || groupFirst[nGroups] != uint64(len(segs)) {
		return nil, nil, TopKBatchStats{}, fmt.Errorf("topk batch: queryFirst / groupFirst do not end at the lengths of the arrays they index")
	}
	offsets := make([]uint64, nQueries+1)
	eligible := make([]uint64, nQueries+1)
	if nQueries == 0 {
		return offsets, eligible[:0], TopKBatchStats{}, nil
	}
	hs := make([]*C.ii2_seg, len(segs)+1)
	for i, s := range segs {
		hs[i] = s.h
	}
	var flags *C.uint8_t
	if len(groupNot) != 0 {
		flags = (*C.uint8_t)(unsafe.Pointer(&groupNot[0]))
	}
	var weights, mins *C.uint32_t
	if len(groupWeight) != 0 {
		weights = (*C.uint32_t)(unsafe.Pointer(&groupWeight[0]))
	}
	if len(minScore) != 0 {
		mins = (*C.uint32_t)(unsafe.Pointer(&minScore[0]))
	}
	var st C.ii2_topk_batch_stats
	rc := C.ii2_topk_batch(c.h, C.uint64_t(nQueries), u64ptr(queryFirst), u64ptr(groupFirst), flags, weights, mins,
		(*C.uint32_t)(unsafe.Pointer(&k[0])), (**C.ii2_seg)(unsafe.Pointer(&hs[0])), u64ptr(listFirst), u64ptr(listEnd), nil, (*C.uint32_t)(ids),
		(*C.uint32_t)(scores), C.uint64_t(capEntries), u64ptr(offsets), u64ptr(eligible), &st)
	stats := TopKBatchStats{uint32(st.n_tiny), uint32(st.n_small), uint32(st.n_single), uint32(st.n_empty), uint64(st.n_staged)}
	if rc == C.II2_ECAPACITY {
		return offsets, eligible[:nQueries], stats, ErrCapacity
	}
	if rc != 0 {
		return nil, nil, TopKBatchStats{}, c.err("topk batch", rc)
	}
	return offsets, eligible[:nQueries], stats, nil
}

// TopKBatchHost is TopKBatch with the results in host memory, one slice per query: a first call with capEntries entries, a second
// one with the size the first reported when they did not fit, and one download.
func (c *Ctx) TopKBatchHost(queryFirst, groupFirst []uint64, groupNot []uint8, groupWeight, minScore, k []uint32, segs []*Segment, listFirst, listEnd []uint64, capEntries uint64) ([][]Scored, error) {
	out := make([][]Scored, len(k))
	if capEntries == 0 {
		capEntries = 1
	}
	for attempt := 0; ; attempt++ {
		var d unsafe.Pointer
		if rc := C.ii2_dev_alloc(c.h, C.size_t(2*capEntries*4), &d); rc != 0 {
			return nil, c.err("topk batch", rc)
		}
		off, _, _, err := c.TopKBatch(queryFirst, groupFirst, groupNot, groupWeight, minScore, k, segs, listFirst, listEnd, d, unsafe.Add(d, int(capEntries*4)), capEntries)
		if err == ErrCapacity && attempt == 0 {
			C.ii2_dev_free(c.h, d)
			capEntries = off[len(off)-1]
			continue
		}
		if err != nil {
			C.ii2_dev_free(c.h, d)
			return nil, err
		}
		if n := off[len(off)-1]; n != 0 {
			raw := make([]uint32, capEntries+n)
			if rc := C.ii2_copy_d2h(c.h, unsafe.Pointer(&raw[0]), d, C.size_t((capEntries+n)*4)); rc != 0 {
				C.ii2_dev_free(c.h, d)
				return nil, c.err("topk batch", rc)
			}
			for q := range out {
				for i := off[q]; i < off[q+1]; i++ {
					out[q] = append(out[q], Scored{raw[i], raw[capEntries+i]})
				}
			}
		}
		C.ii2_dev_free(c.h, d)
		return out, nil
	}
}

// CountStats mirrors ii2_count_stats.
type CountStats struct {
	Lists, Blocks, Decoded, Hits uint64
	Windows                      uint32
}

// CountRanges is the facet count (ii2_count_ranges): per list named by the ranges - lists [listFirst[i], listEnd[i]) of
// segs[i], in range order - the number of its ids that lie in the doc set, one pass over the encoded lists whatever their
// number.  set is a device buffer of nSet ascending, duplicate-free ids, what every query entry point writes (AndNotRanges,
// QueryBatch ...); set == nil means every doc: the lists' lengths.  A list named twice is counted twice; an empty list gets 0.
func (c *Ctx) CountRanges(segs []*Segment, listFirst, listEnd []uint64, set unsafe.Pointer, nSet uint64) ([]uint64, CountStats, error) {
	if len(listFirst) != len(segs) || len(listEnd) != len(segs) {
		return nil, CountStats{}, fmt.Errorf("count ranges: array lengths disagree")
	}
	var named uint64
	for i := range segs {
		if listEnd[i] < listFirst[i] {
			return nil, CountStats{}, fmt.Errorf("count ranges: range %d ends before it begins", i)
		}
		named += listEnd[i] - listFirst[i]
	}
	hs := make([]*C.ii2_seg, len(segs)+1)
	for i, s := range segs {
		hs[i] = s.h
	}
	counts := make([]uint64, named)
	var st C.ii2_count_stats
	rc := C.ii2_count_ranges(c.h, C.uint64_t(len(segs)), (**C.ii2_seg)(unsafe.Pointer(&hs[0])), u64ptr(listFirst), u64ptr(listEnd),
		(*C.uint32_t)(set), C.uint64_t(nSet), nil, u64ptr(counts), C.uint64_t(named), &st)
	if rc != 0 {
		return nil, CountStats{}, c.err("count ranges", rc)
	}
	return counts, CountStats{uint64(st.n_lists), uint64(st.n_blocks), uint64(st.n_decoded), uint64(st.n_hits), uint32(st.n_windows)}, nil
}

// HistStats mirrors ii2_hist_stats.
type HistStats struct {
	Lists, Blocks, Decoded, Hits, Whole, Split, Wide uint64
	Windows, Buckets                                 uint32
}

// HistogramRanges is CountRanges over a value axis (ii2_histogram_ranges): edges holds nBuckets + 1 strictly ascending values, each
// <= 2^32, bucket b is the ids edges[b] <= id < edges[b+1]; ids outside the axis are counted nowhere.  counts[k*nBuckets+b] is
// the ids of the k-th list named in bucket b that lie in the doc set.  Ranges and set as CountRanges takes them; set == nil means
// every doc.
func (c *Ctx) HistogramRanges(segs []*Segment, listFirst, listEnd []uint64, set unsafe.Pointer, nSet uint64, edges []uint64) ([]uint64, HistStats, error) {
	if len(listFirst) != len(segs) || len(listEnd) != len(segs) {
		return nil, HistStats{}, fmt.Errorf("histogram ranges: array lengths disagree")
	}
	if len(edges) < 2 {
		return nil, HistStats{}, fmt.Errorf("histogram ranges: fewer than two edges")
	}
	nb := uint64(len(edges) - 1)
	var named uint64
	for i := range segs {
		if listEnd[i] < listFirst[i] {
			return nil, HistStats{}, fmt.Errorf("histogram ranges: range %d ends before it begins", i)
		}
		named += listEnd[i] - listFirst[i]
	}
	hs := make([]*C.ii2_seg, len(segs)+1)
	for i, s := range segs {
		hs[i] = s.h
	}
	counts := make([]uint64, named*nb)
	var st C.ii2_hist_stats
	rc := C.ii2_histogram_ranges(c.h, C.uint64_t(len(segs)), (**C.ii2_seg)(unsafe.Pointer(&hs[0])), u64ptr(listFirst), u64ptr(listEnd),
		(*C.uint32_t)(set), C.uint64_t(nSet), nil, C.uint32_t(nb), u64ptr(edges), u64ptr(counts), C.uint64_t(named*nb), &st)
	if rc != 0 {
		return nil, HistStats{}, c.err("histogram ranges", rc)
	}
	return counts, HistStats{uint64(st.n_lists), uint64(st.n_blocks), uint64(st.n_decoded), uint64(st.n_hits), uint64(st.n_whole),
		uint64(st.n_split), uint64(st.n_wide), uint32(st.n_windows), uint32(st.n_buckets)}, nil
}

// HistogramIDs counts a device set per bucket of a value axis (ii2_histogram_ids): set is a device buffer of nSet ascending,
// duplicate-free ids, edges as HistogramRanges takes them.
func (c *Ctx) HistogramIDs(set unsafe.Pointer, nSet uint64, edges []uint64) ([]uint64, error) {
	if len(edges) < 2 {
		return nil, fmt.Errorf("histogram ids: fewer than two edges")
	}
	counts := make([]uint64, len(edges)-1)
	rc := C.ii2_histogram_ids(c.h, (*C.uint32_t)(set), C.uint64_t(nSet), nil, C.uint32_t(len(edges)-1), u64ptr(edges), u64ptr(counts),
		C.uint64_t(len(counts)))
	if rc != 0 {
		return nil, c.err("histogram ids", rc)
	}
	return counts, nil
}

// ExplainStats mirrors ii2_explain_stats.
type ExplainStats struct {
	IDs, Lists, Blocks, Decoded, Hits uint64
	Windows, Words, Log2Slots         uint32
}

// ExplainRanges says which groups each doc lies in (ii2_explain_ranges): group g is the ranges groupFirst[g] ..
// groupFirst[g+1]-1 - lists [listFirst[i], listEnd[i]) of segs[i] - exactly as IntersectRanges takes them.  ids is a device
// buffer of nIDs doc ids in any order: a query's ascending result or a ranked page (TopkRanges).  Returns nIDs rows of
// words = ceil(groups / 64) mask words, doc-major: bit g&63 of word i*words + g>>6 is set when ids[i] lies in a list of group g.
// An id given twice has its mask in its first row and zeros after.  One pass over the groups' blocks, whatever their number.
func (c *Ctx) ExplainRanges(groupFirst []uint64, segs []*Segment, listFirst, listEnd []uint64, ids unsafe.Pointer, nIDs uint64) ([]uint64, ExplainStats, error) {
	if len(groupFirst) == 0 || len(listFirst) != len(segs) || len(listEnd) != len(segs) || groupFirst[len(groupFirst)-1] != uint64(len(segs)) {
		return nil, ExplainStats{}, fmt.Errorf("explain ranges: array lengths disagree")
	}
	nGroups := uint64(len(groupFirst) - 1)
	words := (nGroups + 63) / 64
	hs := make([]*C.ii2_seg, len(segs)+1)
	for i, s := range segs {
		hs[i] = s.h
	}
	masks := make([]uint64, nIDs*words)
	var d unsafe.Pointer
	if rc := C.ii2_dev_alloc(c.h, C.size_t((nIDs*words+1)*8), &d); rc != 0 {
		return nil, ExplainStats{}, c.err("explain ranges", rc)
	}
	var st C.ii2_explain_stats
	rc := C.ii2_explain_ranges(c.h, C.uint64_t(nGroups), u64ptr(groupFirst), (**C.ii2_seg)(unsafe.Pointer(&hs[0])), u64ptr(listFirst), u64ptr(listEnd),
		(*C.uint32_t)(ids), C.uint64_t(nIDs), (*C.uint64_t)(d), C.uint64_t(nIDs*words), &st)
	if rc == 0 && len(masks) > 0 {
		rc = C.ii2_copy_d2h(c.h, unsafe.Pointer(&masks[0]), d, C.size_t(len(masks)*8))
	}
	C.ii2_dev_free(c.h, d)
	if rc != 0 {
		return nil, ExplainStats{}, c.err("explain ranges", rc)
	}
	return masks, ExplainStats{uint64(st.n_ids), uint64(st.n_lists), uint64(st.n_blocks), uint64(st.n_decoded), uint64(st.n_hits),
		uint32(st.n_windows), uint32(st.n_words), uint32(st.log2_slots)}, nil
}

// ExplainBatchStats mirrors ii2_explain_batch_stats.
type ExplainBatchStats struct {
	Tiny, Small, Single, Empty uint32
	Rows, Words, Hits          uint64
}

// ExplainBatchIDs is II2_EXPLAIN_BATCH_IDS: the ids of a page the batch kernel takes.
const ExplainBatchIDs = 1024

// ExplainBatch is ExplainRanges for many pages in one call (ii2_explain_batch): query q owns the groups queryFirst[q] ..
// queryFirst[q+1]-1, exactly as QueryBatchGroups takes them, and explains the ids ids[idsOff[q] .. idsOff[q+1]) of the device
// buffer ids - the buffer and the offsets TopKBatch and QueryBatchGroups hand back.  Returns the packed masks and maskOff: query
// q's rows, (idsOff[q+1]-idsOff[q]) x ceil(groups of q / 64) words, start at word maskOff[q] and are what ExplainRanges returns for
// that query alone.  The queries that fit one workgroup share one launch and one wait.
func (c *Ctx) ExplainBatch(queryFirst, groupFirst []uint64, segs []*Segment, listFirst, listEnd []uint64, ids unsafe.Pointer, idsOff []uint64) ([]uint64, []uint64, ExplainBatchStats, error) {
	if len(queryFirst) == 0 || len(groupFirst) == 0 || len(idsOff) != len(queryFirst) || len(listFirst) != len(segs) || len(listEnd) != len(segs) ||
		queryFirst[len(queryFirst)-1] != uint64(len(groupFirst)-1) || groupFirst[len(groupFirst)-1] != uint64(len(segs)) {
		return nil, nil, ExplainBatchStats{}, fmt.Errorf("explain batch: array lengths disagree")
	}
	nQ := len(queryFirst) - 1
	maskOff := make([]uint64, nQ+1)
	for q := 0; q < nQ; q++ {
		if queryFirst[q+1] < queryFirst[q] || idsOff[q+1] < idsOff[q] {
			return nil, nil, ExplainBatchStats{}, fmt.Errorf("explain batch: query %d: offsets do not ascend", q)
		}
		maskOff[q+1] = maskOff[q] + (idsOff[q+1]-idsOff[q])*((queryFirst[q+1]-queryFirst[q]+63)/64)
	}
	total := maskOff[nQ]
	hs := make([]*C.ii2_seg, len(segs)+1)
	for i, s := range segs {
		hs[i] = s.h
	}
	masks := make([]uint64, total)
	var d unsafe.Pointer
	if rc := C.ii2_dev_alloc(c.h, C.size_t((total+1)*8), &d); rc != 0 {
		return nil, nil, ExplainBatchStats{}, c.err("explain batch", rc)
	}
	var st C.ii2_explain_batch_stats
	rc := C.ii2_explain_batch(c.h, C.uint64_t(nQ), u64ptr(queryFirst), u64ptr(groupFirst), (**C.ii2_seg)(unsafe.Pointer(&hs[0])), u64ptr(listFirst),
		u64ptr(listEnd), (*C.uint32_t)(ids), u64ptr(idsOff), (*C.uint64_t)(d), C.uint64_t(total), u64ptr(maskOff), &st)
	if rc == 0 && total > 0 {
		rc = C.ii2_copy_d2h(c.h, unsafe.Pointer(&masks[0]), d, C.size_t(total*8))
	}
	C.ii2_dev_free(c.h, d)
	if rc != 0 {
		return nil, nil, ExplainBatchStats{}, c.err("explain batch", rc)
	}
	return masks, maskOff, ExplainBatchStats{uint32(st.n_tiny), uint32(st.n_small), uint32(st.n_single), uint32(st.n_empty),
		uint64(st.n_rows), uint64(st.n_words), uint64(st.n_hits)}, nil
}

// ExplainBatchHost is ExplainBatch for ids in host memory: one upload of all ids, the call, one download.
func (c *Ctx) ExplainBatchHost(queryFirst, groupFirst []uint64, segs []*Segment, listFirst, listEnd []uint64, ids []uint32, idsOff []uint64) ([]uint64, []uint64, error) {
	var d unsafe.Pointer
	if rc := C.ii2_dev_alloc(c.h, C.size_t((len(ids)+1)*4), &d); rc != 0 {
		return nil, nil, c.err("explain batch", rc)
	}
	defer C.ii2_dev_free(c.h, d)
	if len(ids) > 0 {
		if rc := C.ii2_copy_h2d(c.h, d, unsafe.Pointer(&ids[0]), C.size_t(len(ids)*4)); rc != 0 {
			return nil, nil, c.err("explain batch", rc)
		}
	}
	masks, maskOff, _, err := c.ExplainBatch(queryFirst, groupFirst, segs, listFirst, listEnd, d, idsOff)
	return masks, maskOff, err
}

// Union replaces PrefixSearch's append + slices.Sort + slices.Compact (inverted_index.go:274-292).
func (c *Ctx) Union(listOff []uint64, values, removed []uint32) ([]uint32, error) {
	return c.lists(true, listOff, values, removed)
}

// Intersect: ids present in every list (additive operator; the reference has none).
func (c *Ctx) Intersect(listOff []uint64, values, removed []uint32) ([]uint32, error) {
	return c.lists(false, listOff, values, removed)
}

func (c *Ctx) lists(union bool, listOff []uint64, values, removed []uint32) ([]uint32, error) {
	out := make([]uint32, len(values)+1)
	var n C.uint64_t
	var rc C.int
	if union {
		rc = C.ii2_union_host(c.h, C.uint32_t(len(listOff)-1), u64ptr(listOff), u32ptr(values), u32ptr(removed), C.uint64_t(len(removed)), u32ptr(out), C.uint64_t(len(out)), &n)
	} else {
		rc = C.ii2_intersect_host(c.h, C.uint32_t(len(listOff)-1), u64ptr(listOff), u32ptr(values), u32ptr(removed), C.uint64_t(len(removed)), u32ptr(out), C.uint64_t(len(out)), &n)
	}
	if rc != 0 {
		return nil, c.err("lists", rc)
	}
	return out[:n], nil
}
