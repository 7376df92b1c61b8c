package gpu

// Drop-in bodies for the reference's exported methods.  Signatures are the reference's own,
// verbatim (inverted_index.go:41,62,113,192,300; shard.go:72,127); what changes is that the
// posting work goes through Ctx.  The segment files, the vellum FST walk and the locks stay
// the reference's Go code ("host" below = the unchanged parts of package inverted_index_2).
//
//	func (ii *InvertedIndex) Merge(reqCount, mCount, concurrency int) (mergedSegmentsLen int64, err error)
//	func (ii *InvertedIndex) Read(min, max []byte) (go_iterators.Iterator[file.TermValues], error)
//	func (ii *InvertedIndex) PrefixSearch(prefixes [][]byte) (found map[string][]uint32, err error)
//	func (s *Shard) Merge(reqCount, mCount int) (mergedSegmentsLen int, err error)
//	func (s *Shard) Read(min, max []byte) (go_iterators.Iterator[file.TermValues], error)
//
// PrefixSearch: every prefix is one run of consecutive terms in each segment's sorted dictionary; collect the runs of ALL
// prefixes and make ONE Ctx.QueryBatch call (an OpOr query per prefix) and one download instead of a union per prefix - what
// the C++ host mirror's InvertedIndex::PrefixSearch does (host/host_index.cpp).

import (
	"bytes"
	"errors"
	"fmt"
	"sort"
	"sync"
	"sync/atomic"
)

// TermValues mirrors file.TermValues (file/types.go:9-12).
type TermValues struct {
	Term   []byte
	Values []uint32
}

// EmptyIterator mirrors go_iterators.EmptyIterator: the sentinel Next returns at the end
// (shard.go:170, file/reader.go:41).
var EmptyIterator = errors.New("iterator is empty")

// Iterator mirrors go_iterators.Iterator[T].  Close MUST be called: it releases the segment
// read-locks taken by Shard.Read (shard.go:69-71,268-275).
type Iterator[T any] interface {
	Next() (T, error)
	Close() error
}

// HostShard is what the unchanged Go host code provides per shard: the term-aligned CSR of the
// segments a merge picked (FST walk, shard.go:127-158) and the writer for the result.
type HostShard interface {
	// PickAndLock picks <= mCount smallest segments with the merging CAS (shard.go:135-151) and
	// read-locks them; n < 2 means "nothing to merge".
	PickAndLock(reqCount, mCount int) (n int, err error)
	// Dictionaries returns the picked (or, for Read, all read-locked) segments' sorted term
	// dictionaries, flat, restricted to [min, max] (file/reader.go:33-71).
	Dictionaries(min, max []byte) (termBytes []byte, termOff, segFirst []uint64)
	// Postings returns segment s's decoded lists for the given source lists (-1 = empty slot).
	Postings(s int, srcList []int64) (off []uint64, values []uint32, err error)
	RemovedValues() []uint32 // removed_list.go:44-54
	// WriteMerged appends the surviving terms to a new segment and swaps it in (shard.go:197-242).
	WriteMerged(terms [][]byte, off []uint64, values []uint32) error
	Release() // readRelease / detach (shard.go:214,228-242)
}

// ShardMerge is the body of Shard.Merge (shard.go:127-245) with the loop :163-212 on the GPU.
//
// This body hands host slices over (MergeAligned = ii2_merge_host): the segments' postings cross PCIe on every call.  A shard
// that keeps its segments resident (Ctx.Encode once per segment, *Segment handles next to the file handles) replaces the
// whole body by ONE call for the usual merge of a few small segments - Ctx.MergeSmall (ii2_merge_small: alignment, union,
// removed-list filter, empty-term drop and encode in one launch, ~30 us) - and falls back to NewDictionary / AlignDicts /
// SelectAlignedAll / MergeSegmentsToSeg when it answers ErrTooLarge.  ShardRead likewise: Ctx.ReadSmall (ii2_read_small).
func ShardMerge(c *Ctx, s HostShard, reqCount, mCount int) (mergedSegmentsLen int, err error) {
	n, err := s.PickAndLock(reqCount, mCount)
	if err != nil || n < 2 {
		return 0, err
	}
	defer s.Release()
	tb, toff, first := s.Dictionaries(nil, nil)
	al, err := c.AlignTerms(tb, toff, first) // k-way dictionary merge on the device
	if err != nil {
		return 0, fmt.Errorf("s: merge: %w", err)
	}
	defer al.Free()
	rep, src, err := c.Export(al)
	if err != nil {
		return 0, fmt.Errorf("s: merge: %w", err)
	}
	nT := al.NUnion
	segOff := make([]uint64, 0, uint64(n)*(nT+1))
	segBase := make([]uint64, 1, n+1)
	var values []uint32
	for k := 0; k < n; k++ {
		off, v, perr := s.Postings(k, src[uint64(k)*nT:uint64(k+1)*nT])
		if perr != nil {
			return 0, fmt.Errorf("s: merge: %w", perr)
		}
		segOff = append(segOff, off...)
		values = append(values, v...)
		segBase = append(segBase, uint64(len(values)))
	}
	outOff, outVals, termsOut, err := c.MergeAligned(n, nT, segOff, segBase, values, s.RemovedValues())
	if err != nil {
		return 0, fmt.Errorf("s: merge: %w", err)
	}
	if termsOut > 0 { // lazy writer: nothing survives -> no segment (shard.go:219-225)
		terms := make([][]byte, 0, termsOut)
		off := make([]uint64, 1, termsOut+1)
		for t := uint64(0); t < nT; t++ {
			if outOff[t+1] > outOff[t] { // drop emptied terms (shard.go:192-194)
				terms = append(terms, tb[toff[rep[t]]:toff[rep[t]+1]])
				off = append(off, outOff[t+1])
			}
		}
		if err = s.WriteMerged(terms, off, outVals); err != nil {
			return 0, fmt.Errorf("s: merge: %w", err)
		}
	}
	return n, nil
}

// Doc is one Put: the terms of a document and its value.
type Doc struct {
	Terms [][]byte
	Val   uint32
}

// BatchShard is what the unchanged Go host code provides for a bulk Put: a place for one ordinary (non-direct) segment.
type BatchShard interface {
	// AddSegment makes a segment visible under a fresh key exactly as Put adds its own (shard.go:64): terms is its sorted
	// dictionary, seg holds one list per term.  A shard on disk writes it like a merged segment first (file.NewWriter: term
	// file, then the value file from Ctx.ExportSegment, both renamed when complete).
	AddSegment(terms [][]byte, seg *Segment) error
}

// PutBatch is the bulk form of Shard.Put (additive; shard.go:33-67 N times plus the merges shard.go:163-212 that would fold the
// N direct segments): the shard's dictionary is the sorted, duplicate-free terms of all docs (bytes.Compare order), every
// (doc, term) is one (index of the term, val) pair, and ONE Ctx.SegBuild call sorts and encodes them into one segment.  No docs
// or no terms: no segment.  Put itself is unchanged.
func PutBatch(c *Ctx, s BatchShard, docs []Doc) error {
	var terms [][]byte
	for _, d := range docs {
		terms = append(terms, d.Terms...)
	}
	if len(terms) == 0 {
		return nil
	}
	sort.Slice(terms, func(i, j int) bool { return bytes.Compare(terms[i], terms[j]) < 0 })
	n := 1
	for i := 1; i < len(terms); i++ { // slices.Compact by bytes.Equal
		if !bytes.Equal(terms[i], terms[n-1]) {
			terms[n] = terms[i]
			n++
		}
	}
	terms = terms[:n]
	var listID, vals []uint32
	for _, d := range docs {
		for _, t := range d.Terms {
			i := sort.Search(len(terms), func(i int) bool { return bytes.Compare(terms[i], t) >= 0 })
			listID = append(listID, uint32(i))
			vals = append(vals, d.Val)
		}
	}
	seg, _, err := c.SegBuild(uint64(len(terms)), listID, vals)
	if err != nil {
		return fmt.Errorf("s: put batch: %w", err)
	}
	if err = s.AddSegment(terms, seg); err != nil {
		seg.Free()
		return fmt.Errorf("s: put batch: %w", err)
	}
	return nil
}

// IndexPutBatch is the bulk form of InvertedIndex.Put (inverted_index.go:113-145): every doc's terms are grouped by shardKey
// (shard.go:362-378) as Put groups them, and each shard that receives something gets one PutBatch.  shardOf returns the shard
// of a key, creating it when needed (newShard, inverted_index.go:163-190).
func IndexPutBatch(c *Ctx, shardKey func(term []byte) uint16, shardOf func(key uint16) (BatchShard, error), docs []Doc) error {
	groups := map[uint16][]Doc{}
	var keys []uint16
	for _, d := range docs {
		mine := map[uint16][][]byte{}
		for _, t := range d.Terms {
			k := shardKey(t)
			mine[k] = append(mine[k], t)
		}
		for k, ts := range mine {
			if _, seen := groups[k]; !seen {
				keys = append(keys, k)
			}
			groups[k] = append(groups[k], Doc{ts, d.Val})
		}
	}
	sort.Slice(keys, func(i, j int) bool { return keys[i] < keys[j] })
	for _, k := range keys {
		s, err := shardOf(k)
		if err != nil {
			return fmt.Errorf("index put batch: %w", err)
		}
		if err = PutBatch(c, s, groups[k]); err != nil {
			return fmt.Errorf("index put batch: %w", err)
		}
	}
	return nil
}

// IndexMerge is the body of InvertedIndex.Merge (inverted_index.go:62-109): `concurrency` workers,
// one Ctx each, pull shards off one channel; a failing worker records the error and stops.
func IndexMerge(device int, shards []HostShard, reqCount, mCount, concurrency int) (mergedSegmentsLen int64, err error) {
	workCh := make(chan HostShard)
	go func() {
		for _, s := range shards {
			workCh <- s
		}
		close(workCh)
	}()
	var merged atomic.Int64
	var wg sync.WaitGroup
	for i := 0; i < concurrency; i++ {
		wg.Add(1)
		go func() {
			defer wg.Done()
			c, cerr := NewCtx(device)
			if cerr != nil {
				err = cerr
				return
			}
			defer c.Close()
			for s := range workCh {
				n, serr := ShardMerge(c, s, reqCount, mCount)
				if serr != nil {
					err = serr
					return
				}
				merged.Add(int64(n))
			}
		}()
	}
	wg.Wait()
	return merged.Load(), err
}

// readIterator serves Shard.Read / InvertedIndex.Read: the merged view is computed in one GPU
// call (no tombstones: the reference does not filter on read, shard.go:72-75) and then handed out
// term by term.  Next returns EmptyIterator at the end; Close releases the read-locks.
type readIterator struct {
	terms  [][]byte
	off    []uint64
	values []uint32
	pos    int
	host   HostShard
	closed bool
}

func (it *readIterator) Next() (tv TermValues, err error) {
	if it.pos >= len(it.terms) {
		return tv, EmptyIterator
	}
	tv = TermValues{Term: it.terms[it.pos], Values: it.values[it.off[it.pos]:it.off[it.pos+1]]}
	it.pos++
	return tv, nil
}

func (it *readIterator) Close() error {
	if !it.closed {
		it.closed = true
		it.host.Release()
	}
	return nil
}

// ShardRead is the body of Shard.Read (shard.go:72-75 + makeIterator :253-278); the caller has
// read-locked all segments (readLockAll, segments.go:32).
func ShardRead(c *Ctx, s HostShard, nSegs int, min, max []byte) (Iterator[TermValues], error) {
	tb, toff, first := s.Dictionaries(min, max)
	al, err := c.AlignTerms(tb, toff, first)
	if err != nil {
		s.Release()
		return nil, fmt.Errorf("index read: %w", err)
	}
	defer al.Free()
	rep, src, err := c.Export(al)
	if err != nil {
		s.Release()
		return nil, fmt.Errorf("index read: %w", err)
	}
	nT := al.NUnion
	var segOff, segBase []uint64
	var values []uint32
	segBase = append(segBase, 0)
	for k := 0; k < nSegs; k++ {
		off, v, perr := s.Postings(k, src[uint64(k)*nT:uint64(k+1)*nT])
		if perr != nil {
			s.Release()
			return nil, fmt.Errorf("index read: %w", perr)
		}
		segOff = append(segOff, off...)
		values = append(values, v...)
		segBase = append(segBase, uint64(len(values)))
	}
	outOff, outVals, _, err := c.MergeAligned(nSegs, nT, segOff, segBase, values, nil)
	if err != nil {
		s.Release()
		return nil, fmt.Errorf("index read: %w", err)
	}
	terms := make([][]byte, nT)
	for t := range terms {
		terms[t] = tb[toff[rep[t]]:toff[rep[t]+1]]
	}
	return &readIterator{terms: terms, off: outOff, values: outVals, host: s}, nil
}

// ResidentIndex is what a host that keeps its segments resident (Ctx.Encode once per segment) provides for the additive
// boolean queries: where a term's postings are.
type ResidentIndex interface {
	// TermLists returns, for every segment of the term's shard that holds the term, the resident segment and the term's list
	// index in it, and an upper bound of the term's postings (0 lists: the term is in no segment).  The segments stay
	// read-locked until Release.
	TermLists(term []byte) (segs []*Segment, lists []uint64, postingsBound uint64)
	Release()
}

// MatchIndex is what a host that keeps its segments and their dictionaries resident provides for MatchSearch: every segment of
// every shard with its resident dictionary (Ctx.DictCreate once per segment), in any fixed order.  The segments stay read-locked
// until Release.
type MatchIndex interface {
	ResidentSegments() (segs []*Segment, dicts []*Dictionary)
	Release()
}

// MatchSearch (additive): substring, suffix and wildcard search - for every pattern of kind (MatchContains / MatchSuffix /
// MatchGlob, | MatchNoCase) the ids under any term it matches, over every segment of every shard: a pattern selects no shard.
// Ctx.DictMatch per chunk of at most 64 dictionaries and 64 patterns turns the patterns into runs of lists, then ONE
// Ctx.QueryBatch call - an OpOr query per pattern over all its runs - and one download, with a second call when the results
// exceed the first buffer: what the C++ host mirror's InvertedIndex::MatchSearch does (host/host_index.cpp).  A pattern that
// matches no term has no entry.  Like Read, no tombstone filter.
func MatchSearch(c *Ctx, ix MatchIndex, patterns [][]byte, kind uint8) (found map[string][]uint32, err error) {
	defer ix.Release()
	segs, dicts := ix.ResidentSegments()
	type ranges struct {
		segs       []*Segment
		first, end []uint64
	}
	per := make([]ranges, len(patterns))
	for p0 := 0; p0 < len(patterns); p0 += 64 {
		p1 := p0 + 64
		if p1 > len(patterns) {
			p1 = len(patterns)
		}
		kinds := make([]uint8, p1-p0)
		for i := range kinds {
			kinds[i] = kind
		}
		for s0 := 0; s0 < len(dicts); s0 += 64 {
			s1 := s0 + 64
			if s1 > len(dicts) {
				s1 = len(dicts)
			}
			k := s1 - s0
			runOff, first, end, dict, _, err := c.DictMatch(dicts[s0:s1], patterns[p0:p1], kinds)
			if err != nil {
				return nil, fmt.Errorf("match search: %w", err)
			}
			for p := 0; p < p1-p0; p++ {
				r := &per[p0+p]
				for j := runOff[p*k]; j < runOff[(p+1)*k]; j++ {
					r.segs = append(r.segs, segs[s0+int(dict[j])])
					r.first = append(r.first, first[j])
					r.end = append(r.end, end[j])
				}
			}
		}
	}
	var names []string
	var op []uint8
	queryFirst := []uint64{0}
	var qsegs []*Segment
	var qfirst, qend []uint64
	seen := map[string]bool{}
	for p, r := range per {
		if len(r.segs) == 0 || seen[string(patterns[p])] {
			continue
		}
		seen[string(patterns[p])] = true
		names = append(names, string(patterns[p]))
		op = append(op, OpOr)
		qsegs = append(qsegs, r.segs...)
		qfirst = append(qfirst, r.first...)
		qend = append(qend, r.end...)
		queryFirst = append(queryFirst, uint64(len(qsegs)))
	}
	found = map[string][]uint32{}
	if len(names) == 0 {
		return found, nil
	}
	all, offs, err := c.QueryBatchHost(op, queryFirst, qsegs, qfirst, qend, uint64(1)<<22)
	if err != nil {
		return nil, fmt.Errorf("match search: %w", err)
	}
	for q, name := range names {
		found[name] = all[offs[q]:offs[q+1]]
	}
	return found, nil
}

// fuzzyRuns calls fn(p, segment index, j0, j1) for every run [j0, j1) of consecutive terms of every segment within maxDist edits of
// patterns[p]: Ctx.DictFuzzy per chunk of at most 64 dictionaries and 16 patterns.  A pattern shorter than prefix is compared as
// a whole.
func fuzzyRuns(c *Ctx, dicts []*Dictionary, patterns [][]byte, maxDist, prefix, flags uint8, fn func(p, seg int, j0, j1 uint64)) error {
	for p0 := 0; p0 < len(patterns); p0 += 16 {
		p1 := p0 + 16
		if p1 > len(patterns) {
			p1 = len(patterns)
		}
		dist, pre, fl := make([]uint8, p1-p0), make([]uint8, p1-p0), make([]uint8, p1-p0)
		for i := range dist {
			dist[i], pre[i], fl[i] = maxDist, prefix, flags
			if int(prefix) > len(patterns[p0+i]) {
				pre[i] = uint8(len(patterns[p0+i]))
			}
		}
		for s0 := 0; s0 < len(dicts); s0 += 64 {
			s1 := s0 + 64
			if s1 > len(dicts) {
				s1 = len(dicts)
			}
			k := s1 - s0
			runOff, first, end, dict, _, err := c.DictFuzzy(dicts[s0:s1], patterns[p0:p1], dist, pre, fl)
			if err != nil {
				return err
			}
			for p := 0; p < p1-p0; p++ {
				for j := runOff[p*k]; j < runOff[(p+1)*k]; j++ {
					fn(p0+p, s0+int(dict[j]), first[j], end[j])
				}
			}
		}
	}
	return nil
}

// FuzzySearch (additive): typo-tolerant search - for every query term the ids under any term within maxDist edits of it that
// shares its first prefix bytes (flags: FuzzyTranspose, MatchNoCase), over every segment of every shard.  Ctx.DictFuzzy per chunk
// of at most 64 dictionaries and 16 patterns turns the terms into runs of lists, then ONE Ctx.QueryBatch call - an OpOr query per
// term over all its runs - and one download, with a second call when the results exceed the first buffer: what the C++ host
// mirror's InvertedIndex::FuzzySearch does (host/host_index.cpp).  A term that matches nothing has no entry.  Like Read, no
// tombstone filter.
func FuzzySearch(c *Ctx, ix MatchIndex, terms [][]byte, maxDist, prefix, flags uint8) (found map[string][]uint32, err error) {
	defer ix.Release()
	segs, dicts := ix.ResidentSegments()
	type ranges struct {
		segs       []*Segment
		first, end []uint64
	}
	per := make([]ranges, len(terms))
	if err := fuzzyRuns(c, dicts, terms, maxDist, prefix, flags, func(p, seg int, j0, j1 uint64) {
		r := &per[p]
		r.segs = append(r.segs, segs[seg])
		r.first = append(r.first, j0)
		r.end = append(r.end, j1)
	}); err != nil {
		return nil, fmt.Errorf("fuzzy search: %w", err)
	}
	var names []string
	var op []uint8
	queryFirst := []uint64{0}
	var qsegs []*Segment
	var qfirst, qend []uint64
	seen := map[string]bool{}
	for p, r := range per {
		if len(r.segs) == 0 || seen[string(terms[p])] {
			continue
		}
		seen[string(terms[p])] = true
		names = append(names, string(terms[p]))
		op = append(op, OpOr)
		qsegs = append(qsegs, r.segs...)
		qfirst = append(qfirst, r.first...)
		qend = append(qend, r.end...)
		queryFirst = append(queryFirst, uint64(len(qsegs)))
	}
	found = map[string][]uint32{}
	if len(names) == 0 {
		return found, nil
	}
	all, offs, err := c.QueryBatchHost(op, queryFirst, qsegs, qfirst, qend, uint64(1)<<22)
	if err != nil {
		return nil, fmt.Errorf("fuzzy search: %w", err)
	}
	for q, name := range names {
		found[name] = all[offs[q]:offs[q+1]]
	}
	return found, nil
}

// FuzzyTerm is one answer of FuzzyTerms: a term and its exact distance to the pattern.
type FuzzyTerm struct {
	Term []byte
	Dist uint32
}

// FuzzyTerms (additive): the distinct terms within maxDist edits of the pattern with their distances, distance ascending, then in
// bytes.Compare order, at most limit.  The matched terms are read from the runs (Ctx.DictExport of the dictionaries that hold
// one) and only those get their distance, from TermFuzzy on the host: what InvertedIndex::FuzzyTerms does.
func FuzzyTerms(c *Ctx, ix MatchIndex, pattern []byte, maxDist, prefix, flags uint8, limit int) ([]FuzzyTerm, error) {
	defer ix.Release()
	_, dicts := ix.ResidentSegments()
	exported := map[int][][]byte{}
	seen := map[string]bool{}
	var out []FuzzyTerm
	var failed error
	if err := fuzzyRuns(c, dicts, [][]byte{pattern}, maxDist, prefix, flags, func(_, seg int, j0, j1 uint64) {
		if failed != nil {
			return
		}
		if _, ok := exported[seg]; !ok {
			exported[seg], failed = c.DictExport(dicts[seg])
			if failed != nil {
				return
			}
		}
		for _, t := range exported[seg][j0:j1] {
			if seen[string(t)] {
				continue
			}
			seen[string(t)] = true
			_, d, err := TermFuzzy(pattern, t, uint32(maxDist), 0, flags)
			if err != nil {
				failed = err
				return
			}
			out = append(out, FuzzyTerm{append([]byte{}, t...), d})
		}
	}); err != nil {
		return nil, fmt.Errorf("fuzzy terms: %w", err)
	}
	if failed != nil {
		return nil, fmt.Errorf("fuzzy terms: %w", failed)
	}
	sort.Slice(out, func(i, j int) bool {
		if out[i].Dist != out[j].Dist {
			return out[i].Dist < out[j].Dist
		}
		return bytes.Compare(out[i].Term, out[j].Term) < 0
	})
	if len(out) > limit {
		out = out[:limit]
	}
	return out, nil
}

// regexRuns calls fn(p, segment index, j0, j1) for every run [j0, j1) of consecutive terms of every segment that patterns[p] matches
// as a whole: Ctx.DictRegex per chunk of at most 64 dictionaries and 8 patterns.  Every pattern is parsed first (TermRegex), so
// that one that does not parse fails the call before any search runs.
func regexRuns(c *Ctx, dicts []*Dictionary, patterns [][]byte, flags uint8, fn func(p, seg int, j0, j1 uint64)) error {
	for _, p := range patterns {
		if _, _, err := TermRegex(p, nil, flags); err != nil {
			return fmt.Errorf("pattern %q: %w", p, err)
		}
	}
	for p0 := 0; p0 < len(patterns); p0 += 8 {
		p1 := p0 + 8
		if p1 > len(patterns) {
			p1 = len(patterns)
		}
		fl := make([]uint8, p1-p0)
		for i := range fl {
			fl[i] = flags
		}
		for s0 := 0; s0 < len(dicts); s0 += 64 {
			s1 := s0 + 64
			if s1 > len(dicts) {
				s1 = len(dicts)
			}
			k := s1 - s0
			runOff, first, end, dict, _, err := c.DictRegex(dicts[s0:s1], patterns[p0:p1], fl)
			if err != nil {
				return err
			}
			for p := 0; p < p1-p0; p++ {
				for j := runOff[p*k]; j < runOff[(p+1)*k]; j++ {
					fn(p0+p, s0+int(dict[j]), first[j], end[j])
				}
			}
		}
	}
	return nil
}

// RegexSearch (additive): regular-expression search - for every pattern the ids under any term it matches as a whole (flags: 0
// or MatchNoCase), over every segment of every shard.  Ctx.DictRegex per chunk of at most 64 dictionaries and 8 patterns turns
// the patterns into runs of lists, then ONE Ctx.QueryBatch call - an OpOr query per pattern over all its runs - and one download,
// with a second call when the results exceed the first buffer: what the C++ host mirror's InvertedIndex::RegexSearch does
// (host/host_index.cpp).  A pattern that matches nothing has no entry.  Like Read, no tombstone filter.
func RegexSearch(c *Ctx, ix MatchIndex, patterns [][]byte, flags uint8) (found map[string][]uint32, err error) {
	defer ix.Release()
	segs, dicts := ix.ResidentSegments()
	type ranges struct {
		segs       []*Segment
		first, end []uint64
	}
	per := make([]ranges, len(patterns))
	if err := regexRuns(c, dicts, patterns, flags, func(p, seg int, j0, j1 uint64) {
		r := &per[p]
		r.segs = append(r.segs, segs[seg])
		r.first = append(r.first, j0)
		r.end = append(r.end, j1)
	}); err != nil {
		return nil, fmt.Errorf("regex search: %w", err)
	}
	var names []string
	var op []uint8
	queryFirst := []uint64{0}
	var qsegs []*Segment
	var qfirst, qend []uint64
	seen := map[string]bool{}
	for p, r := range per {
		if len(r.segs) == 0 || seen[string(patterns[p])] {
			continue
		}
		seen[string(patterns[p])] = true
		names = append(names, string(patterns[p]))
		op = append(op, OpOr)
		qsegs = append(qsegs, r.segs...)
		qfirst = append(qfirst, r.first...)
		qend = append(qend, r.end...)
		queryFirst = append(queryFirst, uint64(len(qsegs)))
	}
	found = map[string][]uint32{}
	if len(names) == 0 {
		return found, nil
	}
	all, offs, err := c.QueryBatchHost(op, queryFirst, qsegs, qfirst, qend, uint64(1)<<22)
	if err != nil {
		return nil, fmt.Errorf("regex search: %w", err)
	}
	for q, name := range names {
		found[name] = all[offs[q]:offs[q+1]]
	}
	return found, nil
}

// RegexTerms (additive): the distinct terms the pattern matches, in bytes.Compare order, at most limit.  The matched terms are
// read from the runs (Ctx.DictExport of the dictionaries that hold one): what InvertedIndex::RegexTerms does.
func RegexTerms(c *Ctx, ix MatchIndex, pattern []byte, flags uint8, limit int) ([][]byte, error) {
	defer ix.Release()
	_, dicts := ix.ResidentSegments()
	exported := map[int][][]byte{}
	seen := map[string]bool{}
	var out [][]byte
	var failed error
	if err := regexRuns(c, dicts, [][]byte{pattern}, flags, func(_, seg int, j0, j1 uint64) {
		if failed != nil {
			return
		}
		if _, ok := exported[seg]; !ok {
			exported[seg], failed = c.DictExport(dicts[seg])
			if failed != nil {
				return
			}
		}
		for _, t := range exported[seg][j0:j1] {
			if !seen[string(t)] {
				seen[string(t)] = true
				out = append(out, append([]byte{}, t...))
			}
		}
	}); err != nil {
		return nil, fmt.Errorf("regex terms: %w", err)
	}
	if failed != nil {
		return nil, fmt.Errorf("regex terms: %w", failed)
	}
	sort.Slice(out, func(i, j int) bool { return bytes.Compare(out[i], out[j]) < 0 })
	if len(out) > limit {
		out = out[:limit]
	}
	return out, nil
}

// IntersectAtLeast (additive): the ids under at least minMatch of terms and under none of except - minimum-should-match, "any two
// of these tags".  One group per term as IntersectExcept builds them, but a required term found in no segment is a group without
// ranges (it matches no doc), not an empty result; ONE Ctx.AtLeastRanges call with one download - what the C++ host mirror's
// InvertedIndex::IntersectAtLeast does (host/host_index.cpp).  Like Read, no tombstone filter.
func IntersectAtLeast(c *Ctx, ix ResidentIndex, terms [][]byte, minMatch uint32, except [][]byte) ([]uint32, error) {
	if minMatch == 0 {
		return nil, fmt.Errorf("intersect at least: minMatch is 0")
	}
	defer ix.Release()
	const firstCap = uint64(1) << 22
	groupFirst := []uint64{0}
	var groupNot []uint8
	var segs []*Segment
	var first, end []uint64
	var posts []uint64 // the postings bounds of the terms that some segment holds
	for _, t := range terms {
		s, l, post := ix.TermLists(t)
		segs = append(segs, s...)
		for _, j := range l {
			first = append(first, j)
			end = append(end, j+1)
		}
		groupFirst = append(groupFirst, uint64(len(segs)))
		groupNot = append(groupNot, 0)
		if len(s) > 0 {
			if post == 0 {
				post = 1
			}
			posts = append(posts, post)
		}
	}
	if uint64(len(posts)) < uint64(minMatch) {
		return nil, nil
	}
	for _, t := range except {
		s, l, _ := ix.TermLists(t)
		if len(s) == 0 {
			continue // (in no segment: it removes nothing)
		}
		segs = append(segs, s...)
		for _, j := range l {
			first = append(first, j)
			end = append(end, j+1)
		}
		groupFirst = append(groupFirst, uint64(len(segs)))
		groupNot = append(groupNot, 1)
	}
	// a result id lies in at least one of any n' - minMatch + 1 terms: those with the smallest bounds
	sort.Slice(posts, func(a, b int) bool { return posts[a] < posts[b] })
	bound := uint64(0)
	for k := 0; k+int(minMatch) <= len(posts); k++ {
		bound += posts[k]
	}
	if bound > firstCap {
		bound = firstCap
	}
	ids, err := c.AtLeastRangesHost(groupFirst, groupNot, minMatch, segs, first, end, bound)
	if err != nil {
		return nil, fmt.Errorf("intersect at least: %w", err)
	}
	return ids, nil
}

// IntersectTop (additive): the k ids under the most of terms - at least minMatch of them, under none of except - with the number of
// terms each lies under, score descending, then id ascending: a ranked page of a search.  One group per term as IntersectAtLeast
// builds them (a required term found in no segment is a group without ranges), ONE Ctx.TopKRanges call with one download of the k
// (id, score) pairs - what the C++ host mirror's InvertedIndex::IntersectTop does (host/host_index.cpp).  Like Read, no tombstone
// filter.
func IntersectTop(c *Ctx, ix ResidentIndex, terms [][]byte, k uint64, minMatch uint32, except [][]byte) ([]Scored, error) {
	if minMatch == 0 {
		return nil, fmt.Errorf("intersect top: minMatch is 0")
	}
	if k > TopKMax {
		return nil, fmt.Errorf("intersect top: k above TopKMax")
	}
	defer ix.Release()
	groupFirst := []uint64{0}
	var groupNot []uint8
	var segs []*Segment
	var first, end []uint64
	held := uint32(0) // the terms that some segment holds
	for _, t := range terms {
		s, l, _ := ix.TermLists(t)
		segs = append(segs, s...)
		for _, j := range l {
			first = append(first, j)
			end = append(end, j+1)
		}
		groupFirst = append(groupFirst, uint64(len(segs)))
		groupNot = append(groupNot, 0)
		if len(s) > 0 {
			held++
		}
	}
	if held < minMatch || k == 0 {
		return nil, nil
	}
	for _, t := range except {
		s, l, _ := ix.TermLists(t)
		if len(s) == 0 {
			continue // (in no segment: it removes nothing)
		}
		segs = append(segs, s...)
		for _, j := range l {
			first = append(first, j)
			end = append(end, j+1)
		}
		groupFirst = append(groupFirst, uint64(len(segs)))
		groupNot = append(groupNot, 1)
	}
	top, err := c.TopKRangesHost(groupFirst, groupNot, minMatch, k, segs, first, end)
	if err != nil {
		return nil, fmt.Errorf("intersect top: %w", err)
	}
	return top, nil
}

// IntersectTopWeighted (additive): IntersectTop with a weight per term - an idf tier, a field boost.  A doc's score is the sum of
// weights[i] over the terms[i] it lies under (1 .. 255 each, at most 255 together), at least minScore.  The groups are IntersectTop's:
// a term found in no segment keeps its slot, and its weight, and matches nothing.  ONE Ctx.TopKWeightedRanges call with one download
// - what the C++ host mirror's InvertedIndex::IntersectTopWeighted does (host/host_index.cpp).
func IntersectTopWeighted(c *Ctx, ix ResidentIndex, terms [][]byte, weights []uint32, k uint64, minScore uint32, except [][]byte) ([]Scored, error) {
	if minScore == 0 {
		return nil, fmt.Errorf("intersect top weighted: minScore is 0")
	}
	if len(weights) != len(terms) {
		return nil, fmt.Errorf("intersect top weighted: one weight per term")
	}
	if k > TopKMax {
		return nil, fmt.Errorf("intersect top weighted: k above TopKMax")
	}
	defer ix.Release()
	groupFirst := []uint64{0}
	var groupNot []uint8
	var segs []*Segment
	var first, end []uint64
	groupWeight := append([]uint32(nil), weights...)
	held := 0 // the terms that some segment holds
	for _, t := range terms {
		s, l, _ := ix.TermLists(t)
		segs = append(segs, s...)
		for _, j := range l {
			first = append(first, j)
			end = append(end, j+1)
		}
		groupFirst = append(groupFirst, uint64(len(segs)))
		groupNot = append(groupNot, 0)
		if len(s) > 0 {
			held++
		}
	}
	if held == 0 || k == 0 {
		return nil, nil
	}
	for _, t := range except {
		s, l, _ := ix.TermLists(t)
		if len(s) == 0 {
			continue // (in no segment: it removes nothing)
		}
		segs = append(segs, s...)
		for _, j := range l {
			first = append(first, j)
			end = append(end, j+1)
		}
		groupFirst = append(groupFirst, uint64(len(segs)))
		groupNot = append(groupNot, 1)
		groupWeight = append(groupWeight, 0) // (ignored)
	}
	top, err := c.TopKWeightedRangesHost(groupFirst, groupNot, groupWeight, minScore, k, segs, first, end)
	if err != nil {
		return nil, fmt.Errorf("intersect top weighted: %w", err)
	}
	return top, nil
}

// TopQuery is one query of IntersectTopBatch: IntersectTopWeighted's arguments.
type TopQuery struct {
	Terms    [][]byte
	Weights  []uint32
	K        uint64
	MinScore uint32
	Except   [][]byte
}

// IntersectTopBatch (additive): MANY IntersectTopWeighted queries in one device call; result q is that of IntersectTopWeighted for
// queries[q].  Per query the groups are built exactly as IntersectTopWeighted builds them; a query none of whose terms is in a
// segment, or with K == 0, keeps its place without a group - its result is empty.  ONE Ctx.TopKBatch call, a second one when the
// results exceed the first buffer of at most 4M entries, and one download - what the C++ host mirror's
// InvertedIndex::IntersectTopBatch does (host/host_index.cpp).
func IntersectTopBatch(c *Ctx, ix ResidentIndex, queries []TopQuery) ([][]Scored, error) {
	if len(queries) == 0 {
		return nil, nil
	}
	defer ix.Release()
	const firstCap = uint64(1) << 22
	queryFirst, groupFirst := []uint64{0}, []uint64{0}
	var groupNot []uint8
	var groupWeight, minScore, ks []uint32
	var segs []*Segment
	var first, end []uint64
	total := uint64(0)
	for q, Q := range queries {
		if Q.MinScore == 0 {
			return nil, fmt.Errorf("intersect top batch: query %d: minScore is 0", q)
		}
		if len(Q.Weights) != len(Q.Terms) {
			return nil, fmt.Errorf("intersect top batch: query %d: one weight per term", q)
		}
		if Q.K > TopKMax {
			return nil, fmt.Errorf("intersect top batch: query %d: k above TopKMax", q)
		}
		minScore = append(minScore, Q.MinScore)
		ks = append(ks, uint32(Q.K))
		gMark, rMark := len(groupNot), len(segs)
		posts := uint64(0)
		add := func(t []byte, not uint8, w uint32) {
			s, l, post := ix.TermLists(t)
			if len(s) == 0 && not == 1 {
				return // (an excluded term in no segment removes nothing)
			}
			segs = append(segs, s...)
			for _, j := range l {
				first = append(first, j)
				end = append(end, j+1)
			}
			groupFirst = append(groupFirst, uint64(len(segs)))
			groupNot = append(groupNot, not)
			groupWeight = append(groupWeight, w)
			if not == 0 && len(s) > 0 {
				if post == 0 {
					post = 1
				}
				posts += post
			}
		}
		for i, t := range Q.Terms {
			add(t, 0, Q.Weights[i])
		}
		if posts != 0 && Q.K != 0 {
			for _, t := range Q.Except {
				add(t, 1, 0)
			}
			if Q.K < posts {
				posts = Q.K
			}
			total += posts
		} else { // the query keeps its place, without a group
			groupFirst, groupNot, groupWeight = groupFirst[:gMark+1], groupNot[:gMark], groupWeight[:gMark]
			segs, first, end = segs[:rMark], first[:rMark], end[:rMark]
		}
		queryFirst = append(queryFirst, uint64(len(groupNot)))
	}
	capEntries := total
	if capEntries > firstCap {
		capEntries = firstCap
	}
	if capEntries == 0 {
		capEntries = 1
	}
	out, err := c.TopKBatchHost(queryFirst, groupFirst, groupNot, groupWeight, minScore, ks, segs, first, end, capEntries)
	if err != nil {
		return nil, fmt.Errorf("intersect top batch: %w", err)
	}
	return out, nil
}

// TermsPage is one page of MatchedTermsBatch: doc ids in any order and the terms to test them against.
type TermsPage struct {
	IDs   []uint32
	Terms [][]byte
}

// MatchedTermsBatch (additive): for MANY pages - the ranked pages IntersectTopBatch returns, each with its own terms - which of
// its terms each id of a page lies under.  Result p holds len(IDs) rows of ceil(len(Terms) / 64) words: bit j&63 of word
// i*words + j>>6 says IDs[i] lies under Terms[j]; an id given twice in a page has its bits in its first row and zeros after.  One
// group per term, one one-list range per segment that holds it; a term found in no segment keeps its bit and never sets it; a
// page none of whose terms is in a segment keeps its place without a group and its rows are 0.  One upload of all ids, ONE
// Ctx.ExplainBatch call and one download - what the C++ host mirror's InvertedIndex::MatchedTermsBatch does
// (host/host_index.cpp).  Like Read, no tombstone filter.
func MatchedTermsBatch(c *Ctx, ix ResidentIndex, pages []TermsPage) ([][]uint64, error) {
	if len(pages) == 0 {
		return nil, nil
	}
	defer ix.Release()
	out := make([][]uint64, len(pages))
	queryFirst, groupFirst, idsOff := []uint64{0}, []uint64{0}, []uint64{0}
	var segs []*Segment
	var first, end []uint64
	var ids []uint32
	nOut := uint64(0)
	for p, P := range pages {
		out[p] = make([]uint64, uint64(len(P.IDs))*uint64((len(P.Terms)+63)/64))
		gMark, rMark := len(groupFirst), len(segs)
		found := false
		for _, t := range P.Terms {
			s, l, _ := ix.TermLists(t)
			found = found || len(s) > 0
			segs = append(segs, s...)
			for _, j := range l {
				first = append(first, j)
				end = append(end, j+1)
			}
			groupFirst = append(groupFirst, uint64(len(segs)))
		}
		if found {
			nOut += uint64(len(out[p]))
		} else { // the page keeps its place, without a group
			groupFirst = groupFirst[:gMark]
			segs, first, end = segs[:rMark], first[:rMark], end[:rMark]
		}
		queryFirst = append(queryFirst, uint64(len(groupFirst)-1))
		ids = append(ids, P.IDs...)
		idsOff = append(idsOff, uint64(len(ids)))
	}
	if nOut == 0 {
		return out, nil
	}
	masks, maskOff, err := c.ExplainBatchHost(queryFirst, groupFirst, segs, first, end, ids, idsOff)
	if err != nil {
		return nil, fmt.Errorf("matched terms batch: %w", err)
	}
	for p := range pages {
		copy(out[p], masks[maskOff[p]:maskOff[p+1]])
	}
	return out, nil
}

// IntersectExcept (additive, beside the additive Intersect): the ids under every term of terms and under none of except -
// "error AND db NOT healthcheck".  One group per term, one one-list range per segment that holds it, the excluded terms' groups
// flagged, and ONE Ctx.AndNotRanges call with one download - what the C++ host mirror's InvertedIndex::IntersectExcept does
// (host/host_index.cpp).  An excluded term found in no segment is dropped; a required one gives the empty result.  Like Read,
// no tombstone filter.
func IntersectExcept(c *Ctx, ix ResidentIndex, terms, except [][]byte) ([]uint32, error) {
	if len(terms) == 0 {
		return nil, nil
	}
	defer ix.Release()
	const firstCap = uint64(1) << 22
	groupFirst := []uint64{0}
	var groupNot []uint8
	var segs []*Segment
	var first, end []uint64
	bound := ^uint64(0)
	add := func(t []byte, not uint8) uint64 {
		s, l, post := ix.TermLists(t)
		if len(s) == 0 {
			return 0
		}
		segs = append(segs, s...)
		for _, j := range l {
			first = append(first, j)
			end = append(end, j+1)
		}
		groupFirst = append(groupFirst, uint64(len(segs)))
		groupNot = append(groupNot, not)
		if post == 0 {
			post = 1
		}
		return post
	}
	for _, t := range terms {
		post := add(t, 0)
		if post == 0 {
			return nil, nil // a required term in no segment: nothing is under every term
		}
		if post < bound {
			bound = post
		}
	}
	for _, t := range except {
		add(t, 1) // (in no segment: it removes nothing)
	}
	if bound > firstCap {
		bound = firstCap
	}
	ids, err := c.AndNotRangesHost(groupFirst, groupNot, segs, first, end, bound)
	if err != nil {
		return nil, fmt.Errorf("intersect except: %w", err)
	}
	return ids, nil
}
