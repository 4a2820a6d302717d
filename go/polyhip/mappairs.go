// cgo binding of the paired-end read mapper of libpolyhip.so (include/polyhip.h, "read mapping of paired-end reads").
// UNCOMPILED in the authoring image (no Go toolchain).
package polyhip

/*
#include "polyhip.h"
*/
import "C"

import (
	"fmt"
	"unsafe"
)

// Flag bits of a mate beyond MapResult's two: its pair is proper; the mate was placed by a rescue.
const (
	FlagProper  = 4
	FlagRescued = 8
)

// PairParams is polyhip_map_pair_params: the inserts (outer distance of a forward-reverse pair) that make a pair proper,
// and whether a mate without a placement of its own is searched for in the window its partner implies.
type PairParams struct {
	MinInsert, MaxInsert int
	Rescue               bool
}

// MapPairsInfo is polyhip_map_pairs_info: what the calling OS thread's last MapPairs did.
type MapPairsInfo struct {
	Seeds, SeedsOverMaxOcc, Hits, Clusters, PairsAligned, ReadsMapped uint64
	ProperPairs, RescueAttempts, Rescued, PairsTraced                  uint64
	Chunks                                                             int
}

// MapPairsResult holds two entries per pair in MapResult (2i: mate 1 of pair i, 2i+1: mate 2) and one Tlen per pair: the
// insert of a proper pair, else 0.
type MapPairsResult struct {
	MapResult
	Tlen []int64
}

// MapPairs places mate i of (reads1, offs1) with mate i of (reads2, offs2) on the index's text, with affine gaps in the
// extension as MapReadsAffine has them.  capacity: bytes per string buffer; a batch whose strings outgrow it runs once more
// with the size the library reports in AlnOff[2n].  workLimit: the most device workspace in bytes (0: the default).
func MapPairs(b *BWT, sc *Scoring, p MapParams, pp PairParams, gapOpen, gapExtend int64, reads1 []byte, offs1 []uint64, reads2 []byte, offs2 []uint64, maxLen, capacity int, workLimit uint64) (*MapPairsResult, error) {
	n := len(offs1) - 1
	if n < 0 || len(offs2) != len(offs1) {
		return nil, fmt.Errorf("polyhip.MapPairs: offs1 and offs2 must hold the same number of entries, at least one")
	}
	if len(reads1) == 0 {
		reads1 = []byte{0}
	}
	if len(reads2) == 0 {
		reads2 = []byte{0}
	}
	var hb *C.polyhip_bwt = b.h
	var hs *C.polyhip_scoring = sc.h
	var cp C.polyhip_map_params
	cp.seed_len, cp.seed_stride, cp.max_occ = C.uint32_t(p.SeedLen), C.uint32_t(p.SeedStride), C.uint32_t(p.MaxOcc)
	cp.band, cp.max_cand, cp.min_score = C.uint32_t(p.Band), C.uint32_t(p.MaxCand), C.int64_t(p.MinScore)
	if p.BothStrands {
		cp.both_strands = 1
	}
	var cpp C.polyhip_map_pair_params
	cpp.min_insert, cpp.max_insert = C.uint32_t(pp.MinInsert), C.uint32_t(pp.MaxInsert)
	if pp.Rescue {
		cpp.rescue = 1
	}
	m := 2 * n
	if m == 0 {
		m = 1 // an empty batch still needs &s[0]
	}
	r := &MapPairsResult{MapResult: MapResult{Score: make([]int64, m), Second: make([]int64, m), Flags: make([]uint32, m),
		Votes: make([]uint32, m), RefStart: make([]uint32, m), RefEnd: make([]uint32, m), ReadStart: make([]uint32, m),
		ReadEnd: make([]uint32, m), Errs: make([]uint32, m), AlnOff: make([]uint64, 2*n+1)}, Tlen: make([]int64, m)}
	var err error
	for attempt := 0; attempt < 2; attempt++ {
		r.AlignA, r.AlignB = make([]byte, capacity+1), make([]byte, capacity+1)
		err = call(func() C.int {
			return C.polyhip_map_pairs(hb, hs, (*C.polyhip_map_params)(unsafe.Pointer(&cp)),
				(*C.polyhip_map_pair_params)(unsafe.Pointer(&cpp)), C.int64_t(gapOpen), C.int64_t(gapExtend),
				(*C.uint8_t)(unsafe.Pointer(&reads1[0])), (*C.uint64_t)(unsafe.Pointer(&offs1[0])),
				(*C.uint8_t)(unsafe.Pointer(&reads2[0])), (*C.uint64_t)(unsafe.Pointer(&offs2[0])), C.uint64_t(n), C.uint32_t(maxLen),
				C.uint64_t(workLimit),
				(*C.int64_t)(unsafe.Pointer(&r.Score[0])), (*C.int64_t)(unsafe.Pointer(&r.Second[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.Flags[0])), (*C.uint32_t)(unsafe.Pointer(&r.Votes[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.RefStart[0])), (*C.uint32_t)(unsafe.Pointer(&r.RefEnd[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.ReadStart[0])), (*C.uint32_t)(unsafe.Pointer(&r.ReadEnd[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.Errs[0])), (*C.int64_t)(unsafe.Pointer(&r.Tlen[0])),
				(*C.uint8_t)(unsafe.Pointer(&r.AlignA[0])), (*C.uint8_t)(unsafe.Pointer(&r.AlignB[0])),
				(*C.uint64_t)(unsafe.Pointer(&r.AlnOff[0])), C.uint64_t(capacity))
		})
		if err == nil || r.AlnOff[2*n] <= uint64(capacity) {
			break
		}
		capacity = int(r.AlnOff[2*n])
	}
	if err != nil {
		return nil, err
	}
	for _, s := range []*[]uint32{&r.Flags, &r.Votes, &r.RefStart, &r.RefEnd, &r.ReadStart, &r.ReadEnd, &r.Errs} {
		*s = (*s)[:2*n]
	}
	r.Score, r.Second, r.Tlen = r.Score[:2*n], r.Second[:2*n], r.Tlen[:n]
	r.AlignA, r.AlignB = r.AlignA[:r.AlnOff[2*n]], r.AlignB[:r.AlnOff[2*n]]
	return r, nil
}

// LastMapPairsInfo must run on the OS thread that made the call (runtime.LockOSThread around both).
func LastMapPairsInfo() (MapPairsInfo, error) {
	var ci C.polyhip_map_pairs_info
	err := call(func() C.int { return C.polyhip_map_pairs_last_info((*C.polyhip_map_pairs_info)(unsafe.Pointer(&ci))) })
	return MapPairsInfo{Seeds: uint64(ci.seeds), SeedsOverMaxOcc: uint64(ci.seeds_over_max_occ), Hits: uint64(ci.hits),
		Clusters: uint64(ci.clusters), PairsAligned: uint64(ci.pairs_aligned), ReadsMapped: uint64(ci.reads_mapped),
		ProperPairs: uint64(ci.proper_pairs), RescueAttempts: uint64(ci.rescue_attempts), Rescued: uint64(ci.rescued),
		PairsTraced: uint64(ci.pairs_traced), Chunks: int(ci.chunks)}, err
}
