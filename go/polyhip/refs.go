// cgo binding of the reference set and the read mapper on it of libpolyhip.so (include/polyhip.h, "a reference of several
// contigs, and read mapping onto it").
// UNCOMPILED in the authoring image (no Go toolchain).
package polyhip

/*
#include "polyhip.h"
*/
import "C"

import (
	"fmt"
	"runtime"
	"unsafe"
)

// RefSet wraps polyhip_refs: k contigs, one FM-index over their concatenation C and the contigs' starts in C, resident on
// the HIP device that was current when it was built.  Close releases it, the index included.
type RefSet struct{ h *C.polyhip_refs }

// NewRefSet builds the set of the packed batch: contig c is seqs[offs[c]:offs[c+1]].
func NewRefSet(seqs []byte, offs []uint64) (*RefSet, error) {
	if len(offs) < 1 {
		return nil, fmt.Errorf("polyhip.NewRefSet: offs must hold at least one entry")
	}
	r := &RefSet{}
	buf := seqs
	if len(buf) == 0 {
		buf = []byte{0} // a valid pointer; an empty set is refused with the library's message
	}
	err := call(func() C.int {
		return C.polyhip_refs_create((*C.uint8_t)(unsafe.Pointer(&buf[0])), (*C.uint64_t)(unsafe.Pointer(&offs[0])),
			C.uint64_t(len(offs)-1), &r.h)
	})
	if err != nil {
		return nil, err
	}
	runtime.SetFinalizer(r, func(r *RefSet) { r.Close() })
	return r, nil
}

func (r *RefSet) Close() {
	if r.h != nil {
		C.polyhip_refs_destroy(r.h)
		r.h = nil
	}
}

// Count is the number of contigs.
func (r *RefSet) Count() int { return int(C.polyhip_refs_count(r.h)) }

// Starts holds where every contig begins in C, and C's length last (Count() + 1 entries).
func (r *RefSet) Starts() ([]uint64, error) {
	out := make([]uint64, r.Count()+1)
	err := call(func() C.int { return C.polyhip_refs_starts(r.h, (*C.uint64_t)(unsafe.Pointer(&out[0]))) })
	return out, err
}

// Index is the index of C.  It is borrowed: the set owns it, it lives as long as the set, and it must not be closed.
func (r *RefSet) Index() *BWT { return &BWT{h: (*C.polyhip_bwt)(unsafe.Pointer(C.polyhip_refs_index(r.h)))} }

// Resolve turns positions in C (what Index().LocateBatch returns) with length[i] bytes each (nil: one byte each) into the
// contig and the position in it; errs[i] = 1: not a position of C, 2: the span runs past its contig's end.
func (r *RefSet) Resolve(pos, length []uint32) (rid, local, errs []uint32, err error) {
	n := len(pos)
	if n == 0 {
		return nil, nil, nil, nil
	}
	if length != nil && len(length) != n {
		return nil, nil, nil, fmt.Errorf("polyhip.Resolve: pos and length differ in length")
	}
	var lp *C.uint32_t
	if length != nil {
		lp = (*C.uint32_t)(unsafe.Pointer(&length[0]))
	}
	rid, local, errs = make([]uint32, n), make([]uint32, n), make([]uint32, n)
	err = call(func() C.int {
		return C.polyhip_refs_resolve(r.h, (*C.uint32_t)(unsafe.Pointer(&pos[0])), lp, C.uint64_t(n),
			(*C.uint32_t)(unsafe.Pointer(&rid[0])), (*C.uint32_t)(unsafe.Pointer(&local[0])), (*C.uint32_t)(unsafe.Pointer(&errs[0])))
	})
	return rid, local, errs, err
}

// MapRefsInfo is polyhip_map_refs_info: the contigs of the calling OS thread's last refs call and the seed occurrences it
// dropped because they straddle a boundary.  The other counters are LastMapAffineInfo's / LastMapPairsInfo's.
type MapRefsInfo struct{ Contigs, Straddling uint64 }

// MapRefsResult is MapResult with every entry's contig: RefStart and RefEnd are positions in contig Rid[i].
type MapRefsResult struct {
	MapResult
	Rid []uint32
}

// MapPairsRefsResult is MapPairsResult with every mate's contig.
type MapPairsRefsResult struct {
	MapPairsResult
	Rid []uint32
}

func cMapParams(p MapParams) C.polyhip_map_params {
	var cp C.polyhip_map_params
	cp.seed_len, cp.seed_stride, cp.max_occ = C.uint32_t(p.SeedLen), C.uint32_t(p.SeedStride), C.uint32_t(p.MaxOcc)
	cp.band, cp.max_cand, cp.min_score = C.uint32_t(p.Band), C.uint32_t(p.MaxCand), C.int64_t(p.MinScore)
	if p.BothStrands {
		cp.both_strands = 1
	}
	return cp
}

// MapReadsRefs is MapReadsAffine on a set: no seed, cluster, window or alignment crosses a contig boundary (gapOpen ==
// gapExtend: linear gaps).  capacity and workLimit as there.
func MapReadsRefs(rs *RefSet, sc *Scoring, p MapParams, gapOpen, gapExtend int64, reads []byte, offs []uint64, maxLen, capacity int, workLimit uint64) (*MapRefsResult, error) {
	n := len(offs) - 1
	if n < 0 {
		return nil, fmt.Errorf("polyhip.MapReadsRefs: offs must hold at least one entry")
	}
	if len(reads) == 0 {
		reads = []byte{0}
	}
	var hr *C.polyhip_refs = rs.h
	var hs *C.polyhip_scoring = sc.h
	cp := cMapParams(p)
	m := n
	if m == 0 {
		m = 1 // an empty batch still needs &s[0]
	}
	r := &MapRefsResult{MapResult: MapResult{Score: make([]int64, m), Second: make([]int64, m), Flags: make([]uint32, m),
		Votes: make([]uint32, m), RefStart: make([]uint32, m), RefEnd: make([]uint32, m), ReadStart: make([]uint32, m),
		ReadEnd: make([]uint32, m), Errs: make([]uint32, m), AlnOff: make([]uint64, n+1)}, Rid: make([]uint32, m)}
	var err error
	for attempt := 0; attempt < 2; attempt++ {
		r.AlignA, r.AlignB = make([]byte, capacity+1), make([]byte, capacity+1)
		err = call(func() C.int {
			return C.polyhip_map_reads_refs(hr, hs, (*C.polyhip_map_params)(unsafe.Pointer(&cp)), C.int64_t(gapOpen), C.int64_t(gapExtend),
				(*C.uint8_t)(unsafe.Pointer(&reads[0])), (*C.uint64_t)(unsafe.Pointer(&offs[0])), C.uint64_t(n), C.uint32_t(maxLen),
				C.uint64_t(workLimit),
				(*C.int64_t)(unsafe.Pointer(&r.Score[0])), (*C.int64_t)(unsafe.Pointer(&r.Second[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.Flags[0])), (*C.uint32_t)(unsafe.Pointer(&r.Votes[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.Rid[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.RefStart[0])), (*C.uint32_t)(unsafe.Pointer(&r.RefEnd[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.ReadStart[0])), (*C.uint32_t)(unsafe.Pointer(&r.ReadEnd[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.Errs[0])),
				(*C.uint8_t)(unsafe.Pointer(&r.AlignA[0])), (*C.uint8_t)(unsafe.Pointer(&r.AlignB[0])),
				(*C.uint64_t)(unsafe.Pointer(&r.AlnOff[0])), C.uint64_t(capacity))
		})
		if err == nil || r.AlnOff[n] <= uint64(capacity) {
			break
		}
		capacity = int(r.AlnOff[n])
	}
	if err != nil {
		return nil, err
	}
	for _, s := range []*[]uint32{&r.Flags, &r.Votes, &r.Rid, &r.RefStart, &r.RefEnd, &r.ReadStart, &r.ReadEnd, &r.Errs} {
		*s = (*s)[:n]
	}
	r.Score, r.Second = r.Score[:n], r.Second[:n]
	r.AlignA, r.AlignB = r.AlignA[:r.AlnOff[n]], r.AlignB[:r.AlnOff[n]]
	return r, nil
}

// MapPairsRefs is MapPairs on a set: a proper pair lies on one contig, a rescue window inside the anchor's contig, and a
// rescued mate takes its anchor's contig.
func MapPairsRefs(rs *RefSet, sc *Scoring, p MapParams, pp PairParams, gapOpen, gapExtend int64, reads1 []byte, offs1 []uint64, reads2 []byte, offs2 []uint64, maxLen, capacity int, workLimit uint64) (*MapPairsRefsResult, error) {
	n := len(offs1) - 1
	if n < 0 || len(offs2) != len(offs1) {
		return nil, fmt.Errorf("polyhip.MapPairsRefs: offs1 and offs2 must hold the same number of entries, at least one")
	}
	if len(reads1) == 0 {
		reads1 = []byte{0}
	}
	if len(reads2) == 0 {
		reads2 = []byte{0}
	}
	var hr *C.polyhip_refs = rs.h
	var hs *C.polyhip_scoring = sc.h
	cp := cMapParams(p)
	var cpp C.polyhip_map_pair_params
	cpp.min_insert, cpp.max_insert = C.uint32_t(pp.MinInsert), C.uint32_t(pp.MaxInsert)
	if pp.Rescue {
		cpp.rescue = 1
	}
	m := 2 * n
	if m == 0 {
		m = 1 // an empty batch still needs &s[0]
	}
	r := &MapPairsRefsResult{MapPairsResult: MapPairsResult{MapResult: MapResult{Score: make([]int64, m), Second: make([]int64, m),
		Flags: make([]uint32, m), Votes: make([]uint32, m), RefStart: make([]uint32, m), RefEnd: make([]uint32, m),
		ReadStart: make([]uint32, m), ReadEnd: make([]uint32, m), Errs: make([]uint32, m), AlnOff: make([]uint64, 2*n+1)},
		Tlen: make([]int64, m)}, Rid: make([]uint32, m)}
	var err error
	for attempt := 0; attempt < 2; attempt++ {
		r.AlignA, r.AlignB = make([]byte, capacity+1), make([]byte, capacity+1)
		err = call(func() C.int {
			return C.polyhip_map_pairs_refs(hr, hs, (*C.polyhip_map_params)(unsafe.Pointer(&cp)),
				(*C.polyhip_map_pair_params)(unsafe.Pointer(&cpp)), C.int64_t(gapOpen), C.int64_t(gapExtend),
				(*C.uint8_t)(unsafe.Pointer(&reads1[0])), (*C.uint64_t)(unsafe.Pointer(&offs1[0])),
				(*C.uint8_t)(unsafe.Pointer(&reads2[0])), (*C.uint64_t)(unsafe.Pointer(&offs2[0])), C.uint64_t(n), C.uint32_t(maxLen),
				C.uint64_t(workLimit),
				(*C.int64_t)(unsafe.Pointer(&r.Score[0])), (*C.int64_t)(unsafe.Pointer(&r.Second[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.Flags[0])), (*C.uint32_t)(unsafe.Pointer(&r.Votes[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.Rid[0])),
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
	for _, s := range []*[]uint32{&r.Flags, &r.Votes, &r.Rid, &r.RefStart, &r.RefEnd, &r.ReadStart, &r.ReadEnd, &r.Errs} {
		*s = (*s)[:2*n]
	}
	r.Score, r.Second, r.Tlen = r.Score[:2*n], r.Second[:2*n], r.Tlen[:n]
	r.AlignA, r.AlignB = r.AlignA[:r.AlnOff[2*n]], r.AlignB[:r.AlnOff[2*n]]
	return r, nil
}

// LastMapRefsInfo must run on the OS thread that made the call (runtime.LockOSThread around both).
func LastMapRefsInfo() (MapRefsInfo, error) {
	var ci C.polyhip_map_refs_info
	err := call(func() C.int { return C.polyhip_map_refs_last_info((*C.polyhip_map_refs_info)(unsafe.Pointer(&ci))) })
	return MapRefsInfo{Contigs: uint64(ci.contigs), Straddling: uint64(ci.straddling)}, err
}
