// cgo binding of the read mapper of libpolyhip.so (include/polyhip.h, "read mapping").
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

// MapParams is polyhip_map_params.  DefaultMapParams are unmeasured starting values.
type MapParams struct {
	SeedLen, SeedStride, MaxOcc, Band, MaxCand int
	BothStrands                                bool
	MinScore                                   int64
}

var DefaultMapParams = MapParams{SeedLen: 20, SeedStride: 10, MaxOcc: 32, Band: 24, MaxCand: 4, BothStrands: true, MinScore: 1}

// MapInfo is polyhip_map_info: what the calling OS thread's last MapReads did.
type MapInfo struct {
	Seeds, SeedsOverMaxOcc, Hits, Clusters, PairsAligned, ReadsMapped uint64
	Chunks                                                             int
}

// MapResult holds one entry per read; read i's aligned strings are AlignA[AlnOff[i]:AlnOff[i+1]] and the same range of
// AlignB.  Flags: bit 0 mapped, bit 1 reverse strand.
type MapResult struct {
	Score, Second                                              []int64
	Flags, Votes, RefStart, RefEnd, ReadStart, ReadEnd, Errs []uint32
	AlignA, AlignB                                             []byte
	AlnOff                                                     []uint64
}

// MapReads places every read of the packed batch (reads, offs) on the index's text.  capacity: bytes per string buffer; a
// batch whose strings outgrow it runs once more with the size the library reports in AlnOff[n].
func MapReads(b *BWT, sc *Scoring, p MapParams, reads []byte, offs []uint64, maxLen, capacity int) (*MapResult, error) {
	n := len(offs) - 1
	if n < 0 {
		return nil, fmt.Errorf("polyhip.MapReads: offs holds no entry")
	}
	if len(reads) == 0 {
		reads = []byte{0}
	}
	var hb *C.polyhip_bwt = b.h
	var hs *C.polyhip_scoring = sc.h
	var cp C.polyhip_map_params
	cp.seed_len, cp.seed_stride, cp.max_occ = C.uint32_t(p.SeedLen), C.uint32_t(p.SeedStride), C.uint32_t(p.MaxOcc)
	cp.band, cp.max_cand, cp.min_score = C.uint32_t(p.Band), C.uint32_t(p.MaxCand), C.int64_t(p.MinScore)
	if p.BothStrands {
		cp.both_strands = 1
	}
	m := n
	if m == 0 {
		m = 1 // an empty batch still needs &s[0]
	}
	r := &MapResult{Score: make([]int64, m), Second: make([]int64, m), Flags: make([]uint32, m), Votes: make([]uint32, m),
		RefStart: make([]uint32, m), RefEnd: make([]uint32, m), ReadStart: make([]uint32, m), ReadEnd: make([]uint32, m),
		Errs: make([]uint32, m), AlnOff: make([]uint64, n+1)}
	var err error
	for attempt := 0; attempt < 2; attempt++ {
		r.AlignA, r.AlignB = make([]byte, capacity+1), make([]byte, capacity+1)
		err = call(func() C.int {
			return C.polyhip_map_reads(hb, hs, (*C.polyhip_map_params)(unsafe.Pointer(&cp)), (*C.uint8_t)(unsafe.Pointer(&reads[0])),
				(*C.uint64_t)(unsafe.Pointer(&offs[0])), C.uint64_t(n), C.uint32_t(maxLen),
				(*C.int64_t)(unsafe.Pointer(&r.Score[0])), (*C.int64_t)(unsafe.Pointer(&r.Second[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.Flags[0])), (*C.uint32_t)(unsafe.Pointer(&r.Votes[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.RefStart[0])), (*C.uint32_t)(unsafe.Pointer(&r.RefEnd[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.ReadStart[0])), (*C.uint32_t)(unsafe.Pointer(&r.ReadEnd[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.Errs[0])), (*C.uint8_t)(unsafe.Pointer(&r.AlignA[0])),
				(*C.uint8_t)(unsafe.Pointer(&r.AlignB[0])), (*C.uint64_t)(unsafe.Pointer(&r.AlnOff[0])), C.uint64_t(capacity))
		})
		if err == nil || r.AlnOff[n] <= uint64(capacity) {
			break
		}
		capacity = int(r.AlnOff[n])
	}
	if err != nil {
		return nil, err
	}
	for _, s := range []*[]uint32{&r.Flags, &r.Votes, &r.RefStart, &r.RefEnd, &r.ReadStart, &r.ReadEnd, &r.Errs} {
		*s = (*s)[:n]
	}
	r.Score, r.Second = r.Score[:n], r.Second[:n]
	r.AlignA, r.AlignB = r.AlignA[:r.AlnOff[n]], r.AlignB[:r.AlnOff[n]]
	return r, nil
}

// LastMapInfo must run on the OS thread that made the call (runtime.LockOSThread around both).
func LastMapInfo() (MapInfo, error) {
	var ci C.polyhip_map_info
	err := call(func() C.int { return C.polyhip_map_last_info((*C.polyhip_map_info)(unsafe.Pointer(&ci))) })
	return MapInfo{Seeds: uint64(ci.seeds), SeedsOverMaxOcc: uint64(ci.seeds_over_max_occ), Hits: uint64(ci.hits),
		Clusters: uint64(ci.clusters), PairsAligned: uint64(ci.pairs_aligned), ReadsMapped: uint64(ci.reads_mapped),
		Chunks: int(ci.chunks)}, err
}

// MapAffineInfo is polyhip_map_affine_info: what the calling OS thread's last MapReadsAffine did.
type MapAffineInfo struct {
	Seeds, SeedsOverMaxOcc, Hits, Clusters, PairsAligned, ReadsMapped uint64
	PairsTraced, TbCells                                               uint64
	Chunks, TbChunks                                                   int
}

// MapReadsAffine is MapReads with affine gaps in the extension: the first symbol of a gap costs gapOpen, each further one
// gapExtend (added values, gapOpen <= gapExtend <= -1; the scoring handle's own gap is ignored).  workLimit: the most
// device workspace in bytes (0: the default).
func MapReadsAffine(b *BWT, sc *Scoring, p MapParams, gapOpen, gapExtend int64, reads []byte, offs []uint64, maxLen, capacity int, workLimit uint64) (*MapResult, error) {
	n := len(offs) - 1
	if n < 0 {
		return nil, fmt.Errorf("polyhip.MapReadsAffine: offs holds no entry")
	}
	if len(reads) == 0 {
		reads = []byte{0}
	}
	var hb *C.polyhip_bwt = b.h
	var hs *C.polyhip_scoring = sc.h
	var cp C.polyhip_map_params
	cp.seed_len, cp.seed_stride, cp.max_occ = C.uint32_t(p.SeedLen), C.uint32_t(p.SeedStride), C.uint32_t(p.MaxOcc)
	cp.band, cp.max_cand, cp.min_score = C.uint32_t(p.Band), C.uint32_t(p.MaxCand), C.int64_t(p.MinScore)
	if p.BothStrands {
		cp.both_strands = 1
	}
	m := n
	if m == 0 {
		m = 1 // an empty batch still needs &s[0]
	}
	r := &MapResult{Score: make([]int64, m), Second: make([]int64, m), Flags: make([]uint32, m), Votes: make([]uint32, m),
		RefStart: make([]uint32, m), RefEnd: make([]uint32, m), ReadStart: make([]uint32, m), ReadEnd: make([]uint32, m),
		Errs: make([]uint32, m), AlnOff: make([]uint64, n+1)}
	var err error
	for attempt := 0; attempt < 2; attempt++ {
		r.AlignA, r.AlignB = make([]byte, capacity+1), make([]byte, capacity+1)
		err = call(func() C.int {
			return C.polyhip_map_reads_affine(hb, hs, (*C.polyhip_map_params)(unsafe.Pointer(&cp)), C.int64_t(gapOpen), C.int64_t(gapExtend),
				(*C.uint8_t)(unsafe.Pointer(&reads[0])), (*C.uint64_t)(unsafe.Pointer(&offs[0])), C.uint64_t(n), C.uint32_t(maxLen),
				C.uint64_t(workLimit),
				(*C.int64_t)(unsafe.Pointer(&r.Score[0])), (*C.int64_t)(unsafe.Pointer(&r.Second[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.Flags[0])), (*C.uint32_t)(unsafe.Pointer(&r.Votes[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.RefStart[0])), (*C.uint32_t)(unsafe.Pointer(&r.RefEnd[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.ReadStart[0])), (*C.uint32_t)(unsafe.Pointer(&r.ReadEnd[0])),
				(*C.uint32_t)(unsafe.Pointer(&r.Errs[0])), (*C.uint8_t)(unsafe.Pointer(&r.AlignA[0])),
				(*C.uint8_t)(unsafe.Pointer(&r.AlignB[0])), (*C.uint64_t)(unsafe.Pointer(&r.AlnOff[0])), C.uint64_t(capacity))
		})
		if err == nil || r.AlnOff[n] <= uint64(capacity) {
			break
		}
		capacity = int(r.AlnOff[n])
	}
	if err != nil {
		return nil, err
	}
	for _, s := range []*[]uint32{&r.Flags, &r.Votes, &r.RefStart, &r.RefEnd, &r.ReadStart, &r.ReadEnd, &r.Errs} {
		*s = (*s)[:n]
	}
	r.Score, r.Second = r.Score[:n], r.Second[:n]
	r.AlignA, r.AlignB = r.AlignA[:r.AlnOff[n]], r.AlignB[:r.AlnOff[n]]
	return r, nil
}

// LastMapAffineInfo must run on the OS thread that made the call (runtime.LockOSThread around both).
func LastMapAffineInfo() (MapAffineInfo, error) {
	var ci C.polyhip_map_affine_info
	err := call(func() C.int { return C.polyhip_map_affine_last_info((*C.polyhip_map_affine_info)(unsafe.Pointer(&ci))) })
	return MapAffineInfo{Seeds: uint64(ci.seeds), SeedsOverMaxOcc: uint64(ci.seeds_over_max_occ), Hits: uint64(ci.hits),
		Clusters: uint64(ci.clusters), PairsAligned: uint64(ci.pairs_aligned), ReadsMapped: uint64(ci.reads_mapped),
		PairsTraced: uint64(ci.pairs_traced), TbCells: uint64(ci.tb_cells), Chunks: int(ci.chunks), TbChunks: int(ci.tb_chunks)}, err
}
