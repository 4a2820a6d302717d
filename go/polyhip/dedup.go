// cgo binding of duplicate marking and coordinate order of libpolyhip.so (include/polyhip.h, "duplicate marking and
// coordinate order of the mapper's output").
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

// DedupParams is polyhip_dedup_params.  Paired: the entries are mates in the order 2i, 2i+1.  Weights come from the
// caller (Weight of MarkDuplicates, nil = all 0) unless quality strings are handed in; then a base adds its quality Q to the
// weight when Q >= MinWeightQual (0..93; Picard uses 15), and QualOffset is the Phred offset of the bytes (33 for FASTQ).
type DedupParams struct {
	Paired                    bool
	MinWeightQual, QualOffset uint32
}

// DedupInfo is polyhip_dedup_info: what the calling OS thread's last MarkDuplicates did.
type DedupInfo struct {
	Entries, Candidates, Bad, Pairs, Fragments, DupPairs, DupFragments, PairSets, EndSets uint64
}

// Duplicates: one value per entry.  Dup is 1 for a duplicate, Rep the entry it is a copy of (itself when it is none), Weight
// what it was ranked by, Errs as the header numbers them (2, 6, 7).
type Duplicates struct {
	Dup    []uint8
	Rep    []uint32
	Weight []uint32
	Errs   []uint32
}

// MarkDuplicates marks the entries of a MapResult whose unclipped 5' ends coincide (as pairs with p.Paired).  readLen: the
// length of every read, one per entry.  rid: the contig of every entry (of the refs calls), or nil.  weight: one per entry,
// or nil; quals / qualOff: the quality strings as FastqPackQual packs them, one per entry in the result's order, or nil --
// with them the weights are computed on the device and weight must be nil.  Nothing is removed: clear Flags bit 0 of the
// entries with Dup = 1 before a Pileup, or set 0x400 in their SAM FLAG.
func MarkDuplicates(r *MapResult, readLen, rid, weight []uint32, quals []byte, qualOff []uint64, p DedupParams) (*Duplicates, error) {
	n := len(r.Flags)
	if len(r.RefStart) != n || len(r.RefEnd) != n || len(r.ReadStart) != n || len(r.ReadEnd) != n || len(readLen) != n ||
		(rid != nil && len(rid) != n) || (weight != nil && len(weight) != n) || (qualOff != nil && len(qualOff) != n+1) {
		return nil, fmt.Errorf("polyhip.MarkDuplicates: the arrays hold different numbers of entries")
	}
	if weight != nil && qualOff != nil {
		return nil, fmt.Errorf("polyhip.MarkDuplicates: weights or quality strings, not both")
	}
	var cp C.polyhip_dedup_params
	if p.Paired {
		cp.paired = 1
	}
	if qualOff != nil {
		cp.weight_mode = 1
	}
	cp.min_weight_qual, cp.qual_offset = C.uint32_t(p.MinWeightQual), C.uint32_t(p.QualOffset)
	pad32 := func(s []uint32) []uint32 { // an empty batch still needs &s[0]
		if len(s) == 0 {
			return []uint32{0}
		}
		return s
	}
	flags, refStart, refEnd := pad32(r.Flags), pad32(r.RefStart), pad32(r.RefEnd)
	readStart, readEnd, lens := pad32(r.ReadStart), pad32(r.ReadEnd), pad32(readLen)
	var ridp, wp *C.uint32_t // nil: one contig, no weights
	if len(rid) > 0 {
		ridp = (*C.uint32_t)(unsafe.Pointer(&rid[0]))
	}
	if len(weight) > 0 {
		wp = (*C.uint32_t)(unsafe.Pointer(&weight[0]))
	}
	var qp *C.uint8_t // nil: no quality strings, or only empty ones
	var qo *C.uint64_t
	if qualOff != nil {
		qo = (*C.uint64_t)(unsafe.Pointer(&qualOff[0]))
		if len(quals) > 0 {
			qp = (*C.uint8_t)(unsafe.Pointer(&quals[0]))
		}
	}
	out := &Duplicates{Dup: make([]uint8, n+1), Rep: make([]uint32, n+1), Weight: make([]uint32, n+1), Errs: make([]uint32, n+1)}
	err := call(func() C.int {
		return C.polyhip_mark_duplicates((*C.polyhip_dedup_params)(unsafe.Pointer(&cp)), C.uint64_t(n),
			(*C.uint32_t)(unsafe.Pointer(&flags[0])), (*C.uint32_t)(unsafe.Pointer(ridp)),
			(*C.uint32_t)(unsafe.Pointer(&refStart[0])), (*C.uint32_t)(unsafe.Pointer(&refEnd[0])),
			(*C.uint32_t)(unsafe.Pointer(&readStart[0])), (*C.uint32_t)(unsafe.Pointer(&readEnd[0])),
			(*C.uint32_t)(unsafe.Pointer(&lens[0])), (*C.uint32_t)(unsafe.Pointer(wp)),
			(*C.uint8_t)(unsafe.Pointer(qp)), (*C.uint64_t)(unsafe.Pointer(qo)),
			(*C.uint32_t)(unsafe.Pointer(&out.Weight[0])), (*C.uint8_t)(unsafe.Pointer(&out.Dup[0])),
			(*C.uint32_t)(unsafe.Pointer(&out.Rep[0])), (*C.uint32_t)(unsafe.Pointer(&out.Errs[0])))
	})
	if err != nil {
		return nil, err
	}
	out.Dup, out.Rep, out.Weight, out.Errs = out.Dup[:n], out.Rep[:n], out.Weight[:n], out.Errs[:n]
	return out, nil
}

// LastDedupInfo must run on the OS thread that made the call (runtime.LockOSThread around both).
func LastDedupInfo() (DedupInfo, error) {
	var ci C.polyhip_dedup_info
	err := call(func() C.int { return C.polyhip_dedup_last_info((*C.polyhip_dedup_info)(unsafe.Pointer(&ci))) })
	return DedupInfo{Entries: uint64(ci.entries), Candidates: uint64(ci.candidates), Bad: uint64(ci.bad), Pairs: uint64(ci.pairs),
		Fragments: uint64(ci.fragments), DupPairs: uint64(ci.dup_pairs), DupFragments: uint64(ci.dup_fragments),
		PairSets: uint64(ci.pair_sets), EndSets: uint64(ci.end_sets)}, err
}

// CoordOrder returns the stable permutation that puts the entries into SAM's coordinate order: live entries (samFlag, of
// AlnRecords, lacks 0x4) by (rid, refStart), with paired an entry that is not live beside its live mate, every other entry
// last; ties in index order.  rid may be nil.
func CoordOrder(samFlag, rid, refStart []uint32, paired bool) ([]uint32, error) {
	n := len(samFlag)
	if len(refStart) != n || (rid != nil && len(rid) != n) {
		return nil, fmt.Errorf("polyhip.CoordOrder: the arrays hold different numbers of entries")
	}
	if n == 0 {
		return []uint32{}, nil
	}
	var ridp *C.uint32_t // nil: one contig
	if len(rid) > 0 {
		ridp = (*C.uint32_t)(unsafe.Pointer(&rid[0]))
	}
	mates := 0
	if paired {
		mates = 1
	}
	order := make([]uint32, n)
	err := call(func() C.int {
		return C.polyhip_coord_order(C.uint64_t(n), C.uint32_t(mates), (*C.uint32_t)(unsafe.Pointer(&samFlag[0])),
			(*C.uint32_t)(unsafe.Pointer(ridp)), (*C.uint32_t)(unsafe.Pointer(&refStart[0])),
			(*C.uint32_t)(unsafe.Pointer(&order[0])))
	})
	if err != nil {
		return nil, err
	}
	return order, nil
}
