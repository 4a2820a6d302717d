// cgo binding of the variant calls of libpolyhip.so (include/polyhip.h, "variant calls from the mapped reads").
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

// VarMaxIndel is POLYHIP_VAR_MAX_INDEL: the longest insertion or deletion a call keeps.
const VarMaxIndel = 255

// VariantsParams is polyhip_variants_params: PileupQualParams plus whether indels are left-aligned, the share of the depth from
// which a call is 1/1 (0..1000) and the longest run kept (0 means VarMaxIndel).
type VariantsParams struct {
	PileupQualParams
	LeftAlign              bool
	HomPermille, MaxIndel uint32
}

// Variant is polyhip_variant.  Kind: 1 SNV (Alt is the base), 2 insertion of AlleleLen bytes behind Pos (they stand at
// Alleles[AlleleOff:AlleleOff+AlleleLen]), 3 deletion of the AlleleLen text bytes behind Pos.  Gt: 1 is 0/1, 2 is 1/1.
type Variant struct {
	AlleleOff                                                 uint64
	Pos, Depth, Count, CountFwd, RefCount, Qsum, AlleleLen uint32
	Kind, Ref, Alt, Gt                                        uint8
}

// VariantsInfo is polyhip_variants_info: what the calling OS thread's last CallVariants did.
type VariantsInfo struct {
	PileupQualInfo
	Events, LongEvents, OpenEvents, ShiftedEvents, Alleles, AlleleBytes uint64
}

// VariantsResult: Variants in ascending position (within one: SNVs, insertions by length and bytes, deletions by length),
// Alleles the inserted bytes in upper case, Errs one value per entry.
type VariantsResult struct {
	Variants []Variant
	Alleles  []byte
	Errs     []uint32
}

// CallVariants groups what the entries of a MapResult say into alleles and returns the ones that pass the thresholds.  mapq:
// the Mapq of AlnRecords, or nil when p.MinMapq is 0.  quals / qualOff: as in PileupQual, or nil for a call without qualities
// (p.MinBaseQual must then be 0).  variantCap, alleleCap: entries and bytes of the two buffers; a call that outgrows either
// runs once more with the sizes the library reports.
func CallVariants(r *MapResult, mapq []uint8, quals []byte, qualOff []uint64, ref []byte, p VariantsParams, variantCap, alleleCap int) (*VariantsResult, error) {
	n := len(r.Flags)
	if len(r.AlnOff) != n+1 || len(r.RefStart) != n || len(r.RefEnd) != n || (mapq != nil && len(mapq) != n) ||
		(quals != nil && (len(qualOff) != n+1 || len(r.ReadStart) != n)) {
		return nil, fmt.Errorf("polyhip.CallVariants: the arrays hold different numbers of entries")
	}
	if p.RegionLo > p.RegionHi || p.RegionHi > uint64(len(ref)) {
		return nil, fmt.Errorf("polyhip.CallVariants: the region [%d, %d) is not inside the text of %d bytes", p.RegionLo, p.RegionHi, len(ref))
	}
	var cp C.polyhip_variants_params
	cp.base.base.region_lo, cp.base.base.region_hi = C.uint64_t(p.RegionLo), C.uint64_t(p.RegionHi)
	cp.base.base.min_mapq, cp.base.base.min_depth = C.uint32_t(p.MinMapq), C.uint32_t(p.MinDepth)
	cp.base.base.min_alt_count, cp.base.base.min_alt_permille = C.uint32_t(p.MinAltCount), C.uint32_t(p.MinAltPermille)
	cp.base.min_base_qual, cp.base.qual_offset = C.uint32_t(p.MinBaseQual), C.uint32_t(p.QualOffset)
	cp.hom_permille, cp.max_indel = C.uint32_t(p.HomPermille), C.uint32_t(p.MaxIndel)
	if p.LeftAlign {
		cp.left_align = 1
	}
	pad32 := func(s []uint32) []uint32 { // an empty batch still needs &s[0]
		if len(s) == 0 {
			return []uint32{0}
		}
		return s
	}
	padB := func(s []byte) []byte {
		if len(s) == 0 {
			return []byte{0}
		}
		return s
	}
	flags, refStart, refEnd := pad32(r.Flags), pad32(r.RefStart), pad32(r.RefEnd)
	alnA, alnB, text := padB(r.AlignA), padB(r.AlignB), padB(ref)
	var mq, qp *C.uint8_t // nil: no mapq; nil: no qualities
	var rsp *C.uint32_t
	var qop *C.uint64_t
	if len(mapq) > 0 {
		mq = (*C.uint8_t)(unsafe.Pointer(&mapq[0]))
	}
	if quals != nil && n > 0 {
		qual := padB(quals)
		qp, qop = (*C.uint8_t)(unsafe.Pointer(&qual[0])), (*C.uint64_t)(unsafe.Pointer(&qualOff[0]))
		rsp = (*C.uint32_t)(unsafe.Pointer(&r.ReadStart[0]))
	}
	out := &VariantsResult{Errs: make([]uint32, n+1)}
	var nvar, nbytes C.uint64_t
	var err error
	for attempt := 0; attempt < 2; attempt++ {
		out.Variants, out.Alleles = make([]Variant, variantCap+1), make([]byte, alleleCap+1)
		err = call(func() C.int {
			return C.polyhip_call_variants((*C.polyhip_variants_params)(unsafe.Pointer(&cp)), C.uint64_t(n),
				(*C.uint32_t)(unsafe.Pointer(&flags[0])), (*C.uint8_t)(unsafe.Pointer(mq)),
				(*C.uint32_t)(unsafe.Pointer(&refStart[0])), (*C.uint32_t)(unsafe.Pointer(&refEnd[0])),
				(*C.uint32_t)(unsafe.Pointer(rsp)),
				(*C.uint8_t)(unsafe.Pointer(&alnA[0])), (*C.uint8_t)(unsafe.Pointer(&alnB[0])),
				(*C.uint64_t)(unsafe.Pointer(&r.AlnOff[0])), (*C.uint8_t)(unsafe.Pointer(qp)),
				(*C.uint64_t)(unsafe.Pointer(qop)), (*C.uint8_t)(unsafe.Pointer(&text[0])), C.uint64_t(len(ref)),
				(*C.uint64_t)(unsafe.Pointer(&nvar)), (*C.polyhip_variant)(unsafe.Pointer(&out.Variants[0])), C.uint64_t(variantCap),
				(*C.uint64_t)(unsafe.Pointer(&nbytes)), (*C.uint8_t)(unsafe.Pointer(&out.Alleles[0])), C.uint64_t(alleleCap),
				(*C.uint32_t)(unsafe.Pointer(&out.Errs[0])))
		})
		if err == nil || (uint64(nvar) <= uint64(variantCap) && uint64(nbytes) <= uint64(alleleCap)) {
			break
		}
		variantCap, alleleCap = int(nvar), int(nbytes)
	}
	if err != nil {
		return nil, err
	}
	out.Variants, out.Alleles, out.Errs = out.Variants[:nvar], out.Alleles[:nbytes], out.Errs[:n]
	return out, nil
}

// LastVariantsInfo must run on the OS thread that made the call (runtime.LockOSThread around both).
func LastVariantsInfo() (VariantsInfo, error) {
	var ci C.polyhip_variants_info
	err := call(func() C.int { return C.polyhip_call_variants_last_info((*C.polyhip_variants_info)(unsafe.Pointer(&ci))) })
	return VariantsInfo{PileupQualInfo: PileupQualInfo{PileupInfo: PileupInfo{Entries: uint64(ci.entries), Used: uint64(ci.used),
		SkippedMapq: uint64(ci.skipped_mapq), Bad: uint64(ci.bad), Columns: uint64(ci.columns), EdgeEvents: uint64(ci.edge_events),
		Sites: uint64(ci.sites)}, FilteredBases: uint64(ci.filtered_bases)}, Events: uint64(ci.events), LongEvents: uint64(ci.long_events),
		OpenEvents: uint64(ci.open_events), ShiftedEvents: uint64(ci.shifted_events), Alleles: uint64(ci.alleles),
		AlleleBytes: uint64(ci.allele_bytes)}, err
}
