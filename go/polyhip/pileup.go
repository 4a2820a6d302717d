// cgo binding of the pileup of libpolyhip.so (include/polyhip.h, "pileup of the mapper's output").
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

// PileupChannels is POLYHIP_PILEUP_CHANNELS: Counts holds that many planes of one uint32 per position of the region.
const PileupChannels = 16

// PileupParams is polyhip_pileup_params: the region [RegionLo, RegionHi) of the text and the thresholds.
type PileupParams struct {
	RegionLo, RegionHi                              uint64
	MinMapq, MinDepth, MinAltCount, MinAltPermille uint32
}

// PileupSite is polyhip_pileup_site.  Kind: 1 SNV (Alt is the base), 2 insertion event, 3 deletion event anchored at Pos.
type PileupSite struct {
	Pos, Depth, Count, CountFwd uint32
	Kind, Ref, Alt, Pad         uint8
}

// PileupInfo is polyhip_pileup_info: what the calling OS thread's last Pileup did.
type PileupInfo struct {
	Entries, Used, SkippedMapq, Bad, Columns, EdgeEvents, Sites uint64
}

// PileupResult: Counts[ch*L+(p-RegionLo)] with ch = 8*strand + k (k = 0..3 A C G T, 4 other, 5 deleted base, 6 insertion
// events, 7 deletion events); Consensus one byte per position; Sites in ascending position; Errs one value per entry.
type PileupResult struct {
	Counts    []uint32
	Consensus []byte
	Sites     []PileupSite
	Errs      []uint32
}

// Pileup counts what the entries of a MapResult (of MapReads, MapReadsAffine or MapPairs) say about each position of the
// text ref they were mapped to.  mapq: the Mapq of AlnRecords on the same result, or nil when p.MinMapq is 0.  siteCap:
// entries of the site buffer; a call that outgrows it runs once more with the size the library reports.
func Pileup(r *MapResult, mapq []uint8, ref []byte, p PileupParams, siteCap int) (*PileupResult, error) {
	n := len(r.Flags)
	if len(r.AlnOff) != n+1 || len(r.RefStart) != n || len(r.RefEnd) != n || (mapq != nil && len(mapq) != n) {
		return nil, fmt.Errorf("polyhip.Pileup: the arrays hold different numbers of entries")
	}
	if p.RegionLo > p.RegionHi || p.RegionHi > uint64(len(ref)) {
		return nil, fmt.Errorf("polyhip.Pileup: the region [%d, %d) is not inside the text of %d bytes", p.RegionLo, p.RegionHi, len(ref))
	}
	var cp C.polyhip_pileup_params
	cp.region_lo, cp.region_hi = C.uint64_t(p.RegionLo), C.uint64_t(p.RegionHi)
	cp.min_mapq, cp.min_depth = C.uint32_t(p.MinMapq), C.uint32_t(p.MinDepth)
	cp.min_alt_count, cp.min_alt_permille = C.uint32_t(p.MinAltCount), C.uint32_t(p.MinAltPermille)
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
	var mq *C.uint8_t // nil: no mapq, MinMapq must be 0
	if len(mapq) > 0 {
		mq = (*C.uint8_t)(unsafe.Pointer(&mapq[0]))
	}
	L := int(p.RegionHi - p.RegionLo)
	out := &PileupResult{Counts: make([]uint32, PileupChannels*L+1), Consensus: make([]byte, L+1), Errs: make([]uint32, n+1)}
	var nsites C.uint64_t
	var err error
	for attempt := 0; attempt < 2; attempt++ {
		out.Sites = make([]PileupSite, siteCap+1)
		err = call(func() C.int {
			return C.polyhip_pileup((*C.polyhip_pileup_params)(unsafe.Pointer(&cp)), C.uint64_t(n),
				(*C.uint32_t)(unsafe.Pointer(&flags[0])), (*C.uint8_t)(unsafe.Pointer(mq)),
				(*C.uint32_t)(unsafe.Pointer(&refStart[0])), (*C.uint32_t)(unsafe.Pointer(&refEnd[0])),
				(*C.uint8_t)(unsafe.Pointer(&alnA[0])), (*C.uint8_t)(unsafe.Pointer(&alnB[0])),
				(*C.uint64_t)(unsafe.Pointer(&r.AlnOff[0])), (*C.uint8_t)(unsafe.Pointer(&text[0])), C.uint64_t(len(ref)),
				(*C.uint32_t)(unsafe.Pointer(&out.Counts[0])), (*C.uint8_t)(unsafe.Pointer(&out.Consensus[0])),
				(*C.uint64_t)(unsafe.Pointer(&nsites)), (*C.polyhip_pileup_site)(unsafe.Pointer(&out.Sites[0])),
				C.uint64_t(siteCap), (*C.uint32_t)(unsafe.Pointer(&out.Errs[0])))
		})
		if err == nil || uint64(nsites) <= uint64(siteCap) {
			break
		}
		siteCap = int(nsites)
	}
	if err != nil {
		return nil, err
	}
	out.Counts, out.Consensus, out.Errs = out.Counts[:PileupChannels*L], out.Consensus[:L], out.Errs[:n]
	out.Sites = out.Sites[:nsites]
	return out, nil
}

// LastPileupInfo must run on the OS thread that made the call (runtime.LockOSThread around both).
func LastPileupInfo() (PileupInfo, error) {
	var ci C.polyhip_pileup_info
	err := call(func() C.int { return C.polyhip_pileup_last_info((*C.polyhip_pileup_info)(unsafe.Pointer(&ci))) })
	return PileupInfo{Entries: uint64(ci.entries), Used: uint64(ci.used), SkippedMapq: uint64(ci.skipped_mapq), Bad: uint64(ci.bad),
		Columns: uint64(ci.columns), EdgeEvents: uint64(ci.edge_events), Sites: uint64(ci.sites)}, err
}

// PileupQualParams is polyhip_pileup_qual_params: PileupParams plus the minimum base quality (0..93) and the Phred offset of
// the quality bytes (33 for FASTQ).
type PileupQualParams struct {
	PileupParams
	MinBaseQual, QualOffset uint32
}

// PileupQualInfo is polyhip_pileup_qual_info: PileupInfo plus the base columns of used entries below MinBaseQual.
type PileupQualInfo struct {
	PileupInfo
	FilteredBases uint64
}

// PileupQualResult: PileupResult of the bases that reached MinBaseQual, plus Qsum[(4*strand+k)*L+(p-RegionLo)], k = 0..3: the
// sum of the qualities of the counted bases.  Deleted bases and events are not filtered.
type PileupQualResult struct {
	PileupResult
	Qsum []uint32
}

// PileupQual is Pileup with the reads' base qualities: quals[qualOff[i]:qualOff[i+1]] is entry i's quality string as
// sequenced (FastqPackQual's Quals and QualOffsets when QualMismatch is 0; for MapPairs the mates' strings interleaved).
func PileupQual(r *MapResult, mapq []uint8, quals []byte, qualOff []uint64, ref []byte, p PileupQualParams, siteCap int) (*PileupQualResult, error) {
	n := len(r.Flags)
	if len(r.AlnOff) != n+1 || len(qualOff) != n+1 || len(r.RefStart) != n || len(r.RefEnd) != n || len(r.ReadStart) != n ||
		(mapq != nil && len(mapq) != n) {
		return nil, fmt.Errorf("polyhip.PileupQual: the arrays hold different numbers of entries")
	}
	if p.RegionLo > p.RegionHi || p.RegionHi > uint64(len(ref)) {
		return nil, fmt.Errorf("polyhip.PileupQual: the region [%d, %d) is not inside the text of %d bytes", p.RegionLo, p.RegionHi, len(ref))
	}
	var cp C.polyhip_pileup_qual_params
	cp.base.region_lo, cp.base.region_hi = C.uint64_t(p.RegionLo), C.uint64_t(p.RegionHi)
	cp.base.min_mapq, cp.base.min_depth = C.uint32_t(p.MinMapq), C.uint32_t(p.MinDepth)
	cp.base.min_alt_count, cp.base.min_alt_permille = C.uint32_t(p.MinAltCount), C.uint32_t(p.MinAltPermille)
	cp.min_base_qual, cp.qual_offset = C.uint32_t(p.MinBaseQual), C.uint32_t(p.QualOffset)
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
	flags, refStart, refEnd, readStart := pad32(r.Flags), pad32(r.RefStart), pad32(r.RefEnd), pad32(r.ReadStart)
	alnA, alnB, qual, text := padB(r.AlignA), padB(r.AlignB), padB(quals), padB(ref)
	var mq *C.uint8_t // nil: no mapq, MinMapq must be 0
	if len(mapq) > 0 {
		mq = (*C.uint8_t)(unsafe.Pointer(&mapq[0]))
	}
	L := int(p.RegionHi - p.RegionLo)
	out := &PileupQualResult{PileupResult: PileupResult{Counts: make([]uint32, PileupChannels*L+1), Consensus: make([]byte, L+1),
		Errs: make([]uint32, n+1)}, Qsum: make([]uint32, PileupChannels/2*L+1)}
	var nsites C.uint64_t
	var err error
	for attempt := 0; attempt < 2; attempt++ {
		out.Sites = make([]PileupSite, siteCap+1)
		err = call(func() C.int {
			return C.polyhip_pileup_qual((*C.polyhip_pileup_qual_params)(unsafe.Pointer(&cp)), C.uint64_t(n),
				(*C.uint32_t)(unsafe.Pointer(&flags[0])), (*C.uint8_t)(unsafe.Pointer(mq)),
				(*C.uint32_t)(unsafe.Pointer(&refStart[0])), (*C.uint32_t)(unsafe.Pointer(&refEnd[0])),
				(*C.uint32_t)(unsafe.Pointer(&readStart[0])),
				(*C.uint8_t)(unsafe.Pointer(&alnA[0])), (*C.uint8_t)(unsafe.Pointer(&alnB[0])),
				(*C.uint64_t)(unsafe.Pointer(&r.AlnOff[0])), (*C.uint8_t)(unsafe.Pointer(&qual[0])),
				(*C.uint64_t)(unsafe.Pointer(&qualOff[0])), (*C.uint8_t)(unsafe.Pointer(&text[0])), C.uint64_t(len(ref)),
				(*C.uint32_t)(unsafe.Pointer(&out.Counts[0])), (*C.uint32_t)(unsafe.Pointer(&out.Qsum[0])),
				(*C.uint8_t)(unsafe.Pointer(&out.Consensus[0])),
				(*C.uint64_t)(unsafe.Pointer(&nsites)), (*C.polyhip_pileup_site)(unsafe.Pointer(&out.Sites[0])),
				C.uint64_t(siteCap), (*C.uint32_t)(unsafe.Pointer(&out.Errs[0])))
		})
		if err == nil || uint64(nsites) <= uint64(siteCap) {
			break
		}
		siteCap = int(nsites)
	}
	if err != nil {
		return nil, err
	}
	out.Counts, out.Consensus, out.Errs = out.Counts[:PileupChannels*L], out.Consensus[:L], out.Errs[:n]
	out.Qsum = out.Qsum[:PileupChannels/2*L]
	out.Sites = out.Sites[:nsites]
	return out, nil
}

// LastPileupQualInfo must run on the OS thread that made the call (runtime.LockOSThread around both).
func LastPileupQualInfo() (PileupQualInfo, error) {
	var ci C.polyhip_pileup_qual_info
	err := call(func() C.int { return C.polyhip_pileup_qual_last_info((*C.polyhip_pileup_qual_info)(unsafe.Pointer(&ci))) })
	return PileupQualInfo{PileupInfo: PileupInfo{Entries: uint64(ci.entries), Used: uint64(ci.used), SkippedMapq: uint64(ci.skipped_mapq),
		Bad: uint64(ci.bad), Columns: uint64(ci.columns), EdgeEvents: uint64(ci.edge_events), Sites: uint64(ci.sites)},
		FilteredBases: uint64(ci.filtered_bases)}, err
}

// PileupRowsParams is polyhip_pileup_rows_params: the region, the origin column 2 counts from (PosOrigin <= RegionLo; column
// 2 prints p - PosOrigin + 1), the minimum mapping quality, the Phred offset of the input qualities and whether positions
// without a read get a row.
type PileupRowsParams struct {
	RegionLo, RegionHi, PosOrigin uint64
	MinMapq, QualOffset           uint32
	AllPositions                  bool
}

// PileupRowsInfo is polyhip_pileup_rows_info.  MaxRowBytes above 65536 means pileup.Parse of the fork refuses the longest row.
type PileupRowsInfo struct {
	Entries, Used, SkippedMapq, Bad, Columns, Tokens, Rows, TextBytes, DroppedEvents, MaxRowBytes uint64
}

// PileupRowsResult: Text holds the rows of the region in ascending position, each "name \t pos \t ref \t depth \t tokens \t
// qualities \n"; the row of position p is Text[RowOff[p-RegionLo]:RowOff[p-RegionLo+1]]; Errs one value per entry.
type PileupRowsResult struct {
	Text   []byte
	RowOff []uint64
	Errs   []uint32
}

// PileupRows writes what the entries of a MapResult say about each position of the text ref as six-column pileup rows, the
// text that pileup.Parse reads.  mapq: the Mapq of AlnRecords (nil: p.MinMapq must be 0 and the byte behind '^' is '~').
// quals / qualOff: as in PileupQual, or nil for rows without qualities.  order: the permutation of CoordOrder, or nil for
// entry order.  textCap: bytes of the text buffer; a call that outgrows it runs once more with the size the library reports.
func PileupRows(r *MapResult, mapq []uint8, quals []byte, qualOff []uint64, ref []byte, order []uint32, name string, p PileupRowsParams,
	textCap int) (*PileupRowsResult, error) {
	n := len(r.Flags)
	if len(r.AlnOff) != n+1 || len(r.RefStart) != n || len(r.RefEnd) != n || (mapq != nil && len(mapq) != n) ||
		(order != nil && len(order) != n) || (quals != nil && (len(qualOff) != n+1 || len(r.ReadStart) != n)) {
		return nil, fmt.Errorf("polyhip.PileupRows: the arrays hold different numbers of entries")
	}
	if p.RegionLo > p.RegionHi || p.RegionHi > uint64(len(ref)) {
		return nil, fmt.Errorf("polyhip.PileupRows: the region [%d, %d) is not inside the text of %d bytes", p.RegionLo, p.RegionHi, len(ref))
	}
	if len(name) == 0 {
		return nil, fmt.Errorf("polyhip.PileupRows: the name is empty")
	}
	var cp C.polyhip_pileup_rows_params
	cp.region_lo, cp.region_hi, cp.pos_origin = C.uint64_t(p.RegionLo), C.uint64_t(p.RegionHi), C.uint64_t(p.PosOrigin)
	cp.min_mapq, cp.qual_offset = C.uint32_t(p.MinMapq), C.uint32_t(p.QualOffset)
	if p.AllPositions {
		cp.all_positions = 1
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
	alnA, alnB, text, nameB := padB(r.AlignA), padB(r.AlignB), padB(ref), []byte(name)
	var mq, qp *C.uint8_t // nil: no mapq; nil: no qualities
	var rsp, op *C.uint32_t
	var qop *C.uint64_t
	if len(mapq) > 0 {
		mq = (*C.uint8_t)(unsafe.Pointer(&mapq[0]))
	}
	if quals != nil && n > 0 {
		qual := padB(quals)
		qp, qop = (*C.uint8_t)(unsafe.Pointer(&qual[0])), (*C.uint64_t)(unsafe.Pointer(&qualOff[0]))
		rsp = (*C.uint32_t)(unsafe.Pointer(&r.ReadStart[0]))
	}
	if len(order) > 0 {
		op = (*C.uint32_t)(unsafe.Pointer(&order[0]))
	}
	L := int(p.RegionHi - p.RegionLo)
	out := &PileupRowsResult{RowOff: make([]uint64, L+1), Errs: make([]uint32, n+1)}
	var ntext C.uint64_t
	var err error
	for attempt := 0; attempt < 2; attempt++ {
		out.Text = make([]byte, textCap+1)
		err = call(func() C.int {
			return C.polyhip_pileup_rows((*C.polyhip_pileup_rows_params)(unsafe.Pointer(&cp)), C.uint64_t(n),
				(*C.uint32_t)(unsafe.Pointer(&flags[0])), (*C.uint8_t)(unsafe.Pointer(mq)),
				(*C.uint32_t)(unsafe.Pointer(&refStart[0])), (*C.uint32_t)(unsafe.Pointer(&refEnd[0])),
				(*C.uint32_t)(unsafe.Pointer(rsp)),
				(*C.uint8_t)(unsafe.Pointer(&alnA[0])), (*C.uint8_t)(unsafe.Pointer(&alnB[0])),
				(*C.uint64_t)(unsafe.Pointer(&r.AlnOff[0])), (*C.uint8_t)(unsafe.Pointer(qp)),
				(*C.uint64_t)(unsafe.Pointer(qop)), (*C.uint8_t)(unsafe.Pointer(&text[0])), C.uint64_t(len(ref)),
				(*C.uint32_t)(unsafe.Pointer(op)), (*C.uint8_t)(unsafe.Pointer(&nameB[0])), C.uint64_t(len(nameB)),
				(*C.uint64_t)(unsafe.Pointer(&ntext)), (*C.uint8_t)(unsafe.Pointer(&out.Text[0])), C.uint64_t(textCap),
				(*C.uint64_t)(unsafe.Pointer(&out.RowOff[0])), (*C.uint32_t)(unsafe.Pointer(&out.Errs[0])))
		})
		if err == nil || uint64(ntext) <= uint64(textCap) {
			break
		}
		textCap = int(ntext)
	}
	if err != nil {
		return nil, err
	}
	out.Text, out.Errs = out.Text[:ntext], out.Errs[:n]
	return out, nil
}

// LastPileupRowsInfo must run on the OS thread that made the call (runtime.LockOSThread around both).
func LastPileupRowsInfo() (PileupRowsInfo, error) {
	var ci C.polyhip_pileup_rows_info
	err := call(func() C.int { return C.polyhip_pileup_rows_last_info((*C.polyhip_pileup_rows_info)(unsafe.Pointer(&ci))) })
	return PileupRowsInfo{Entries: uint64(ci.entries), Used: uint64(ci.used), SkippedMapq: uint64(ci.skipped_mapq), Bad: uint64(ci.bad),
		Columns: uint64(ci.columns), Tokens: uint64(ci.tokens), Rows: uint64(ci.rows), TextBytes: uint64(ci.text_bytes),
		DroppedEvents: uint64(ci.dropped_events), MaxRowBytes: uint64(ci.max_row_bytes)}, err
}
