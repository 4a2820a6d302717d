// cgo binding of the alignment records of libpolyhip.so (include/polyhip.h, "the mapper's output as alignment records").
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

// AlnRecordsInfo is polyhip_aln_records_info: what the calling OS thread's last AlnRecords did.
type AlnRecordsInfo struct {
	Entries, Mapped, Columns, CigarOps, MdBytes, Bad uint64
}

// AlnRecordsResult holds one entry per entry of the MapResult: entry i's CIGAR is Cigar[CigarOff[i]:CigarOff[i+1]] (BAM's
// len<<4|op), its MD string Md[MdOff[i]:MdOff[i+1]].  Mapq is a stated convention, not a calibrated quality.
type AlnRecordsResult struct {
	CigarOff, MdOff   []uint64
	Cigar             []uint32
	Md                []byte
	Nm, SamFlag, Errs []uint32
	Mapq              []uint8
}

// AlnRecords turns a MapResult (of MapReads, MapReadsAffine or MapPairs; readLen[i] is the length of read i, in the result's
// order) into CIGAR, NM, MD, MAPQ and the SAM FLAG word.  eqx: '=' and 'X' instead of 'M'; paired: the entries are mates
// (2i, 2i+1).  cigarCap, mdCap: entries / bytes of the two buffers; a batch that outgrows them runs once more with the sizes
// the library reports in CigarOff[n] and MdOff[n].
func AlnRecords(r *MapResult, readLen []uint32, eqx, paired bool, cigarCap, mdCap int) (*AlnRecordsResult, error) {
	n := len(r.Flags)
	if len(readLen) != n || len(r.AlnOff) != n+1 {
		return nil, fmt.Errorf("polyhip.AlnRecords: readLen and the result hold different numbers of entries")
	}
	var cp C.polyhip_aln_records_params
	if eqx {
		cp.eqx = 1
	}
	if paired {
		cp.paired = 1
	}
	pad32 := func(s []uint32) []uint32 { // an empty batch still needs &s[0]
		if len(s) == 0 {
			return []uint32{0}
		}
		return s
	}
	pad64 := func(s []int64) []int64 {
		if len(s) == 0 {
			return []int64{0}
		}
		return s
	}
	padB := func(s []byte) []byte {
		if len(s) == 0 {
			return []byte{0}
		}
		return s
	}
	flags, readStart, readEnd, rl := pad32(r.Flags), pad32(r.ReadStart), pad32(r.ReadEnd), pad32(readLen)
	score, second := pad64(r.Score), pad64(r.Second)
	alnA, alnB := padB(r.AlignA), padB(r.AlignB)
	m := n
	if m == 0 {
		m = 1
	}
	out := &AlnRecordsResult{CigarOff: make([]uint64, n+1), MdOff: make([]uint64, n+1), Nm: make([]uint32, m), SamFlag: make([]uint32, m),
		Errs: make([]uint32, m), Mapq: make([]uint8, m)}
	var err error
	for attempt := 0; attempt < 2; attempt++ {
		out.Cigar, out.Md = make([]uint32, cigarCap+1), make([]byte, mdCap+1)
		err = call(func() C.int {
			return C.polyhip_aln_records((*C.polyhip_aln_records_params)(unsafe.Pointer(&cp)), C.uint64_t(n),
				(*C.uint32_t)(unsafe.Pointer(&flags[0])), (*C.int64_t)(unsafe.Pointer(&score[0])),
				(*C.int64_t)(unsafe.Pointer(&second[0])), (*C.uint32_t)(unsafe.Pointer(&readStart[0])),
				(*C.uint32_t)(unsafe.Pointer(&readEnd[0])), (*C.uint32_t)(unsafe.Pointer(&rl[0])),
				(*C.uint8_t)(unsafe.Pointer(&alnA[0])), (*C.uint8_t)(unsafe.Pointer(&alnB[0])),
				(*C.uint64_t)(unsafe.Pointer(&r.AlnOff[0])), (*C.uint64_t)(unsafe.Pointer(&out.CigarOff[0])),
				(*C.uint32_t)(unsafe.Pointer(&out.Cigar[0])), C.uint64_t(cigarCap), (*C.uint64_t)(unsafe.Pointer(&out.MdOff[0])),
				(*C.uint8_t)(unsafe.Pointer(&out.Md[0])), C.uint64_t(mdCap), (*C.uint32_t)(unsafe.Pointer(&out.Nm[0])),
				(*C.uint8_t)(unsafe.Pointer(&out.Mapq[0])), (*C.uint32_t)(unsafe.Pointer(&out.SamFlag[0])),
				(*C.uint32_t)(unsafe.Pointer(&out.Errs[0])))
		})
		if err == nil || (out.CigarOff[n] <= uint64(cigarCap) && out.MdOff[n] <= uint64(mdCap)) {
			break
		}
		cigarCap, mdCap = int(out.CigarOff[n]), int(out.MdOff[n])
	}
	if err != nil {
		return nil, err
	}
	out.Cigar, out.Md = out.Cigar[:out.CigarOff[n]], out.Md[:out.MdOff[n]]
	out.Nm, out.SamFlag, out.Errs, out.Mapq = out.Nm[:n], out.SamFlag[:n], out.Errs[:n], out.Mapq[:n]
	return out, nil
}

// LastAlnRecordsInfo must run on the OS thread that made the call (runtime.LockOSThread around both).
func LastAlnRecordsInfo() (AlnRecordsInfo, error) {
	var ci C.polyhip_aln_records_info
	err := call(func() C.int { return C.polyhip_aln_records_last_info((*C.polyhip_aln_records_info)(unsafe.Pointer(&ci))) })
	return AlnRecordsInfo{Entries: uint64(ci.entries), Mapped: uint64(ci.mapped), Columns: uint64(ci.columns),
		CigarOps: uint64(ci.cigar_ops), MdBytes: uint64(ci.md_bytes), Bad: uint64(ci.bad)}, err
}
