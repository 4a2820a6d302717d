// cgo binding of read trimming of libpolyhip.so (include/polyhip.h, "read trimming: quality ends, 3' adapters, mate
// overlap").
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

// Flags of a trimmed entry (Trimmed.Flags); bits 8..15 hold the index of the adapter that hit.
const (
	TrimQual3p  = 1  // the 3' end lost bytes to the quality cut-off
	TrimQual5p  = 2  // the 5' end did
	TrimAdapter = 4  // an adapter was found and cut off
	TrimShort   = 8  // shorter than MinLen: empty in the output
	TrimOverlap = 16 // cut at the insert the two mates agree on
)

// TrimParams is polyhip_trim_params.  A cut-off of 0 switches that end off, PairMinOverlap 0 the mate overlap; MinOverlap is
// at least 1.
type TrimParams struct {
	QualOffset, MinQual5p, MinQual3p, AdapterErrPct, MinOverlap, MinLen, PairMinOverlap, PairErrPct uint32
}

// TrimInfo is polyhip_trim_info: what the calling OS thread's last TrimReads / TrimPairs did.
type TrimInfo struct {
	Reads, BytesIn, BytesOut, Cut3p, Cut5p, AdapterHits, OverlapCut, TooShort, Bad uint64
}

// TrimBatch is one trimmed batch: read i is Seqs[Offs[i]:Offs[i+1]], its qualities Quals[Offs[i]:Offs[i+1]] (nil when none
// were handed in).  An emptied read has length 0; no read is removed.
type TrimBatch struct {
	Seqs  []byte
	Offs  []uint64
	Quals []byte
}

// Trimmed: one value per entry.  Start and End of what was kept, Flags as the Trim* constants, Errs as the header numbers
// them (1: the quality string has another length than the read, 2: a quality byte out of range).
type Trimmed struct {
	Start, End, Flags, Errs []uint32
}

func trimParams(p TrimParams) C.polyhip_trim_params {
	var cp C.polyhip_trim_params
	cp.qual_offset, cp.min_qual_5p, cp.min_qual_3p = C.uint32_t(p.QualOffset), C.uint32_t(p.MinQual5p), C.uint32_t(p.MinQual3p)
	cp.adapter_err_pct, cp.min_overlap, cp.min_len = C.uint32_t(p.AdapterErrPct), C.uint32_t(p.MinOverlap), C.uint32_t(p.MinLen)
	cp.pair_min_overlap, cp.pair_err_pct = C.uint32_t(p.PairMinOverlap), C.uint32_t(p.PairErrPct)
	return cp
}

// packAdapters: the adapters back to back and their nadapters + 1 offsets (one spare byte: an empty list still needs &b[0])
func packAdapters(adapters []string) ([]byte, []uint32) {
	buf, off := []byte{}, make([]uint32, 1, len(adapters)+1)
	for _, a := range adapters {
		buf = append(buf, a...)
		off = append(off, uint32(len(buf)))
	}
	return append(buf, 0), off
}

// trimIn is one batch as the C call wants it: pointers to the first elements, nil for absent qualities, and its output
type trimIn struct {
	reads, quals, outReads, outQuals *C.uint8_t
	offs, qualOffs, outOffs          *C.uint64_t
	out                              TrimBatch
}

func newTrimIn(who string, reads []byte, offs []uint64, quals []byte, qualOffs []uint64) (*trimIn, error) {
	n := len(offs) - 1
	if n < 0 || (qualOffs != nil && len(qualOffs) != n+1) {
		return nil, fmt.Errorf("polyhip.%s: offsets hold one entry more than there are reads", who)
	}
	if offs[n] < offs[0] || uint64(len(reads)) < offs[n] || (qualOffs != nil && uint64(len(quals)) < qualOffs[n]) {
		return nil, fmt.Errorf("polyhip.%s: the offsets reach beyond the bytes", who)
	}
	t := &trimIn{}
	total := int(offs[n] - offs[0])
	t.out = TrimBatch{Seqs: make([]byte, total+1), Offs: make([]uint64, n+1)}
	pad := func(s []byte) []byte { // an empty batch still needs &s[0]
		if len(s) == 0 {
			return []byte{0}
		}
		return s
	}
	reads = pad(reads)
	t.reads, t.offs = (*C.uint8_t)(unsafe.Pointer(&reads[0])), (*C.uint64_t)(unsafe.Pointer(&offs[0]))
	t.outReads, t.outOffs = (*C.uint8_t)(unsafe.Pointer(&t.out.Seqs[0])), (*C.uint64_t)(unsafe.Pointer(&t.out.Offs[0]))
	if qualOffs != nil {
		quals = pad(quals)
		t.out.Quals = make([]byte, total+1)
		t.quals, t.qualOffs = (*C.uint8_t)(unsafe.Pointer(&quals[0])), (*C.uint64_t)(unsafe.Pointer(&qualOffs[0]))
		t.outQuals = (*C.uint8_t)(unsafe.Pointer(&t.out.Quals[0]))
	}
	return t, nil
}

func (t *trimIn) result() TrimBatch {
	kept := t.out.Offs[len(t.out.Offs)-1]
	t.out.Seqs = t.out.Seqs[:kept]
	if t.out.Quals != nil {
		t.out.Quals = t.out.Quals[:kept]
	}
	return t.out
}

func newTrimmed(entries int) *Trimmed {
	return &Trimmed{Start: make([]uint32, entries+1), End: make([]uint32, entries+1), Flags: make([]uint32, entries+1),
		Errs: make([]uint32, entries+1)}
}

func (t *Trimmed) cut(entries int) {
	t.Start, t.End, t.Flags, t.Errs = t.Start[:entries], t.End[:entries], t.Flags[:entries], t.Errs[:entries]
}

// TrimReads cuts low-quality ends and 3' adapters off a packed batch (reads, offs as the mappers take them; quals, qualOffs
// as FastqPackQual packs them, or both nil).  adapters: up to 255 strings of 1..64 upper-case ACGT.  Entry i in is entry i
// out.
func TrimReads(reads []byte, offs []uint64, quals []byte, qualOffs []uint64, adapters []string, p TrimParams) (*TrimBatch, *Trimmed, error) {
	in, err := newTrimIn("TrimReads", reads, offs, quals, qualOffs)
	if err != nil {
		return nil, nil, err
	}
	n := len(offs) - 1
	cp := trimParams(p)
	ad, adOff := packAdapters(adapters)
	res := newTrimmed(n)
	err = call(func() C.int {
		return C.polyhip_trim_reads((*C.polyhip_trim_params)(unsafe.Pointer(&cp)), (*C.uint8_t)(unsafe.Pointer(&ad[0])),
			(*C.uint32_t)(unsafe.Pointer(&adOff[0])), C.uint32_t(len(adapters)), (*C.uint8_t)(unsafe.Pointer(in.reads)),
			(*C.uint64_t)(unsafe.Pointer(in.offs)), (*C.uint8_t)(unsafe.Pointer(in.quals)), (*C.uint64_t)(unsafe.Pointer(in.qualOffs)),
			C.uint64_t(n), (*C.uint32_t)(unsafe.Pointer(&res.Start[0])), (*C.uint32_t)(unsafe.Pointer(&res.End[0])),
			(*C.uint32_t)(unsafe.Pointer(&res.Flags[0])), (*C.uint32_t)(unsafe.Pointer(&res.Errs[0])),
			(*C.uint8_t)(unsafe.Pointer(in.outReads)), (*C.uint8_t)(unsafe.Pointer(in.outQuals)), (*C.uint64_t)(unsafe.Pointer(in.outOffs)))
	})
	if err != nil {
		return nil, nil, err
	}
	res.cut(n)
	out := in.result()
	return &out, res, nil
}

// TrimPairs is TrimReads on two batches of mates (mate i of the first with mate i of the second) with the mate overlap
// between the adapter search and the length rule.  The entries of the Trimmed are 2i (mate 1) and 2i+1 (mate 2), as
// MapPairs orders its result; each mate has an output batch of its own.
func TrimPairs(reads1 []byte, offs1 []uint64, quals1 []byte, qualOffs1 []uint64, reads2 []byte, offs2 []uint64, quals2 []byte, qualOffs2 []uint64, adapters []string, p TrimParams) (*TrimBatch, *TrimBatch, *Trimmed, error) {
	if len(offs1) != len(offs2) {
		return nil, nil, nil, fmt.Errorf("polyhip.TrimPairs: the two batches hold different numbers of reads")
	}
	in1, err := newTrimIn("TrimPairs", reads1, offs1, quals1, qualOffs1)
	if err != nil {
		return nil, nil, nil, err
	}
	in2, err := newTrimIn("TrimPairs", reads2, offs2, quals2, qualOffs2)
	if err != nil {
		return nil, nil, nil, err
	}
	n := len(offs1) - 1
	cp := trimParams(p)
	ad, adOff := packAdapters(adapters)
	res := newTrimmed(2 * n)
	err = call(func() C.int {
		return C.polyhip_trim_pairs((*C.polyhip_trim_params)(unsafe.Pointer(&cp)), (*C.uint8_t)(unsafe.Pointer(&ad[0])),
			(*C.uint32_t)(unsafe.Pointer(&adOff[0])), C.uint32_t(len(adapters)),
			(*C.uint8_t)(unsafe.Pointer(in1.reads)), (*C.uint64_t)(unsafe.Pointer(in1.offs)),
			(*C.uint8_t)(unsafe.Pointer(in1.quals)), (*C.uint64_t)(unsafe.Pointer(in1.qualOffs)),
			(*C.uint8_t)(unsafe.Pointer(in2.reads)), (*C.uint64_t)(unsafe.Pointer(in2.offs)),
			(*C.uint8_t)(unsafe.Pointer(in2.quals)), (*C.uint64_t)(unsafe.Pointer(in2.qualOffs)), C.uint64_t(n),
			(*C.uint32_t)(unsafe.Pointer(&res.Start[0])), (*C.uint32_t)(unsafe.Pointer(&res.End[0])),
			(*C.uint32_t)(unsafe.Pointer(&res.Flags[0])), (*C.uint32_t)(unsafe.Pointer(&res.Errs[0])),
			(*C.uint8_t)(unsafe.Pointer(in1.outReads)), (*C.uint8_t)(unsafe.Pointer(in1.outQuals)), (*C.uint64_t)(unsafe.Pointer(in1.outOffs)),
			(*C.uint8_t)(unsafe.Pointer(in2.outReads)), (*C.uint8_t)(unsafe.Pointer(in2.outQuals)), (*C.uint64_t)(unsafe.Pointer(in2.outOffs)))
	})
	if err != nil {
		return nil, nil, nil, err
	}
	res.cut(2 * n)
	out1, out2 := in1.result(), in2.result()
	return &out1, &out2, res, nil
}

// LastTrimInfo must run on the OS thread that made the call (runtime.LockOSThread around both).
func LastTrimInfo() (TrimInfo, error) {
	var ci C.polyhip_trim_info
	err := call(func() C.int { return C.polyhip_trim_last_info((*C.polyhip_trim_info)(unsafe.Pointer(&ci))) })
	return TrimInfo{Reads: uint64(ci.reads), BytesIn: uint64(ci.bytes_in), BytesOut: uint64(ci.bytes_out), Cut3p: uint64(ci.cut_3p),
		Cut5p: uint64(ci.cut_5p), AdapterHits: uint64(ci.adapter_hits), OverlapCut: uint64(ci.overlap_cut),
		TooShort: uint64(ci.too_short), Bad: uint64(ci.bad)}, err
}
