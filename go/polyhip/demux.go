// cgo binding of demultiplexing of libpolyhip.so (include/polyhip.h, "demultiplexing: pooled reads split by inline 5'
// barcodes").
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

// DemuxNone is "none" in Demuxed.Barcode, BStart, Mism and Sample, and a hole in a pair table.
const DemuxNone = 0xFFFFFFFF

// Flags of a demultiplexed entry (Demuxed.Flags).
const (
	DemuxNoBarcode  = 1 // no barcode within MaxMismatches
	DemuxAmbiguous  = 2 // the runner-up is less than MinMargin behind
	DemuxNotInSheet = 4 // both mates have a barcode, the table has no sample for the combination
)

// DemuxParams is polyhip_demux_params without nsamples, which the calls take from the barcodes or the table.
type DemuxParams struct {
	MaxShift, MaxMismatches, MinMargin, Clip, ClipExtra uint32
}

// DemuxInfo is polyhip_demux_info: what the calling OS thread's last DemuxReads / DemuxPairs did.
type DemuxInfo struct {
	Reads, Assigned, Exact, NoBarcode, Ambiguous, NotInSheet, Bad, BytesIn, BytesOut uint64
}

// Demuxed: one value per entry in Barcode, BStart, Mism, Flags and Errs (pairs: 2i is mate 1, 2i+1 mate 2), one per read or
// pair in Sample and Order.  Output read j is input read Order[j]; sample k is output reads SampleStart[k] ..
// SampleStart[k+1], the unassigned are sample NSamples.
type Demuxed struct {
	NSamples                           int
	Barcode, BStart, Mism, Flags, Errs []uint32
	Sample, Order                      []uint32
	SampleStart                        []uint64
}

// SampleOffs is the slice of a grouped batch's offsets that holds sample k (k == NSamples: the unassigned): with the batch's
// Seqs and Quals it goes to TrimReads and the mappers as it is.
func (d *Demuxed) SampleOffs(b *TrimBatch, k int) []uint64 {
	return b.Offs[d.SampleStart[k] : d.SampleStart[k+1]+1]
}

func demuxParams(p DemuxParams, nsamples int) C.polyhip_demux_params {
	var cp C.polyhip_demux_params
	cp.max_shift, cp.max_mismatches, cp.min_margin = C.uint32_t(p.MaxShift), C.uint32_t(p.MaxMismatches), C.uint32_t(p.MinMargin)
	cp.clip, cp.clip_extra, cp.nsamples = C.uint32_t(p.Clip), C.uint32_t(p.ClipExtra), C.uint32_t(nsamples)
	return cp
}

func newDemuxed(entries, n, nsamples int) *Demuxed {
	return &Demuxed{NSamples: nsamples, Barcode: make([]uint32, entries+1), BStart: make([]uint32, entries+1),
		Mism: make([]uint32, entries+1), Flags: make([]uint32, entries+1), Errs: make([]uint32, entries+1),
		Sample: make([]uint32, n+1), Order: make([]uint32, n+1), SampleStart: make([]uint64, nsamples+2)}
}

func (d *Demuxed) cut(entries, n int) {
	d.Barcode, d.BStart, d.Mism, d.Flags, d.Errs = d.Barcode[:entries], d.BStart[:entries], d.Mism[:entries], d.Flags[:entries], d.Errs[:entries]
	d.Sample, d.Order = d.Sample[:n], d.Order[:n]
}

// DemuxReads finds the inline 5' barcode of every read of a packed batch (reads, offs as the mappers take them; quals,
// qualOffs as FastqPackQual packs them, or both nil) and returns the batch grouped by sample.  barcodes: 1..4096 strings of
// 4..64 upper-case ACGT; barcode k is sample k.
func DemuxReads(reads []byte, offs []uint64, quals []byte, qualOffs []uint64, barcodes []string, p DemuxParams) (*TrimBatch, *Demuxed, error) {
	in, err := newTrimIn("DemuxReads", reads, offs, quals, qualOffs)
	if err != nil {
		return nil, nil, err
	}
	if len(barcodes) < 1 || len(barcodes) > 4096 {
		return nil, nil, fmt.Errorf("polyhip.DemuxReads: %d barcodes, a set holds 1..4096", len(barcodes))
	}
	n := len(offs) - 1
	cp := demuxParams(p, len(barcodes))
	bc, bcOff := packAdapters(barcodes)
	res := newDemuxed(n, n, len(barcodes))
	err = call(func() C.int {
		return C.polyhip_demux_reads((*C.polyhip_demux_params)(unsafe.Pointer(&cp)), (*C.uint8_t)(unsafe.Pointer(&bc[0])),
			(*C.uint32_t)(unsafe.Pointer(&bcOff[0])), C.uint32_t(len(barcodes)), (*C.uint8_t)(unsafe.Pointer(in.reads)),
			(*C.uint64_t)(unsafe.Pointer(in.offs)), (*C.uint8_t)(unsafe.Pointer(in.quals)), (*C.uint64_t)(unsafe.Pointer(in.qualOffs)),
			C.uint64_t(n), (*C.uint32_t)(unsafe.Pointer(&res.Barcode[0])), (*C.uint32_t)(unsafe.Pointer(&res.BStart[0])),
			(*C.uint32_t)(unsafe.Pointer(&res.Mism[0])), (*C.uint32_t)(unsafe.Pointer(&res.Flags[0])),
			(*C.uint32_t)(unsafe.Pointer(&res.Errs[0])), (*C.uint32_t)(unsafe.Pointer(&res.Sample[0])),
			(*C.uint32_t)(unsafe.Pointer(&res.Order[0])), (*C.uint64_t)(unsafe.Pointer(&res.SampleStart[0])),
			(*C.uint8_t)(unsafe.Pointer(in.outReads)), (*C.uint8_t)(unsafe.Pointer(in.outQuals)), (*C.uint64_t)(unsafe.Pointer(in.outOffs)))
	})
	if err != nil {
		return nil, nil, err
	}
	res.cut(n, n)
	out := in.result()
	return &out, res, nil
}

// DemuxPairs is DemuxReads on two batches of mates (mate i of the first with mate i of the second).  With barcodes2 empty
// mate 1's barcode is the sample and pairSample is nil; otherwise pairSample holds len(barcodes1) * len(barcodes2) samples
// below nsamples, row b1, column b2, DemuxNone for a combination that is not in the sheet.  Each mate has an output batch
// of its own, both in the same Order.
func DemuxPairs(reads1 []byte, offs1 []uint64, quals1 []byte, qualOffs1 []uint64, reads2 []byte, offs2 []uint64, quals2 []byte, qualOffs2 []uint64, barcodes1, barcodes2 []string, pairSample []uint32, nsamples int, p DemuxParams) (*TrimBatch, *TrimBatch, *Demuxed, error) {
	if len(offs1) != len(offs2) {
		return nil, nil, nil, fmt.Errorf("polyhip.DemuxPairs: the two batches hold different numbers of reads")
	}
	if len(barcodes2) == 0 {
		nsamples, pairSample = len(barcodes1), nil
	} else if len(pairSample) != len(barcodes1)*len(barcodes2) {
		return nil, nil, nil, fmt.Errorf("polyhip.DemuxPairs: pairSample holds len(barcodes1) * len(barcodes2) entries")
	}
	if nsamples < 1 || nsamples > 65536 {
		return nil, nil, nil, fmt.Errorf("polyhip.DemuxPairs: %d samples, there are 1..65536", nsamples)
	}
	in1, err := newTrimIn("DemuxPairs", reads1, offs1, quals1, qualOffs1)
	if err != nil {
		return nil, nil, nil, err
	}
	in2, err := newTrimIn("DemuxPairs", reads2, offs2, quals2, qualOffs2)
	if err != nil {
		return nil, nil, nil, err
	}
	n := len(offs1) - 1
	cp := demuxParams(p, nsamples)
	bc1, bcOff1 := packAdapters(barcodes1)
	bc2, bcOff2 := packAdapters(barcodes2)
	var table *C.uint32_t
	if pairSample != nil {
		table = (*C.uint32_t)(unsafe.Pointer(&pairSample[0]))
	}
	res := newDemuxed(2*n, n, nsamples)
	err = call(func() C.int {
		return C.polyhip_demux_pairs((*C.polyhip_demux_params)(unsafe.Pointer(&cp)), (*C.uint8_t)(unsafe.Pointer(&bc1[0])),
			(*C.uint32_t)(unsafe.Pointer(&bcOff1[0])), C.uint32_t(len(barcodes1)), (*C.uint8_t)(unsafe.Pointer(&bc2[0])),
			(*C.uint32_t)(unsafe.Pointer(&bcOff2[0])), C.uint32_t(len(barcodes2)), (*C.uint32_t)(unsafe.Pointer(table)),
			(*C.uint8_t)(unsafe.Pointer(in1.reads)), (*C.uint64_t)(unsafe.Pointer(in1.offs)),
			(*C.uint8_t)(unsafe.Pointer(in1.quals)), (*C.uint64_t)(unsafe.Pointer(in1.qualOffs)),
			(*C.uint8_t)(unsafe.Pointer(in2.reads)), (*C.uint64_t)(unsafe.Pointer(in2.offs)),
			(*C.uint8_t)(unsafe.Pointer(in2.quals)), (*C.uint64_t)(unsafe.Pointer(in2.qualOffs)), C.uint64_t(n),
			(*C.uint32_t)(unsafe.Pointer(&res.Barcode[0])), (*C.uint32_t)(unsafe.Pointer(&res.BStart[0])),
			(*C.uint32_t)(unsafe.Pointer(&res.Mism[0])), (*C.uint32_t)(unsafe.Pointer(&res.Flags[0])),
			(*C.uint32_t)(unsafe.Pointer(&res.Errs[0])), (*C.uint32_t)(unsafe.Pointer(&res.Sample[0])),
			(*C.uint32_t)(unsafe.Pointer(&res.Order[0])), (*C.uint64_t)(unsafe.Pointer(&res.SampleStart[0])),
			(*C.uint8_t)(unsafe.Pointer(in1.outReads)), (*C.uint8_t)(unsafe.Pointer(in1.outQuals)), (*C.uint64_t)(unsafe.Pointer(in1.outOffs)),
			(*C.uint8_t)(unsafe.Pointer(in2.outReads)), (*C.uint8_t)(unsafe.Pointer(in2.outQuals)), (*C.uint64_t)(unsafe.Pointer(in2.outOffs)))
	})
	if err != nil {
		return nil, nil, nil, err
	}
	res.cut(2*n, n)
	out1, out2 := in1.result(), in2.result()
	return &out1, &out2, res, nil
}

// LastDemuxInfo must run on the OS thread that made the call (runtime.LockOSThread around both).
func LastDemuxInfo() (DemuxInfo, error) {
	var ci C.polyhip_demux_info
	err := call(func() C.int { return C.polyhip_demux_last_info((*C.polyhip_demux_info)(unsafe.Pointer(&ci))) })
	return DemuxInfo{Reads: uint64(ci.reads), Assigned: uint64(ci.assigned), Exact: uint64(ci.exact), NoBarcode: uint64(ci.no_barcode),
		Ambiguous: uint64(ci.ambiguous), NotInSheet: uint64(ci.not_in_sheet), Bad: uint64(ci.bad), BytesIn: uint64(ci.bytes_in),
		BytesOut: uint64(ci.bytes_out)}, err
}
