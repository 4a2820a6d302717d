// cgo binding of the affine-gap SmithWaterman entry points of libpolyhip.so (include/polyhip.h, "search/align
// SmithWaterman with affine gaps").
// UNCOMPILED in the authoring image (no Go toolchain).
package polyhip

/*
#include "polyhip.h"
*/
import "C"

import "unsafe"

// SWAffineBatch: the score pass with affine gaps (the first symbol of a gap costs gapOpen, each further one gapExtend;
// the handle's own gap is ignored) for every A against one shared B (offB == nil) or pairwise.  Results carry Score,
// EndA, EndB and Err; the strings stay empty.
func (s *Scoring) SWAffineBatch(gapOpen, gapExtend int, A []byte, offA []uint64, B []byte, offB []uint64) ([]AlignResult, error) {
	n := len(offA) - 1
	var pOffB *C.uint64_t
	shared := C.uint64_t(len(B))
	if offB != nil {
		pOffB = (*C.uint64_t)(unsafe.Pointer(&offB[0]))
		shared = 0
	}
	if len(A) == 0 {
		A = []byte{0} // a valid pointer: every read is empty
	}
	if len(B) == 0 {
		B = []byte{0} // a valid pointer: an empty reference gives score 0 and empty strings
	}
	score := make([]int64, n+1)
	endA, endB, errs := make([]uint32, n+1), make([]uint32, n+1), make([]uint32, n+1)
	err := call(func() C.int {
		return C.polyhip_sw_affine_batch((*C.polyhip_scoring)(s.h), C.int64_t(gapOpen), C.int64_t(gapExtend),
			(*C.uint8_t)(unsafe.Pointer(&A[0])), (*C.uint64_t)(unsafe.Pointer(&offA[0])), C.uint64_t(n),
			(*C.uint8_t)(unsafe.Pointer(&B[0])), (*C.uint64_t)(pOffB), C.uint64_t(shared),
			(*C.int64_t)(unsafe.Pointer(&score[0])), (*C.uint32_t)(unsafe.Pointer(&endA[0])),
			(*C.uint32_t)(unsafe.Pointer(&endB[0])), (*C.uint32_t)(unsafe.Pointer(&errs[0])))
	})
	if err != nil {
		return nil, err
	}
	res := make([]AlignResult, n)
	for p := 0; p < n; p++ {
		res[p] = AlignResult{Score: score[p], Err: errs[p], EndA: endA[p], EndB: endB[p]}
	}
	return res, nil
}

// SWAffineAlignBatch: the whole affine SmithWaterman with packed strings (polyhip_sw_affine_align_batch_packed); a batch
// whose strings outgrow the first guess is run once more with the size the library reports, as SWAlignBatch does.
func (s *Scoring) SWAffineAlignBatch(gapOpen, gapExtend int, A []byte, offA []uint64, B []byte, offB []uint64) ([]AlignResult, error) {
	n := len(offA) - 1
	var pOffB *C.uint64_t
	shared := C.uint64_t(len(B))
	if offB != nil {
		pOffB = (*C.uint64_t)(unsafe.Pointer(&offB[0]))
		shared = 0
	}
	if len(A) == 0 {
		A = []byte{0} // a valid pointer: every read is empty
	}
	if len(B) == 0 {
		B = []byte{0} // a valid pointer: an empty reference gives score 0 and empty strings
	}
	score := make([]int64, n+1)
	endA, endB, errs := make([]uint32, n+1), make([]uint32, n+1), make([]uint32, n+1)
	off := make([]uint64, n+1)
	capacity := uint64(len(A)) + uint64(len(A))/4 + 65536
	var alnA, alnB []byte
	for attempt := 0; ; attempt++ {
		alnA, alnB = make([]byte, capacity+1), make([]byte, capacity+1)
		var status C.int
		err := call(func() C.int {
			status = C.polyhip_sw_affine_align_batch_packed((*C.polyhip_scoring)(s.h), C.int64_t(gapOpen), C.int64_t(gapExtend),
				(*C.uint8_t)(unsafe.Pointer(&A[0])), (*C.uint64_t)(unsafe.Pointer(&offA[0])), C.uint64_t(n),
				(*C.uint8_t)(unsafe.Pointer(&B[0])), (*C.uint64_t)(pOffB), C.uint64_t(shared),
				(*C.int64_t)(unsafe.Pointer(&score[0])), (*C.uint32_t)(unsafe.Pointer(&endA[0])),
				(*C.uint32_t)(unsafe.Pointer(&endB[0])), (*C.uint32_t)(unsafe.Pointer(&errs[0])),
				(*C.uint8_t)(unsafe.Pointer(&alnA[0])), (*C.uint8_t)(unsafe.Pointer(&alnB[0])),
				(*C.uint64_t)(unsafe.Pointer(&off[0])), C.uint64_t(capacity))
			return status
		})
		if err != nil && attempt == 0 && status == C.POLYHIP_ERR_INVALID && off[n] > capacity {
			capacity = off[n] // the strings did not fit: alnOff[npairs] is what they need
			continue
		}
		if err != nil {
			return nil, err
		}
		break
	}
	res := make([]AlignResult, n)
	for p := 0; p < n; p++ {
		res[p] = AlignResult{Score: score[p], AlignA: string(alnA[off[p]:off[p+1]]), AlignB: string(alnB[off[p]:off[p+1]]), Err: errs[p],
			EndA: endA[p], EndB: endB[p]}
	}
	return res, nil
}
