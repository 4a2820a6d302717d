// cgo binding of the search/bwt entry points of libpolyhip.so (include/polyhip.h, "search/bwt: FM-index").
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

// BWT wraps polyhip_bwt: the FM-index of one sequence, resident on the HIP device that was current when it was
// built (every call runs there).  Close releases it.
type BWT struct{ h *C.polyhip_bwt }

// NewBWT builds the index on the device (search/bwt/bwt.go:455-517); the reference's New errors come back verbatim.
func NewBWT(seq []byte) (*BWT, error) {
	b := &BWT{}
	buf := seq
	if len(buf) == 0 {
		buf = []byte{0} // a valid pointer; n = 0 is refused with the reference's message
	}
	err := call(func() C.int {
		return C.polyhip_bwt_create((*C.uint8_t)(unsafe.Pointer(&buf[0])), C.uint64_t(len(seq)), &b.h)
	})
	if err != nil {
		return nil, err
	}
	runtime.SetFinalizer(b, func(b *BWT) { b.Close() })
	return b, nil
}

func (b *BWT) Close() {
	if b.h != nil {
		C.polyhip_bwt_destroy(b.h)
		b.h = nil
	}
}

// Len is the sequence's length (bwt.go:301-304).
func (b *BWT) Len() int { return int(C.polyhip_bwt_len(b.h)) }

// Transform is the last column, '$' included (bwt.go:306-323).
func (b *BWT) Transform() ([]byte, error) {
	out := make([]byte, b.Len()+1)
	err := call(func() C.int { return C.polyhip_bwt_transform(b.h, (*C.uint8_t)(unsafe.Pointer(&out[0]))) })
	return out, err
}

// CountBatch: the rows [start[p], end[p]) that begin with pattern p of the packed batch; errs[p] = 1 for an empty
// pattern (bwt.go:235-247).
func (b *BWT) CountBatch(pats []byte, offs []uint64) (start, end, errs []uint32, err error) {
	n := len(offs) - 1
	if n <= 0 {
		return nil, nil, nil, nil
	}
	if len(pats) == 0 {
		pats = []byte{0}
	}
	start, end, errs = make([]uint32, n), make([]uint32, n), make([]uint32, n)
	err = call(func() C.int {
		return C.polyhip_bwt_count(b.h, (*C.uint8_t)(unsafe.Pointer(&pats[0])), (*C.uint64_t)(unsafe.Pointer(&offs[0])),
			C.uint64_t(n), (*C.uint32_t)(unsafe.Pointer(&start[0])), (*C.uint32_t)(unsafe.Pointer(&end[0])),
			(*C.uint32_t)(unsafe.Pointer(&errs[0])))
	})
	return start, end, errs, err
}

// LocateBatch: pattern p's offsets are out[first[p]:first[p+1]], in suffix-array row order (bwt.go:249-273).  A
// batch whose offsets outgrow `capacity` runs once more with the size the library reports in first[n].
func (b *BWT) LocateBatch(pats []byte, offs []uint64, capacity int) (first []uint64, out []uint32, errs []uint32, err error) {
	n := len(offs) - 1
	if n <= 0 {
		return []uint64{0}, nil, nil, nil
	}
	if len(pats) == 0 {
		pats = []byte{0}
	}
	first, errs = make([]uint64, n+1), make([]uint32, n)
	for attempt := 0; attempt < 2; attempt++ {
		out = make([]uint32, capacity+1)
		err = call(func() C.int {
			return C.polyhip_bwt_locate(b.h, (*C.uint8_t)(unsafe.Pointer(&pats[0])), (*C.uint64_t)(unsafe.Pointer(&offs[0])),
				C.uint64_t(n), (*C.uint64_t)(unsafe.Pointer(&first[0])), (*C.uint32_t)(unsafe.Pointer(&out[0])),
				C.uint64_t(capacity), (*C.uint32_t)(unsafe.Pointer(&errs[0])))
		})
		if err == nil || first[n] <= uint64(capacity) {
			break
		}
		capacity = int(first[n])
	}
	if err != nil {
		return nil, nil, nil, err
	}
	return first, out[:first[n]], errs, nil
}

// ExtractBatch: request i = sequence[start[i]:end[i]] into out[outOff[i]:]; errs[i] = 0 or the reference's first failing
// check (1 start >= end, 2 end > Len, 3 start < 0; bwt.go:275-299).
func (b *BWT) ExtractBatch(start, end []int64, outOff []uint64) (out []byte, errs []uint32, err error) {
	n := len(start)
	if n == 0 {
		return nil, nil, nil
	}
	if len(end) != n || len(outOff) != n+1 {
		return nil, nil, fmt.Errorf("polyhip: ExtractBatch wants len(end) == len(start) and len(outOff) == len(start) + 1")
	}
	out, errs = make([]byte, outOff[n]+1), make([]uint32, n)
	err = call(func() C.int {
		return C.polyhip_bwt_extract(b.h, (*C.int64_t)(unsafe.Pointer(&start[0])), (*C.int64_t)(unsafe.Pointer(&end[0])),
			C.uint64_t(n), (*C.uint64_t)(unsafe.Pointer(&outOff[0])), (*C.uint8_t)(unsafe.Pointer(&out[0])),
			(*C.uint32_t)(unsafe.Pointer(&errs[0])))
	})
	return out[:outOff[n]], errs, err
}

// MaxMismatches is POLYHIP_BWT_MAX_MISMATCHES: the largest k the search with mismatches takes.
const MaxMismatches = 4

// BWTMismatchInfo mirrors polyhip_bwt_mismatch_info: the calling thread's last CountMismatchBatch / LocateMismatchBatch.
type BWTMismatchInfo struct{ Patterns, Nodes, OccLines, Leaves, Hits uint64 }

// CountMismatchBatch: counts[p*(k+1)+d] = the positions of the sequence at which pattern p of the packed batch has exactly
// d mismatches (substitutions only, matches inside the sequence, k <= MaxMismatches); errs[p] = 1 for an empty pattern.
func (b *BWT) CountMismatchBatch(pats []byte, offs []uint64, k int) (counts, errs []uint32, err error) {
	n := len(offs) - 1
	if n <= 0 { // an empty batch still goes to the library: it refuses k > MaxMismatches first, as for any batch
		n, offs = 0, []uint64{0}
	}
	if len(pats) == 0 {
		pats = []byte{0}
	}
	if k < 0 {
		k = MaxMismatches + 1 // refused by the library
	}
	counts, errs = make([]uint32, n*(k+1)+1), make([]uint32, n+1)
	err = call(func() C.int {
		return C.polyhip_bwt_count_mismatch(b.h, (*C.uint8_t)(unsafe.Pointer(&pats[0])), (*C.uint64_t)(unsafe.Pointer(&offs[0])),
			C.uint64_t(n), C.uint32_t(k), (*C.uint32_t)(unsafe.Pointer(&counts[0])), (*C.uint32_t)(unsafe.Pointer(&errs[0])))
	})
	if err != nil {
		return nil, nil, err
	}
	return counts[:n*(k+1)], errs[:n], nil
}

// LocateMismatchBatch: pattern p's hits are pos[first[p]:first[p+1]], ascending, with their mismatches in mm.  A batch
// whose hits outgrow `capacity` runs once more with the size the library reports in first[n].
func (b *BWT) LocateMismatchBatch(pats []byte, offs []uint64, k, capacity int) (first []uint64, pos []uint32, mm []uint8, errs []uint32, err error) {
	n := len(offs) - 1
	if n <= 0 { // as CountMismatchBatch: the library answers an empty batch too (first[0] = 0, or k refused)
		n, offs = 0, []uint64{0}
	}
	if len(pats) == 0 {
		pats = []byte{0}
	}
	if k < 0 {
		k = MaxMismatches + 1
	}
	if capacity < 0 {
		capacity = 0
	}
	first, errs = make([]uint64, n+1), make([]uint32, n+1)
	for attempt := 0; attempt < 2; attempt++ {
		pos, mm = make([]uint32, capacity+1), make([]uint8, capacity+1)
		err = call(func() C.int {
			return C.polyhip_bwt_locate_mismatch(b.h, (*C.uint8_t)(unsafe.Pointer(&pats[0])), (*C.uint64_t)(unsafe.Pointer(&offs[0])),
				C.uint64_t(n), C.uint32_t(k), (*C.uint64_t)(unsafe.Pointer(&first[0])), (*C.uint32_t)(unsafe.Pointer(&pos[0])),
				(*C.uint8_t)(unsafe.Pointer(&mm[0])), C.uint64_t(capacity), (*C.uint32_t)(unsafe.Pointer(&errs[0])))
		})
		if err == nil || first[n] <= uint64(capacity) {
			break
		}
		capacity = int(first[n])
	}
	if err != nil {
		return nil, nil, nil, nil, err
	}
	return first, pos[:first[n]], mm[:first[n]], errs[:n], nil
}

// MismatchLastInfo: polyhip_bwt_mismatch_last_info (thread-local in the library: lock the goroutine to its OS thread
// around the search and this call if the figures must belong together).
func MismatchLastInfo() (BWTMismatchInfo, error) {
	var info C.polyhip_bwt_mismatch_info
	err := call(func() C.int { return C.polyhip_bwt_mismatch_last_info((*C.polyhip_bwt_mismatch_info)(unsafe.Pointer(&info))) })
	return BWTMismatchInfo{uint64(info.patterns), uint64(info.nodes), uint64(info.occ_lines), uint64(info.leaves), uint64(info.hits)}, err
}
