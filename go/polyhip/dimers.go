// cgo binding of the primer-dimer screen of libpolyhip.so (include/polyhip.h, "primer dimers: which primers of a pool bind
// each other").
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

// DimerNone is "no partner" in DimerScreen.AnyPartner and EndPartner.
const DimerNone = 0xFFFFFFFF

// DimerParams is polyhip_dimer_params: the stack table (PrimerStackDG) and the two thresholds in cal/mol, both at most 0.
type DimerParams struct {
	StackDG                    [16]int32
	AnyThreshold, EndThreshold int32
}

// DimerInfo is polyhip_dimer_info: what the calling OS thread's last PrimerDimerMatrix / PrimerDimerScreen did.
type DimerInfo struct {
	Primers, Bad, Pairs, Shifts, Launches uint64
}

// DimerMatrix: DGAny and DGEnd are row-major len(ErrX) x len(ErrY) (nil for a plane that was not asked for), in cal/mol; ErrX
// and ErrY per primer (1 empty, 2 longer than 64 bytes).  In pool mode ErrY is ErrX.
type DimerMatrix struct {
	NX, NY       int
	DGAny, DGEnd []int32
	ErrX, ErrY   []uint32
}

// DimerScreen: one entry per primer of X.  The partner with the lowest energy over any run of pairs (DimerNone: none below 0),
// that energy and where the run sits; the same over the runs that hold x's 3' base; the partners at or below the thresholds.
type DimerScreen struct {
	AnyDG                                   []int32
	AnyPartner, AnyShift, AnyPos, AnyPairs  []uint32
	EndDG                                   []int32
	EndPartner, EndShift, EndPairs          []uint32
	AnyCount, EndCount                      []uint32
	ErrX, ErrY                              []uint32
}

// PrimerStackDG fills the stack table from the library's nearest-neighbour table at tempMK millikelvin (273150..338000).
func PrimerStackDG(tempMK uint32) ([16]int32, error) {
	var out [16]int32
	err := call(func() C.int { return C.polyhip_primer_stack_dg(C.uint32_t(tempMK), (*C.int32_t)(unsafe.Pointer(&out[0]))) })
	return out, err
}

// dimerSide is one packed set of primers as the C calls want it; the pointers of a missing Y stay nil (pool mode)
type dimerSide struct {
	bytes *C.uint8_t
	offs  *C.uint64_t
	err   *C.uint32_t
	n     int
	errs  []uint32
}

func newDimerSide(who string, seqs []byte, offs []uint64) (*dimerSide, error) {
	n := len(offs) - 1
	if n < 0 {
		return nil, fmt.Errorf("polyhip.%s: offsets hold one entry more than there are primers", who)
	}
	if offs[n] < offs[0] || uint64(len(seqs)) < offs[n] {
		return nil, fmt.Errorf("polyhip.%s: the offsets reach beyond the bytes", who)
	}
	if len(seqs) == 0 { // an empty set still needs &seqs[0]
		seqs = []byte{0}
	}
	s := &dimerSide{n: n, errs: make([]uint32, n+1)}
	s.bytes, s.offs = (*C.uint8_t)(unsafe.Pointer(&seqs[0])), (*C.uint64_t)(unsafe.Pointer(&offs[0]))
	s.err = (*C.uint32_t)(unsafe.Pointer(&s.errs[0]))
	return s, nil
}

// dimerSides: X, and Y when offsY is not nil; with offsY == nil the pool of X against itself
func dimerSides(who string, seqsX []byte, offsX []uint64, seqsY []byte, offsY []uint64) (*dimerSide, *dimerSide, error) {
	x, err := newDimerSide(who, seqsX, offsX)
	if err != nil {
		return nil, nil, err
	}
	if offsY == nil {
		return x, &dimerSide{}, nil
	}
	y, err := newDimerSide(who, seqsY, offsY)
	if err != nil {
		return nil, nil, err
	}
	if y.n == 0 {
		return nil, nil, fmt.Errorf("polyhip.%s: an empty Y (pass nil offsets for the pool against itself)", who)
	}
	return x, y, nil
}

// PrimerDimerMatrix fills the planes of every primer of X against every primer of Y (offsY == nil: of X).  At most 2^30 cells a
// call: the caller tiles.
func PrimerDimerMatrix(stackDG [16]int32, seqsX []byte, offsX []uint64, seqsY []byte, offsY []uint64, wantAny, wantEnd bool) (*DimerMatrix, error) {
	x, y, err := dimerSides("PrimerDimerMatrix", seqsX, offsX, seqsY, offsY)
	if err != nil {
		return nil, err
	}
	ny := y.n
	if offsY == nil {
		ny = x.n
	}
	res := &DimerMatrix{NX: x.n, NY: ny}
	var pAny, pEnd *C.int32_t
	if wantAny {
		res.DGAny = make([]int32, x.n*ny+1)
		pAny = (*C.int32_t)(unsafe.Pointer(&res.DGAny[0]))
	}
	if wantEnd {
		res.DGEnd = make([]int32, x.n*ny+1)
		pEnd = (*C.int32_t)(unsafe.Pointer(&res.DGEnd[0]))
	}
	err = call(func() C.int {
		return C.polyhip_primer_dimer_matrix((*C.int32_t)(unsafe.Pointer(&stackDG[0])), (*C.uint8_t)(unsafe.Pointer(x.bytes)),
			(*C.uint64_t)(unsafe.Pointer(x.offs)), C.uint64_t(x.n), (*C.uint8_t)(unsafe.Pointer(y.bytes)),
			(*C.uint64_t)(unsafe.Pointer(y.offs)), C.uint64_t(y.n), (*C.int32_t)(unsafe.Pointer(pAny)),
			(*C.int32_t)(unsafe.Pointer(pEnd)), (*C.uint32_t)(unsafe.Pointer(x.err)), (*C.uint32_t)(unsafe.Pointer(y.err)))
	})
	if err != nil {
		return nil, err
	}
	if wantAny {
		res.DGAny = res.DGAny[:x.n*ny]
	}
	if wantEnd {
		res.DGEnd = res.DGEnd[:x.n*ny]
	}
	res.ErrX = x.errs[:x.n]
	res.ErrY = res.ErrX
	if offsY != nil {
		res.ErrY = y.errs[:y.n]
	}
	return res, nil
}

// PrimerDimerScreen finds for every primer of X its worst partner in Y (offsY == nil: in X itself) and counts the partners at or
// below the thresholds, without ever holding len(X) x len(Y) values.
func PrimerDimerScreen(p DimerParams, seqsX []byte, offsX []uint64, seqsY []byte, offsY []uint64) (*DimerScreen, error) {
	x, y, err := dimerSides("PrimerDimerScreen", seqsX, offsX, seqsY, offsY)
	if err != nil {
		return nil, err
	}
	var cp C.polyhip_dimer_params
	for t := 0; t < 16; t++ {
		cp.stack_dg[t] = C.int32_t(p.StackDG[t])
	}
	cp.any_threshold, cp.end_threshold = C.int32_t(p.AnyThreshold), C.int32_t(p.EndThreshold)
	n := x.n
	u := func() []uint32 { return make([]uint32, n+1) }
	s := &DimerScreen{AnyDG: make([]int32, n+1), AnyPartner: u(), AnyShift: u(), AnyPos: u(), AnyPairs: u(), EndDG: make([]int32, n+1),
		EndPartner: u(), EndShift: u(), EndPairs: u(), AnyCount: u(), EndCount: u()}
	err = call(func() C.int {
		return C.polyhip_primer_dimer_screen((*C.polyhip_dimer_params)(unsafe.Pointer(&cp)), (*C.uint8_t)(unsafe.Pointer(x.bytes)),
			(*C.uint64_t)(unsafe.Pointer(x.offs)), C.uint64_t(x.n), (*C.uint8_t)(unsafe.Pointer(y.bytes)),
			(*C.uint64_t)(unsafe.Pointer(y.offs)), C.uint64_t(y.n), (*C.int32_t)(unsafe.Pointer(&s.AnyDG[0])),
			(*C.uint32_t)(unsafe.Pointer(&s.AnyPartner[0])), (*C.uint32_t)(unsafe.Pointer(&s.AnyShift[0])),
			(*C.uint32_t)(unsafe.Pointer(&s.AnyPos[0])), (*C.uint32_t)(unsafe.Pointer(&s.AnyPairs[0])),
			(*C.int32_t)(unsafe.Pointer(&s.EndDG[0])), (*C.uint32_t)(unsafe.Pointer(&s.EndPartner[0])),
			(*C.uint32_t)(unsafe.Pointer(&s.EndShift[0])), (*C.uint32_t)(unsafe.Pointer(&s.EndPairs[0])),
			(*C.uint32_t)(unsafe.Pointer(&s.AnyCount[0])), (*C.uint32_t)(unsafe.Pointer(&s.EndCount[0])),
			(*C.uint32_t)(unsafe.Pointer(x.err)), (*C.uint32_t)(unsafe.Pointer(y.err)))
	})
	if err != nil {
		return nil, err
	}
	s.AnyDG, s.EndDG = s.AnyDG[:n], s.EndDG[:n]
	s.AnyPartner, s.AnyShift, s.AnyPos, s.AnyPairs = s.AnyPartner[:n], s.AnyShift[:n], s.AnyPos[:n], s.AnyPairs[:n]
	s.EndPartner, s.EndShift, s.EndPairs = s.EndPartner[:n], s.EndShift[:n], s.EndPairs[:n]
	s.AnyCount, s.EndCount = s.AnyCount[:n], s.EndCount[:n]
	s.ErrX = x.errs[:n]
	s.ErrY = s.ErrX
	if offsY != nil {
		s.ErrY = y.errs[:y.n]
	}
	return s, nil
}

// LastDimerInfo must run on the OS thread that made the call (runtime.LockOSThread around both).
func LastDimerInfo() (DimerInfo, error) {
	var ci C.polyhip_dimer_info
	err := call(func() C.int { return C.polyhip_primer_dimer_last_info((*C.polyhip_dimer_info)(unsafe.Pointer(&ci))) })
	return DimerInfo{Primers: uint64(ci.primers), Bad: uint64(ci.bad), Pairs: uint64(ci.pairs), Shifts: uint64(ci.shifts),
		Launches: uint64(ci.launches)}, err
}
