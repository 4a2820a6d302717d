// cgo binding of the K2 neighbour-list entry points of libpolyhip.so (include/polyhip.h, "K2 neighbour lists").
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

// NeighborsInfo is polyhip_neighbors_info: what the calling OS thread's last MashNeighbors did.
type NeighborsInfo struct {
	ColumnBlocks, IndexBuilds, RowChunks, Assembly int
	EntriesThresholded, Entries                    uint64
	Devices                                        int
}

// MashNeighbors: X is nx*sx, Y is ny*sy.  Row i of the list is cols/shared/dist[first[i]:first[i+1]]: every j with at least
// minShared shared hashes (not j == i+selfOffset if excludeSelf), the k best of them if k > 0.  first is nx+1 long and
// always carries the true counts; cols, shared and dist (nil: not wanted) hold `capacity` entries and nothing is written
// beyond them, so a caller whose first[nx] exceeds its capacity resizes and calls again.
func MashNeighbors(X []uint32, nx, sx int, Y []uint32, ny, sy int, minShared, k int, excludeSelf bool, selfOffset int,
	first []uint64, cols []uint32, shared []uint16, dist []float64, capacity int) error {
	var pc *C.uint32_t
	var ps *C.uint16_t
	var pd *C.double
	if capacity > 0 && cols != nil {
		pc = (*C.uint32_t)(unsafe.Pointer(&cols[0]))
		ps = (*C.uint16_t)(unsafe.Pointer(&shared[0]))
		if dist != nil {
			pd = (*C.double)(unsafe.Pointer(&dist[0]))
		}
	}
	// nx == 0 or ny == 0 is the empty list (the library reads neither X nor Y then); an empty slice has no &s[0]
	var px *C.uint32_t
	var py *C.uint32_t
	if len(X) > 0 {
		px = (*C.uint32_t)(unsafe.Pointer(&X[0]))
	}
	if len(Y) > 0 {
		py = (*C.uint32_t)(unsafe.Pointer(&Y[0]))
	}
	if len(first) < nx+1 {
		return fmt.Errorf("polyhip.MashNeighbors: first holds %d values, nx+1 = %d are written", len(first), nx+1)
	}
	ex := 0
	if excludeSelf {
		ex = 1
	}
	return call(func() C.int {
		return C.polyhip_mash_neighbors(px, C.uint64_t(nx), C.uint32_t(sx), py, C.uint64_t(ny), C.uint32_t(sy), C.uint32_t(minShared), C.uint32_t(k),
			C.int(ex), C.uint64_t(selfOffset), (*C.uint64_t)(unsafe.Pointer(&first[0])), pc, ps, pd, C.uint64_t(capacity))
	})
}

// LastNeighborsInfo must run on the OS thread that made the call (runtime.LockOSThread around both).
func LastNeighborsInfo() (NeighborsInfo, error) {
	var ci C.polyhip_neighbors_info
	err := call(func() C.int { return C.polyhip_mash_neighbors_last_info((*C.polyhip_neighbors_info)(unsafe.Pointer(&ci))) })
	return NeighborsInfo{ColumnBlocks: int(ci.column_blocks), IndexBuilds: int(ci.index_builds), RowChunks: int(ci.row_chunks),
		Assembly: int(ci.assembly), EntriesThresholded: uint64(ci.entries_thresholded), Entries: uint64(ci.entries),
		Devices: int(ci.devices)}, err
}
