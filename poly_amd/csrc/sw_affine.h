// sw_affine.h -- the affine-gap Smith-Waterman (sw_affine.hip) on device pointers, for callers inside the library: the
// score pass and the traceback ordered on the caller's stream with the caller's workspace, what sizes that workspace, and
// choose().  Nothing here is part of the C ABI (include/polyhip.h declares the host-pointer entry points only).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "sw_scoring.h"

namespace polyhip {
namespace k3a {

// columns of pair's traceback window: min(endB, W_p), W_p = endA + floor((smax * endA - s) / -ge); 0: nothing to trace
__host__ __device__ inline uint32_t window_cols(uint32_t eA, uint32_t eB, int64_t s, int smax, int ge)
{
    if (s < 1 || eA == 0 || eB == 0 || smax < 1)
        return 0;
    const uint64_t top = (uint64_t)smax * eA, g = (uint64_t)(-ge);
    const uint64_t W = eA + (top > (uint64_t)s ? (top - (uint64_t)s) / g : 0);
    return W < eB ? (uint32_t)W : eB;
}
// ... and the most bytes its strings can have: endA + min(endB, W_p - endA)
__host__ __device__ inline uint32_t string_bound(uint32_t eA, uint32_t eB, int64_t s, int smax, int ge)
{
    const uint32_t w = window_cols(eA, eB, s, smax, ge);
    if (w == 0)
        return 0;
    const uint64_t top = (uint64_t)smax * eA, g = (uint64_t)(-ge);
    const uint64_t left = top > (uint64_t)s ? (top - (uint64_t)s) / g : 0; // W_p - endA
    return eA + (uint32_t)(eB < left ? eB : left);
}

// What runs, and (choose) the only place that reads the testing aid
struct Choice {
    int rb;               // rows per band of the kernels
    bool lds;             // the compact table is staged in LDS
    size_t smem;          // dynamic LDS per workgroup
    unsigned max_blocks;  // workgroups of the persistent grids
    uint64_t chunk_pairs; // the traceback's chunks: most pairs per chunk (POLYHIP_SWA_CHUNK_PAIRS)
    uint64_t dir_cap;     // ... and most bytes of direction words per chunk
    uint64_t slot_cap;    // ... and most bytes of one side's string slots per chunk
    uint64_t band_cap;    // most bytes of band scratch (fewer workgroups beyond)
};
Choice choose(const polyhip_scoring *sc, int cus);

// ---- sizes of the caller's workspace
// workgroups of a persistent grid over npairs pairs whose band scratch holds `cols` columns per wave, and that scratch
unsigned grid_blocks(const Choice &c, uint64_t npairs, uint64_t cols);
size_t band_bytes(unsigned blocks, uint64_t cols);
// words of direction bits of a window of eA rows and ncol columns, a multiple of 4; with (max lenA, max lenB) the most any
// pair of a batch needs, whatever its score
uint64_t dir_words(uint32_t eA, uint32_t ncol);
// bytes of a string slot that holds any pair's strings: string_bound never exceeds lenA + lenB
inline uint32_t slot_stride(uint32_t max_lenA, uint32_t max_lenB) { return std::max<uint32_t>(max_lenA + max_lenB, 1); }

// The score pass on device pointers: d_band holds band_bytes(blocks, lenB) bytes.  lenB: the shared B's length (d_offB ==
// nullptr), or the longest B of the batch.  Cells are int32: the caller has checked absmax * (lenA + lenB) < 2^30.
int score_pass(const polyhip_scoring *sc, const Choice &c, int go, int ge, const uint8_t *d_A, const uint64_t *d_offA,
               uint64_t npairs, const uint8_t *d_B, const uint64_t *d_offB, uint32_t lenB, int64_t *d_score, uint32_t *d_endA,
               uint32_t *d_endB, uint32_t *d_err, void *d_band, unsigned blocks, hipStream_t st);

// The traceback of pairs [0, npairs) (a chunk: every pointer is the chunk's own) from the score pass's outputs:
// d_dirOff[p] = where pair p's dir_words(endA, window_cols) words start in d_dir (a multiple of 4); d_band holds
// band_bytes(blocks, max_cols) bytes, max_cols = the chunk's widest window; the strings go right-aligned into stride-byte
// slots (stride >= the pairs' string_bound), their lengths to d_alnLen.
int traceback_pass(const polyhip_scoring *sc, const Choice &c, int go, int ge, const uint8_t *d_A, const uint64_t *d_offA,
                   uint64_t npairs, const uint8_t *d_B, const uint64_t *d_offB, uint32_t lenB, const int64_t *d_score,
                   const uint32_t *d_endA, const uint32_t *d_endB, const uint32_t *d_err, const uint64_t *d_dirOff,
                   uint32_t *d_dir, void *d_band, uint32_t max_cols, unsigned blocks, uint8_t *d_alnA, uint8_t *d_alnB,
                   uint32_t *d_alnLen, uint32_t stride, hipStream_t st);

} // namespace k3a
} // namespace polyhip
