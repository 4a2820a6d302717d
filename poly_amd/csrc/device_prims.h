// device_prims.h -- general device primitives of the string units (bwt.hip, bwt_mismatch.hip, map_reads.hip, refs.hip,
// aln_records.hip, pileup.hip, pileup_walk.hip, pileup_rows.hip, variants.hip): the exclusive scans and the LSD radix sort
// of (uint64 key, uint32 value), the wave and block helpers their own kernels call, and the host helpers around a launch
// (grids, workspaces, the device of a handle).
// scan_excl and radix_sort are compiled once, in device_prims.hip: the library is built without relocatable device code, so
// a kernel is launched from the unit that defines it.  Everything else here is inline.
#pragma once
#include <algorithm>

#include "common.h"

namespace polyhip {

constexpr int BT = 256;           // threads per block everywhere in these units
constexpr int ITEMS = 16;         // items per thread of a scan / radix tile
constexpr int TILE = BT * ITEMS;  // 4096

constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- exclusive scan (uint32 or uint64), three phases, recursive over the block sums ------------------------------------
// out[0..M] = exclusive prefix sums of in[0..M), out[M] = the total; in == out is allowed (out then has M + 1 slots).
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) { return dpp_incl_scan(v); }
__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t u = __shfl_up(v, d, 64);
        if (lane >= d)
            v += u;
    }
    return v;
}

// exclusive prefix of `v` over the block, and the block's total
template <class T> __device__ __forceinline__ T block_excl_scan(T v, T &total)
{
    __shared__ T wsum[BT / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T inc = wave_incl_scan(v);
    if (lane == 63)
        wsum[w] = inc;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < BT / 64; ++q) {
        before += q < w ? wsum[q] : T(0);
        all += wsum[q];
    }
    __syncthreads();
    total = all;
    return before + inc - v;
}

template <class T> size_t scan_scratch_bytes(uint64_t m)
{
    if (m <= (uint64_t)TILE)
        return 0;
    const uint64_t nb = (m + TILE - 1) / TILE;
    return align256((nb + 1) * sizeof(T)) + scan_scratch_bytes<T>(nb);
}

template <class T> hipError_t scan_excl(const T *in, T *out, uint64_t m, uint8_t *scratch, hipStream_t st);
extern template hipError_t scan_excl<uint32_t>(const uint32_t *, uint32_t *, uint64_t, uint8_t *, hipStream_t);
extern template hipError_t scan_excl<uint64_t>(const uint64_t *, uint64_t *, uint64_t, uint8_t *, hipStream_t);

// ---- LSD radix sort of (uint64 key, uint32 value), 8 bits per pass, stable ---------------------------------------------
// Lanes of one wave holding the same digit: eight ballots (no LDS atomics on a skewed digit, e.g. a one-symbol text).
__device__ __forceinline__ uint64_t same_digit_lanes(uint32_t d, bool valid)
{
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t v = __ballot(bit);
        m &= bit ? v : ~v;
    }
    return m;
}

inline uint64_t radix_blocks(uint64_t N) { return (N + TILE - 1) / TILE; }

// sorts by the low `bits` bits of the keys; the sorted arrays are the ones ka / va name afterwards (the pairs swap every
// pass).  hist: 256 * radix_blocks(N) + 1 uint32; scratch: scan_scratch_bytes<uint32_t>(256 * radix_blocks(N))
int radix_sort(uint64_t *&ka, uint32_t *&va, uint64_t *&kb, uint32_t *&vb, uint64_t N, int bits, uint32_t *hist, uint8_t *scratch,
               hipStream_t st);

// ---- masks of a wave's lanes ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ int top_bit(uint64_t m) { return 63 - __clzll((long long)m); } // m != 0

// ---- host helpers --------------------------------------------------------------------------------------------------------
inline unsigned grid_for(uint64_t items, uint64_t per_block = BT, uint64_t cap = 256 * 64)
{
    uint64_t g = (items + per_block - 1) / per_block;
    if (g < 1)
        g = 1;
    if (g > cap)
        g = cap;
    return (unsigned)g;
}

inline int bits_for(uint64_t v) // bits needed to hold 0..v
{
    int b = 1;
    while (b < 64 && (v >> b))
        ++b;
    return b;
}

// a workspace carved in order
struct Carve {
    uint8_t *p;
    size_t used = 0;
    template <class T> T *take(uint64_t count)
    {
        T *r = reinterpret_cast<T *>(p ? p + used : nullptr);
        used += align256(count * sizeof(T));
        return r;
    }
};

// one device allocation, carved in 256-byte steps
struct Arena {
    DevBuf buf;
    size_t used = 0;
    size_t reserve(size_t bytes)
    {
        const size_t at = used;
        used += align256(bytes ? bytes : 1);
        return at;
    }
    template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(buf.as<uint8_t>() + off); }
};

// the calling thread runs a call on a handle's device and gets its own device back afterwards
struct DeviceScope {
    int prev = -1;
    hipError_t enter(int dev)
    {
        hipError_t e = hipGetDevice(&prev);
        if (e == hipSuccess && prev != dev)
            e = hipSetDevice(dev);
        else
            prev = -1;
        return e;
    }
    ~DeviceScope()
    {
        if (prev >= 0)
            (void)hipSetDevice(prev);
    }
};

} // namespace polyhip
