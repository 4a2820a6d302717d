// bwt_index.h -- what the FM-index (bwt.hip) and the read mapper (map_reads.hip) share: the index handle and its occurrence
// functions, the exclusive scans and the LSD radix sort of (uint64 key, uint32 value).  Kernels and helpers sit in an
// anonymous namespace: every translation unit that includes this header gets its own copies.
#pragma once
#include <algorithm>
#include <cstring>

#include "common.h"

namespace polyhip {

// ---- the index as the query kernels see it ------------------------------------------------------------------------------
struct Index {
    int layout;            // 0 nucleotide, 1 general
    uint32_t N;            // n + 1
    uint32_t primary;      // the row whose L is '$'
    uint32_t sigma;        // distinct bytes of the sequence
    const uint8_t *dense;  // [256] byte -> code 0..sigma-1, 0xFF absent
    const uint32_t *C;     // [256] by code: 1 + rows of smaller symbols ('$' is row 0)
    const uint4 *lines;    // nucleotide
    const uint8_t *L;      // general: L bytes, padded to whole blocks
    const uint32_t *cp;    // general checkpoints
};

namespace {

constexpr int BT = 256;           // threads per block everywhere in this file
constexpr int ITEMS = 16;         // items per thread of a scan / radix tile
constexpr int TILE = BT * ITEMS;  // 4096
constexpr int NUC_SYMS = 448;     // 2-bit symbols per 128-byte line (16 bytes of counts + 112 bytes of symbols)
constexpr int GEN_ROWS = 64;      // rows per checkpoint of the general layout
constexpr uint8_t NULL_CHAR = '$';

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

template <class T> __global__ __launch_bounds__(BT) void scan_reduce_kernel(const T *__restrict__ in, uint64_t m, T *__restrict__ sums)
{
    const uint64_t base = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * ITEMS;
    T s = 0;
#pragma unroll
    for (int q = 0; q < ITEMS; ++q)
        if (base + q < m)
            s += in[base + q];
    T total;
    (void)block_excl_scan<T>(s, total);
    if (threadIdx.x == 0)
        sums[blockIdx.x] = total;
}

// offs == nullptr: a single block, offset 0
template <class T>
__global__ __launch_bounds__(BT) void scan_apply_kernel(const T *in, T *out, uint64_t m, const T *__restrict__ offs)
{
    const uint64_t base = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * ITEMS;
    T v[ITEMS];
    T s = 0;
#pragma unroll
    for (int q = 0; q < ITEMS; ++q) {
        v[q] = base + q < m ? in[base + q] : T(0);
        s += v[q];
    }
    T total;
    T run = block_excl_scan<T>(s, total) + (offs ? offs[blockIdx.x] : T(0));
#pragma unroll
    for (int q = 0; q < ITEMS; ++q)
        if (base + q < m) {
            out[base + q] = run;
            run += v[q];
        }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == BT - 1)
        out[m] = run;
}

template <class T> size_t scan_scratch_bytes(uint64_t m)
{
    if (m <= (uint64_t)TILE)
        return 0;
    const uint64_t nb = (m + TILE - 1) / TILE;
    return align256((nb + 1) * sizeof(T)) + scan_scratch_bytes<T>(nb);
}

template <class T> hipError_t scan_excl(const T *in, T *out, uint64_t m, uint8_t *scratch, hipStream_t st)
{
    if (m == 0)
        return hipMemsetAsync(out, 0, sizeof(T), st);
    const uint64_t nb = (m + TILE - 1) / TILE;
    if (nb == 1) {
        hipLaunchKernelGGL(scan_apply_kernel<T>, dim3(1), dim3(BT), 0, st, in, out, m, (const T *)nullptr);
        return hipGetLastError();
    }
    T *sums = reinterpret_cast<T *>(scratch);
    hipLaunchKernelGGL(scan_reduce_kernel<T>, dim3((unsigned)nb), dim3(BT), 0, st, in, m, sums);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = scan_excl<T>(sums, sums, nb, scratch + align256((nb + 1) * sizeof(T)), st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(scan_apply_kernel<T>, dim3((unsigned)nb), dim3(BT), 0, st, in, out, m, (const T *)sums);
    return hipGetLastError();
}

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

// hist[d * nblocks + block] = items of the block's tile with digit d
__global__ __launch_bounds__(BT) void radix_hist_kernel(const uint64_t *__restrict__ keys, uint64_t n, int shift,
                                                        uint32_t *__restrict__ hist, uint32_t nblocks)
{
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t tile0 = (uint64_t)blockIdx.x * TILE;
    for (int it = 0; it < ITEMS; ++it) {
        const uint64_t i = tile0 + (uint64_t)it * BT + threadIdx.x;
        const bool valid = i < n;
        const uint32_t d = valid ? (uint32_t)(keys[i] >> shift) & 255u : 0u;
        const uint64_t m = same_digit_lanes(d, valid);
        if (valid && (m & ((1ull << lane) - 1)) == 0)
            atomicAdd(&cnt[d], (uint32_t)__popcll(m));
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * nblocks + blockIdx.x] = cnt[threadIdx.x];
}

// base = the exclusive scan of hist: every item goes to base[digit][block] + (items of that digit before it in the tile)
__global__ __launch_bounds__(BT) void radix_scatter_kernel(const uint64_t *__restrict__ kin, const uint32_t *__restrict__ vin,
                                                           uint64_t *__restrict__ kout, uint32_t *__restrict__ vout, uint64_t n,
                                                           int shift, const uint32_t *__restrict__ base, uint32_t nblocks)
{
    __shared__ uint32_t run[256];
    __shared__ uint32_t wcnt[BT / 64][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    run[threadIdx.x] = base[(uint64_t)threadIdx.x * nblocks + blockIdx.x];
#pragma unroll
    for (int q = 0; q < BT / 64; ++q)
        wcnt[q][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t tile0 = (uint64_t)blockIdx.x * TILE;
    for (int it = 0; it < ITEMS; ++it) {
        const uint64_t i = tile0 + (uint64_t)it * BT + threadIdx.x;
        const bool valid = i < n;
        const uint64_t k = valid ? kin[i] : 0;
        const uint32_t d = (uint32_t)(k >> shift) & 255u;
        const uint64_t m = same_digit_lanes(d, valid);
        const uint64_t below = m & ((1ull << lane) - 1);
        if (valid && below == 0)
            wcnt[w][d] = (uint32_t)__popcll(m);
        __syncthreads();
        if (valid) {
            uint32_t pos = run[d] + (uint32_t)__popcll(below);
            for (int q = 0; q < w; ++q)
                pos += wcnt[q][d];
            kout[pos] = k;
            vout[pos] = vin[i];
        }
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (int q = 0; q < BT / 64; ++q) {
            add += wcnt[q][threadIdx.x];
            wcnt[q][threadIdx.x] = 0;
        }
        run[threadIdx.x] += add;
        __syncthreads();
    }
}

// ---- occurrences: rows [0, i) of L that hold a symbol --------------------------------------------------------------------
__device__ __forceinline__ uint32_t occ_nuc(const Index &x, uint32_t c, uint32_t i)
{
    const uint32_t line = i / NUC_SYMS, off = i - line * NUC_SYMS;
    const uint4 *p = x.lines + (uint64_t)line * 8;
    const uint4 head = p[0];
    uint32_t r = c == 0 ? head.x : c == 1 ? head.y : c == 2 ? head.z : head.w;
    const uint64_t pat = 0x5555555555555555ull * c;
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        if (off <= 64u * q)
            break;
        const uint4 v = p[1 + q];
        const uint64_t wd[2] = {(uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32)};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int first = 64 * q + 32 * h;
            if ((int)off <= first)
                break;
            const int take = min((int)off - first, 32);
            const uint64_t y = ~(wd[h] ^ pat);
            uint64_t m = y & (y >> 1) & 0x5555555555555555ull;
            if (take < 32)
                m &= (1ull << (2 * take)) - 1;
            r += (uint32_t)__popcll(m);
        }
    }
    if (c == 0 && x.primary >= line * NUC_SYMS && x.primary < i)
        r -= 1; // the '$' slot holds code 0 and is no base
    return r;
}

// the occurrences of all four codes in rows [0, i) from one pass over the line's words (x: code 0 .. w: code 3); what a
// search that branches on every symbol needs per range end (bwt_mismatch.hip).  Each component equals occ_nuc's.
__device__ __forceinline__ uint4 occ_nuc4(const Index &x, uint32_t i)
{
    const uint32_t line = i / NUC_SYMS, off = i - line * NUC_SYMS;
    const uint4 *p = x.lines + (uint64_t)line * 8;
    uint4 r = p[0];
    constexpr uint64_t LOW = 0x5555555555555555ull;
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        if (off <= 64u * q)
            break;
        const uint4 v = p[1 + q];
        const uint64_t wd[2] = {(uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32)};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int first = 64 * q + 32 * h;
            if ((int)off <= first)
                break;
            const int take = min((int)off - first, 32);
            const uint64_t keep = take < 32 ? LOW & ((1ull << (2 * take)) - 1) : LOW;
            const uint64_t lo = wd[h] & keep, hi = (wd[h] >> 1) & keep;
            const uint32_t n1 = (uint32_t)__popcll(lo & ~hi), n2 = (uint32_t)__popcll(hi & ~lo), n3 = (uint32_t)__popcll(hi & lo);
            r.x += (uint32_t)take - n1 - n2 - n3;
            r.y += n1;
            r.z += n2;
            r.w += n3;
        }
    }
    if (x.primary >= line * NUC_SYMS && x.primary < i)
        r.x -= 1; // the '$' slot holds code 0 and is no base
    return r;
}

__device__ __forceinline__ uint32_t occ_gen(const Index &x, uint32_t c, uint8_t b, uint32_t i)
{
    const uint32_t blk = i / GEN_ROWS, off = i - blk * GEN_ROWS;
    uint32_t r = x.cp[(uint64_t)blk * x.sigma + c];
    const uint4 *p = reinterpret_cast<const uint4 *>(x.L + (uint64_t)blk * GEN_ROWS);
    const uint64_t rep = 0x0101010101010101ull * b;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (off <= 16u * q)
            break;
        const uint4 v = p[q];
        const uint64_t wd[2] = {(uint64_t)v.x | ((uint64_t)v.y << 32), (uint64_t)v.z | ((uint64_t)v.w << 32)};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int first = 16 * q + 8 * h;
            if ((int)off <= first)
                break;
            const int take = min((int)off - first, 8);
            const uint64_t z = wd[h] ^ rep; // zero bytes = matches
            uint64_t zb = ~(((z & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | z) & 0x8080808080808080ull;
            if (take < 8)
                zb &= (1ull << (8 * take)) - 1;
            r += (uint32_t)__popcll(zb);
        }
    }
    return r;
}

unsigned grid_for(uint64_t items, uint64_t per_block = BT)
{
    uint64_t g = (items + per_block - 1) / per_block;
    if (g < 1)
        g = 1;
    if (g > 256 * 64)
        g = 256 * 64;
    return (unsigned)g;
}

int bits_for(uint64_t v) // bits needed to hold 0..v
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

uint64_t radix_blocks(uint64_t N) { return (N + TILE - 1) / TILE; }

} // namespace

// ---- the handle --------------------------------------------------------------------------------------------------------
struct BwtHandle {
    int dev = 0;
    hipStream_t stream = nullptr; // the host-pointer calls' stream
    uint64_t n = 0;
    Index x{};
    uint8_t *d_text = nullptr;  // T, N bytes
    uint32_t *d_sa = nullptr;   // N
    uint8_t *d_L = nullptr;     // L bytes padded to whole blocks / lines
    uint8_t *d_tables = nullptr; // dense[256] + C[256]
    uint4 *d_lines = nullptr;   // nucleotide
    uint32_t *d_cp = nullptr;   // general
    int rounds = 0;
    ~BwtHandle()
    {
        for (void *q : {(void *)d_text, (void *)d_sa, (void *)d_L, (void *)d_tables, (void *)d_lines, (void *)d_cp})
            if (q)
                (void)hipFree(q);
        if (stream)
            (void)hipStreamDestroy(stream);
    }
};

// A reference set (refs.hip; the mapper's refs calls read it): k contigs concatenated into the text of `index`, which the
// set owns.  start[c] = where contig c begins in that text, start[k] = its length.
struct RefsHandle {
    polyhip_bwt *index = nullptr;
    uint32_t k = 0;
    uint32_t nmax = 0;           // the longest contig
    uint32_t *d_start = nullptr; // k + 1, on the index's device
    uint64_t *starts = nullptr;  // the same on the host, as polyhip_refs_starts returns them
};

namespace {

const RefsHandle *as_refs(const polyhip_refs *h) { return reinterpret_cast<const RefsHandle *>(h); }

// the calling thread runs a bwt call on the handle's device and gets its own device back afterwards
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

int radix_sort(uint64_t *&ka, uint32_t *&va, uint64_t *&kb, uint32_t *&vb, uint64_t N, int bits, uint32_t *hist, uint8_t *scratch,
               hipStream_t st)
{
    const uint64_t nb = radix_blocks(N);
    for (int shift = 0; shift < bits; shift += 8) {
        hipLaunchKernelGGL(radix_hist_kernel, dim3((unsigned)nb), dim3(BT), 0, st, ka, N, shift, hist, (uint32_t)nb);
        PH_HIP(hipGetLastError());
        PH_HIP(scan_excl<uint32_t>(hist, hist, 256 * nb, scratch, st));
        hipLaunchKernelGGL(radix_scatter_kernel, dim3((unsigned)nb), dim3(BT), 0, st, ka, va, kb, vb, N, shift, hist, (uint32_t)nb);
        PH_HIP(hipGetLastError());
        std::swap(ka, kb);
        std::swap(va, vb);
    }
    return POLYHIP_OK;
}

const BwtHandle *as_h(const polyhip_bwt *h) { return reinterpret_cast<const BwtHandle *>(h); }

} // namespace
} // namespace polyhip
