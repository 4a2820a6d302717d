// bwt_index.h -- the FM-index as its users see it (bwt.hip builds it; bwt_mismatch.hip, map_reads.hip and refs.hip read it):
// the index handle and the reference-set handle, the index as the query kernels get it, and its occurrence functions, which
// are inlined into the kernels of the unit that calls them.
#pragma once
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

constexpr int NUC_SYMS = 448;     // 2-bit symbols per 128-byte line (16 bytes of counts + 112 bytes of symbols)
constexpr int GEN_ROWS = 64;      // rows per checkpoint of the general layout
constexpr uint8_t NULL_CHAR = '$';

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

inline const BwtHandle *as_h(const polyhip_bwt *h) { return reinterpret_cast<const BwtHandle *>(h); }
inline const RefsHandle *as_refs(const polyhip_refs *h) { return reinterpret_cast<const RefsHandle *>(h); }

} // namespace polyhip
