// pileup_walk.h -- the entry walks of polyhip_pileup (pileup.hip) and polyhip_pileup_qual (pileup_qual.hip), in a header since
// polyhip_pileup_rows (pileup_rows.hip) judges its entries with the same two: walk_kernel<false> without qualities,
// walk_qual_kernel<false> with them.  The kernels are the text those units held, unchanged; each unit compiles the
// instantiations it launches (internal linkage, as pileup_call.h).
#pragma once
#include "device_prims.h"
#include "pileup_call.h"

namespace polyhip {
namespace {

// ADD == false: err[i] is written, info[USED, SKIPPED, BAD, COLUMNS] are added to, counts is not touched.
// ADD == true: err[i] is read, the used entries add to counts, info[EDGE] is added to.
template <bool ADD>
__global__ __launch_bounds__(BT) void walk_kernel(uint64_t n, uint32_t min_mapq, uint64_t lo, uint64_t L, uint64_t ref_len,
                                                  const uint32_t *__restrict__ flags, const uint8_t *__restrict__ mapq,
                                                  const uint32_t *__restrict__ ref_start, const uint32_t *__restrict__ ref_end,
                                                  const uint8_t *__restrict__ alnA, const uint8_t *__restrict__ alnB,
                                                  const uint64_t *__restrict__ alnOff, const uint8_t *__restrict__ ref, uint32_t *err,
                                                  uint32_t *counts, unsigned long long *info)
{
    const int lane = threadIdx.x & 63;
    const uint64_t off0 = n ? alnOff[0] : 0; // the device copy of the strings starts at the first entry's columns
    uint64_t n_used = 0, n_skipped = 0, n_bad = 0, n_cols = 0, n_edge = 0; // of this wave's entries, the same in every lane
    for (uint64_t i = (uint64_t)blockIdx.x * PU_WAVES + (threadIdx.x >> 6); i < n; i += (uint64_t)gridDim.x * PU_WAVES) {
        const uint32_t f = flags[i];
        const bool mapped = f & 1u;
        const bool skipped = mapped && min_mapq > 0 && mapq[i] < min_mapq; // min_mapq > 0 comes with a mapq array
        const uint64_t ncol = alnOff[i + 1] - alnOff[i];
        if (!ADD && (!mapped || skipped || ncol > POLYHIP_ALN_MAX_COLUMNS)) {
            const uint32_t e = mapped && !skipped ? 4u : 0u;
            if (lane == 0)
                err[i] = e;
            n_skipped += skipped ? 1u : 0u;
            n_bad += e ? 1u : 0u;
            continue;
        }
        if (ADD && (!mapped || skipped || err[i] != 0))
            continue;
        const uint32_t ncols = (uint32_t)ncol;
        const uint64_t rs = ref_start[i];
        const uint8_t *a = alnA + (alnOff[i] - off0), *b = alnB + (alnOff[i] - off0);
        const uint32_t strand = f & 2u ? CH_STRAND : 0u;
        uint64_t tbase = rs;   // text position of the next column with b != '-'
        uint32_t carry = 0;    // the column before this step: bit 0 it was I, bit 1 it was D
        bool invalid = false, differs = false;
        for (uint32_t base = 0; base < ncols; base += 64) {
            const uint32_t c = base + lane;
            const bool v = c < ncols;
            const uint32_t ca = v ? a[c] : 0u, cb = v ? b[c] : 0u;
            const bool ga = ca == '-', gb = cb == '-';
            const uint64_t mV = __ballot(v);
            if (!ADD && __ballot(v && ga && gb)) {
                invalid = true;
                break;
            }
            const uint64_t mD = __ballot(v && ga), mI = __ballot(v && gb), mT = mV & ~mI;
            // a column with b != '-' sits at p; a run that starts at this lane is anchored at p - 1
            const uint64_t p = tbase + (uint64_t)__popcll(mT & lanes_below(lane));
            if (!ADD) {
                if (__ballot(v && !gb && (p >= ref_len || cb != ref[p])))
                    differs = true;
            } else {
                const uint64_t sI = mI & ~(mI << 1 | (carry & 1u)), sD = mD & ~(mD << 1 | (carry >> 1 & 1u));
                bool edge = false;
                if (v && !gb && p - lo < L) // p < lo wraps to a value above L
                    atomicAdd(&counts[(strand + (ga ? (uint32_t)CH_DEL : base_class(ca))) * L + (p - lo)], 1u);
                if ((sI | sD) >> lane & 1ull) {
                    if (p == 0)
                        edge = true;
                    else if (p - 1 - lo < L)
                        atomicAdd(&counts[(strand + (gb ? (uint32_t)CH_INS_EVENT : (uint32_t)CH_DEL_EVENT)) * L + (p - 1 - lo)], 1u);
                }
                n_edge += (uint64_t)__popcll(__ballot(edge));
            }
            const int nv = __popcll(mV);
            carry = (uint32_t)(mI >> (nv - 1) & 1ull) | (uint32_t)(mD >> (nv - 1) & 1ull) << 1;
            tbase += (uint64_t)__popcll(mT);
        }
        if (!ADD) {
            const uint64_t re = ref_end[i];
            const uint32_t e = invalid ? 1u : (tbase != re || re > ref_len) ? 2u : ncols == 0 ? 3u : differs ? 5u : 0u;
            if (lane == 0)
                err[i] = e;
            n_bad += e ? 1u : 0u;
            n_used += e ? 0u : 1u;
            n_cols += e ? 0u : ncol;
        }
    }
    if (lane == 0) {
        if (n_used) {
            atomicAdd(&info[INFO_USED], (unsigned long long)n_used);
            atomicAdd(&info[INFO_COLUMNS], (unsigned long long)n_cols);
        }
        if (n_skipped)
            atomicAdd(&info[INFO_SKIPPED], (unsigned long long)n_skipped);
        if (n_bad)
            atomicAdd(&info[INFO_BAD], (unsigned long long)n_bad);
        if (n_edge)
            atomicAdd(&info[INFO_EDGE], (unsigned long long)n_edge);
    }
}

enum : int { QINFO_FILTERED = INFO_WORDS, QINFO_WORDS };
constexpr uint32_t MAX_Q = 93;

// ADD == false: err[i] is written, info[USED, SKIPPED, BAD, COLUMNS] are added to, counts and qsum are not touched.
// ADD == true: err[i] is read, the used entries add to counts and qsum, info[EDGE, FILTERED] are added to.
template <bool ADD>
__global__ __launch_bounds__(BT) void walk_qual_kernel(uint64_t n, uint32_t min_mapq, uint32_t min_q, uint32_t qbase, uint64_t lo, uint64_t L,
                                                       uint64_t ref_len, const uint32_t *__restrict__ flags, const uint8_t *__restrict__ mapq,
                                                       const uint32_t *__restrict__ ref_start, const uint32_t *__restrict__ ref_end,
                                                       const uint32_t *__restrict__ read_start, const uint8_t *__restrict__ alnA,
                                                       const uint8_t *__restrict__ alnB, const uint64_t *__restrict__ alnOff,
                                                       const uint8_t *__restrict__ qual, const uint64_t *__restrict__ qualOff,
                                                       const uint8_t *__restrict__ ref, uint32_t *err, uint32_t *counts, uint32_t *qsum,
                                                       unsigned long long *info)
{
    const int lane = threadIdx.x & 63;
    const uint64_t off0 = n ? alnOff[0] : 0, qoff0 = n ? qualOff[0] : 0; // the device copies start at the first entry's bytes
    uint64_t n_used = 0, n_skipped = 0, n_bad = 0, n_cols = 0, n_edge = 0, n_filtered = 0; // of this wave's entries, the same in every lane
    for (uint64_t i = (uint64_t)blockIdx.x * PU_WAVES + (threadIdx.x >> 6); i < n; i += (uint64_t)gridDim.x * PU_WAVES) {
        const uint32_t f = flags[i];
        const bool mapped = f & 1u;
        const bool skipped = mapped && min_mapq > 0 && mapq[i] < min_mapq; // min_mapq > 0 comes with a mapq array
        const uint64_t ncol = alnOff[i + 1] - alnOff[i];
        if (!ADD && (!mapped || skipped || ncol > POLYHIP_ALN_MAX_COLUMNS)) {
            const uint32_t e = mapped && !skipped ? 4u : 0u;
            if (lane == 0)
                err[i] = e;
            n_skipped += skipped ? 1u : 0u;
            n_bad += e ? 1u : 0u;
            continue;
        }
        if (ADD && (!mapped || skipped || err[i] != 0))
            continue;
        const uint32_t ncols = (uint32_t)ncol;
        const uint64_t rs = ref_start[i];
        const uint8_t *a = alnA + (alnOff[i] - off0), *b = alnB + (alnOff[i] - off0);
        const uint8_t *q = qual + (qualOff[i] - qoff0);
        const uint64_t m = qualOff[i + 1] - qualOff[i];
        const bool reverse = f & 2u;
        const uint32_t strand = reverse ? CH_STRAND : 0u;
        uint64_t tbase = rs;            // text position of the next column with b != '-'
        uint64_t abase = read_start[i]; // index in the oriented read of the next column with a != '-'
        uint32_t carry = 0;             // the column before this step: bit 0 it was I, bit 1 it was D
        bool invalid = false, differs = false;
        for (uint32_t base = 0; base < ncols; base += 64) {
            const uint32_t c = base + lane;
            const bool v = c < ncols;
            const uint32_t ca = v ? a[c] : 0u, cb = v ? b[c] : 0u;
            const bool ga = ca == '-', gb = cb == '-';
            const uint64_t mV = __ballot(v);
            if (!ADD && __ballot(v && ga && gb)) {
                invalid = true;
                break;
            }
            const uint64_t mD = __ballot(v && ga), mI = __ballot(v && gb), mT = mV & ~mI, mA = mV & ~mD;
            // a column with b != '-' sits at p; a run that starts at this lane is anchored at p - 1
            const uint64_t p = tbase + (uint64_t)__popcll(mT & lanes_below(lane));
            if (!ADD) {
                if (__ballot(v && !gb && (p >= ref_len || cb != ref[p])))
                    differs = true;
            } else {
                const uint64_t sI = mI & ~(mI << 1 | (carry & 1u)), sD = mD & ~(mD << 1 | (carry >> 1 & 1u));
                const bool is_base = v && !ga && !gb;
                bool edge = false, low = false;
                if (is_base) { // err[i] == 0: x < m, the byte is inside the entry's string and in qbase .. qbase + 93
                    const uint64_t x = abase + (uint64_t)__popcll(mA & lanes_below(lane));
                    const uint32_t Q = (uint32_t)q[reverse ? m - 1 - x : x] - qbase;
                    low = Q < min_q;
                    if (!low && p - lo < L) { // p < lo wraps to a value above L
                        const uint32_t k = base_class(ca);
                        atomicAdd(&counts[(strand + k) * L + (p - lo)], 1u);
                        if (k < 4)
                            atomicAdd(&qsum[((strand >> 1) + k) * L + (p - lo)], Q);
                    }
                } else if (v && !gb && p - lo < L) {
                    atomicAdd(&counts[(strand + (uint32_t)CH_DEL) * L + (p - lo)], 1u);
                }
                if ((sI | sD) >> lane & 1ull) {
                    if (p == 0)
                        edge = true;
                    else if (p - 1 - lo < L)
                        atomicAdd(&counts[(strand + (gb ? (uint32_t)CH_INS_EVENT : (uint32_t)CH_DEL_EVENT)) * L + (p - 1 - lo)], 1u);
                }
                n_edge += (uint64_t)__popcll(__ballot(edge));
                n_filtered += (uint64_t)__popcll(__ballot(low));
            }
            const int nv = __popcll(mV);
            carry = (uint32_t)(mI >> (nv - 1) & 1ull) | (uint32_t)(mD >> (nv - 1) & 1ull) << 1;
            tbase += (uint64_t)__popcll(mT);
            abase += (uint64_t)__popcll(mA);
        }
        if (!ADD) {
            const uint64_t re = ref_end[i];
            uint32_t e = invalid ? 1u : (tbase != re || re > ref_len) ? 2u : ncols == 0 ? 3u : differs ? 5u : abase > m ? 6u : 0u;
            if (e == 0) { // the whole quality string, clipped parts included
                bool outside = false;
                for (uint64_t y0 = 0; y0 < m; y0 += 64) {
                    const uint64_t y = y0 + lane;
                    if (__ballot(y < m && (uint32_t)q[y] - qbase > MAX_Q)) // a byte below qbase wraps to a value above 93
                        outside = true;
                }
                e = outside ? 7u : 0u;
            }
            if (lane == 0)
                err[i] = e;
            n_bad += e ? 1u : 0u;
            n_used += e ? 0u : 1u;
            n_cols += e ? 0u : ncol;
        }
    }
    if (lane == 0) {
        if (n_used) {
            atomicAdd(&info[INFO_USED], (unsigned long long)n_used);
            atomicAdd(&info[INFO_COLUMNS], (unsigned long long)n_cols);
        }
        if (n_skipped)
            atomicAdd(&info[INFO_SKIPPED], (unsigned long long)n_skipped);
        if (n_bad)
            atomicAdd(&info[INFO_BAD], (unsigned long long)n_bad);
        if (n_edge)
            atomicAdd(&info[INFO_EDGE], (unsigned long long)n_edge);
        if (n_filtered)
            atomicAdd(&info[QINFO_FILTERED], (unsigned long long)n_filtered);
    }
}

} // namespace
} // namespace polyhip
