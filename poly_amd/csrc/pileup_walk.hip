// pileup_walk.hip -- walk_entries (pileup_walk.h): the entry walk of the pileup family, one kernel in four instantiations.
//
//   walk_kernel<false, QUAL>  one wave per entry, 64 columns per step: err of the entry (the whole entry is judged before any
//                             add); with QUAL then (only if nothing else applies) a sweep of the entry's whole quality
//                             string, 64 bytes per step, for err 7
//   walk_kernel<true, QUAL>   the same walk over the used entries: one 32-bit integer atomic add per counted column or event;
//                             with QUAL a base column below min_q is not counted and A, C, G, T add their quality to qsum
//
// The quality of a column is one byte gathered from the entry's string at the lane's index in the oriented read, counted
// from the other end on the reverse strand: either way the 64 lanes of a step read one contiguous run.  Everything about
// qualities stands under if constexpr (QUAL): the plain instantiations hold none of it (DESIGN.md M5 has the resource
// numbers of all four).  counts is channel-major: the lanes of a run of matching columns add to consecutive words of one
// plane.  Sums of integers do not depend on the order of the adds.
#include "pileup_walk.h"

namespace polyhip {
namespace {

template <bool ADD, bool QUAL> __global__ __launch_bounds__(BT) void walk_kernel(Entries E, WalkArgs W)
{
    const int lane = threadIdx.x & 63;
    const uint64_t lo = W.lo, L = W.L;
    const uint64_t off0 = E.n ? E.alnOff[0] : 0; // the device copies of the strings start at the first entry's bytes
    uint64_t qoff0 = 0;
    if constexpr (QUAL)
        qoff0 = E.n ? E.qualOff[0] : 0;
    uint64_t n_used = 0, n_skipped = 0, n_bad = 0, n_cols = 0, n_edge = 0, n_filtered = 0; // of this wave's entries, the same in every lane
    for (uint64_t i = (uint64_t)blockIdx.x * PU_WAVES + (threadIdx.x >> 6); i < E.n; i += (uint64_t)gridDim.x * PU_WAVES) {
        const uint32_t f = E.flags[i];
        const bool mapped = f & 1u;
        const bool skipped = mapped && E.min_mapq > 0 && E.mapq[i] < E.min_mapq; // min_mapq > 0 comes with a mapq array
        const uint64_t ncol = E.alnOff[i + 1] - E.alnOff[i];
        if (!ADD && (!mapped || skipped || ncol > POLYHIP_ALN_MAX_COLUMNS)) {
            const uint32_t e = mapped && !skipped ? 4u : 0u;
            if (lane == 0)
                E.err[i] = e;
            n_skipped += skipped ? 1u : 0u;
            n_bad += e ? 1u : 0u;
            continue;
        }
        if (ADD && (!mapped || skipped || E.err[i] != 0))
            continue;
        const uint32_t ncols = (uint32_t)ncol;
        const uint8_t *a = E.alnA + (E.alnOff[i] - off0), *b = E.alnB + (E.alnOff[i] - off0);
        const uint8_t *q = nullptr;
        uint64_t m = 0;
        if constexpr (QUAL) {
            q = E.qual + (E.qualOff[i] - qoff0);
            m = E.qualOff[i + 1] - E.qualOff[i];
        }
        const bool reverse = f & 2u;
        const uint32_t strand = reverse ? CH_STRAND : 0u;
        ColumnWalk S(E.ref_start[i], QUAL ? E.read_start[i] : 0u);
        bool invalid = false, differs = false;
        for (uint32_t base = 0; base < ncols; base += 64) {
            S.load(a, b, base, ncols, lane);
            const bool v = S.v, ga = S.ga, gb = S.gb;
            const uint64_t p = S.p;
            if (!ADD && __ballot(v && ga && gb)) {
                invalid = true;
                break;
            }
            if (!ADD) {
                if (__ballot(v && !gb && (p >= W.ref_len || S.cb != W.ref[p])))
                    differs = true;
            } else {
                bool edge = false, low = false;
                if constexpr (QUAL) {
                    if (v && !ga && !gb) { // err[i] == 0: x < m, the byte is inside the entry's string and in qbase .. qbase + 93
                        const uint64_t x = S.x(lane);
                        const uint32_t Q = (uint32_t)q[reverse ? m - 1 - x : x] - W.qbase;
                        low = Q < W.min_q;
                        if (!low && p - lo < L) { // p < lo wraps to a value above L
                            const uint32_t k = base_class(S.ca);
                            atomicAdd(&W.counts[(strand + k) * L + (p - lo)], 1u);
                            if (k < 4)
                                atomicAdd(&W.qsum[((strand >> 1) + k) * L + (p - lo)], Q);
                        }
                    } else if (v && !gb && p - lo < L) {
                        atomicAdd(&W.counts[(strand + (uint32_t)CH_DEL) * L + (p - lo)], 1u);
                    }
                } else if (v && !gb && p - lo < L) { // p < lo wraps to a value above L
                    atomicAdd(&W.counts[(strand + (ga ? (uint32_t)CH_DEL : base_class(S.ca))) * L + (p - lo)], 1u);
                }
                if ((S.sI() | S.sD()) >> lane & 1ull) {
                    if (p == 0)
                        edge = true;
                    else if (p - 1 - lo < L)
                        atomicAdd(&W.counts[(strand + (gb ? (uint32_t)CH_INS_EVENT : (uint32_t)CH_DEL_EVENT)) * L + (p - 1 - lo)], 1u);
                }
                n_edge += (uint64_t)__popcll(__ballot(edge));
                if constexpr (QUAL)
                    n_filtered += (uint64_t)__popcll(__ballot(low));
            }
            S.advance();
        }
        if (!ADD) {
            const uint64_t re = E.ref_end[i];
            uint32_t e = invalid ? 1u : (S.tbase != re || re > W.ref_len) ? 2u : ncols == 0 ? 3u : differs ? 5u : 0u;
            if constexpr (QUAL) {
                if (e == 0 && S.abase > m)
                    e = 6u;
                if (e == 0) { // the whole quality string, clipped parts included
                    bool outside = false;
                    for (uint64_t y0 = 0; y0 < m; y0 += 64) {
                        const uint64_t y = y0 + lane;
                        if (__ballot(y < m && (uint32_t)q[y] - W.qbase > MAX_Q)) // a byte below qbase wraps to a value above 93
                            outside = true;
                    }
                    e = outside ? 7u : 0u;
                }
            }
            if (lane == 0)
                E.err[i] = e;
            n_bad += e ? 1u : 0u;
            n_used += e ? 0u : 1u;
            n_cols += e ? 0u : ncol;
        }
    }
    if (lane == 0) {
        if (n_used) {
            atomicAdd(&W.info[INFO_USED], (unsigned long long)n_used);
            atomicAdd(&W.info[INFO_COLUMNS], (unsigned long long)n_cols);
        }
        if (n_skipped)
            atomicAdd(&W.info[INFO_SKIPPED], (unsigned long long)n_skipped);
        if (n_bad)
            atomicAdd(&W.info[INFO_BAD], (unsigned long long)n_bad);
        if (n_edge)
            atomicAdd(&W.info[INFO_EDGE], (unsigned long long)n_edge);
        if (n_filtered)
            atomicAdd(&W.info[QINFO_FILTERED], (unsigned long long)n_filtered);
    }
}

} // namespace

hipError_t walk_entries(const Entries &E, const WalkArgs &W, bool add, bool with_qual, hipStream_t st)
{
    if (E.n == 0)
        return hipSuccess;
    const dim3 grid(grid_for(E.n, PU_WAVES, PU_MAX_BLOCKS)), block(BT);
    if (with_qual && add)
        hipLaunchKernelGGL((walk_kernel<true, true>), grid, block, 0, st, E, W);
    else if (with_qual)
        hipLaunchKernelGGL((walk_kernel<false, true>), grid, block, 0, st, E, W);
    else if (add)
        hipLaunchKernelGGL((walk_kernel<true, false>), grid, block, 0, st, E, W);
    else
        hipLaunchKernelGGL((walk_kernel<false, false>), grid, block, 0, st, E, W);
    return hipGetLastError();
}

} // namespace polyhip
