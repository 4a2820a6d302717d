// pileup.hip -- polyhip_pileup: what the mapped reads say about each text position: 16 integer counts, a consensus byte and
// the variant sites.  The definition is the comment above polyhip_pileup in include/polyhip.h; tests/pileup_oracle.py restates
// it in plain Python.
//
//   walk_kernel<false>  one wave per entry, 64 columns per step: err of the entry (the whole entry is judged before any add)
//   walk_kernel<true>   the same walk over the used entries: one 32-bit integer atomic add per counted column or event
//   call_kernel<false>  (pileup_call.h) one lane per position: the consensus byte and the number of sites (uint64, for the scan)
//   scan_excl           site offsets; the total comes back to the host with counts, consensus and err
//   call_kernel<true>   the same pass, writing the sites at the scanned offsets (after the host compared total and capacity)
//
// The walk is the one of aln_records.hip: a step loads one byte of alnA and one of alnB per lane and turns the classes into
// 64-bit masks with __ballot.  A lane's text position is the entry's running base plus the popcount of the b != '-' mask
// below the lane; the anchor of a run that starts at the lane is that position minus one, whichever step the column before
// it sat in, so the only other carry is the class of the step's last column.  counts is channel-major: the lanes of a run
// of matching columns add to consecutive words of one plane.  Sums of integers do not depend on the order of the adds.
#include "device_prims.h"
#include "host_pipeline.h"
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

thread_local polyhip_pileup_info t_info{};

} // namespace
} // namespace polyhip

using namespace polyhip;

extern "C" {

int polyhip_pileup(const polyhip_pileup_params *params, uint64_t n, const uint32_t *flags, const uint8_t *mapq, const uint32_t *ref_start,
                   const uint32_t *ref_end, const uint8_t *alnA, const uint8_t *alnB, const uint64_t *alnOff, const uint8_t *ref,
                   uint64_t ref_len, uint32_t *counts, uint8_t *consensus, uint64_t *nsites, polyhip_pileup_site *sites,
                   uint64_t site_capacity, uint32_t *err)
{
    const char *who = "polyhip_pileup";
    PH_REQUIRE(params, "%s: null params", who);
    PH_REQUIRE(params->region_lo <= params->region_hi, "%s: region_lo = %llu is above region_hi = %llu", who,
               (unsigned long long)params->region_lo, (unsigned long long)params->region_hi);
    PH_REQUIRE(params->region_hi <= ref_len, "%s: region_hi = %llu is above ref_len = %llu", who, (unsigned long long)params->region_hi,
               (unsigned long long)ref_len);
    PH_REQUIRE(params->min_alt_permille <= 1000, "%s: min_alt_permille = %u, it is 0 to 1000", who, params->min_alt_permille);
    if (n >> 32)
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %llu entries, the counts are uint32 and hold fewer than 2^32", who,
                         (unsigned long long)n);
    PH_REQUIRE(params->min_mapq == 0 || mapq, "%s: min_mapq = %u needs mapq, which is null", who, params->min_mapq);
    const uint64_t lo = params->region_lo, L = params->region_hi - params->region_lo;
    PH_REQUIRE(ref && nsites && (sites || site_capacity == 0) && (L == 0 || (counts && consensus)), "%s: null argument", who);
    PH_REQUIRE(n == 0 || (flags && ref_start && ref_end && alnOff && err && ((alnA && alnB) || alnOff[n] == alnOff[0])),
               "%s: null argument", who);
    for (uint64_t i = 0; i < n; ++i)
        PH_REQUIRE(alnOff[i + 1] >= alnOff[i], "%s: offsets are not ascending", who);
    const uint64_t nbytes = n ? alnOff[n] - alnOff[0] : 0;
    const bool by_mapq = params->min_mapq > 0;
    t_info = polyhip_pileup_info{};
    *nsites = 0;

    HostStreams &hs = host_streams();
    PH_HIP(hs.init());
    hipStream_t st = hs.s[0];
    Arena w;
    const size_t o_flags = w.reserve(n * 4), o_mapq = w.reserve(by_mapq ? n : 0), o_rs = w.reserve(n * 4), o_re = w.reserve(n * 4),
                 o_a = w.reserve(nbytes), o_b = w.reserve(nbytes), o_off = w.reserve((n + 1) * 8), o_ref = w.reserve(ref_len),
                 o_err = w.reserve(n * 4), o_counts = w.reserve(POLYHIP_PILEUP_CHANNELS * L * 4), o_cons = w.reserve(L),
                 o_nsite = w.reserve((L + 1) * 8), o_info = w.reserve(INFO_WORDS * sizeof(unsigned long long)),
                 o_scan = w.reserve(scan_scratch_bytes<uint64_t>(L));
    PH_HIP(w.buf.alloc(w.used));
    SyncOnExit sync(st);
    const struct {
        size_t at;
        const void *src;
        size_t bytes;
    } in[] = {{o_flags, flags, n * 4}, {o_mapq, mapq, by_mapq ? n : 0}, {o_rs, ref_start, n * 4}, {o_re, ref_end, n * 4},
              {o_a, nbytes ? alnA + alnOff[0] : nullptr, nbytes}, {o_b, nbytes ? alnB + alnOff[0] : nullptr, nbytes},
              {o_off, alnOff, n ? (n + 1) * 8 : 0}, {o_ref, ref, ref_len}};
    for (const auto &x : in)
        if (x.bytes)
            PH_HIP(hipMemcpyAsync(w.at<uint8_t>(x.at), x.src, x.bytes, hipMemcpyHostToDevice, st));
    PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_info), 0, INFO_WORDS * sizeof(unsigned long long), st));
    if (L)
        PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_counts), 0, POLYHIP_PILEUP_CHANNELS * L * 4, st));

    if (n) {
        const unsigned wgrid = grid_for(n, PU_WAVES, PU_MAX_BLOCKS);
        hipLaunchKernelGGL(walk_kernel<false>, dim3(wgrid), dim3(BT), 0, st, n, params->min_mapq, lo, L, ref_len, w.at<uint32_t>(o_flags),
                           w.at<uint8_t>(o_mapq), w.at<uint32_t>(o_rs), w.at<uint32_t>(o_re), w.at<uint8_t>(o_a), w.at<uint8_t>(o_b),
                           w.at<uint64_t>(o_off), w.at<uint8_t>(o_ref), w.at<uint32_t>(o_err), w.at<uint32_t>(o_counts),
                           w.at<unsigned long long>(o_info));
        PH_HIP(hipGetLastError());
        // with L == 0 no add lands anywhere, but the events at anchor -1 are still counted
        hipLaunchKernelGGL(walk_kernel<true>, dim3(wgrid), dim3(BT), 0, st, n, params->min_mapq, lo, L, ref_len, w.at<uint32_t>(o_flags),
                           w.at<uint8_t>(o_mapq), w.at<uint32_t>(o_rs), w.at<uint32_t>(o_re), w.at<uint8_t>(o_a), w.at<uint8_t>(o_b),
                           w.at<uint64_t>(o_off), w.at<uint8_t>(o_ref), w.at<uint32_t>(o_err), w.at<uint32_t>(o_counts),
                           w.at<unsigned long long>(o_info));
        PH_HIP(hipGetLastError());
    }
    const uint32_t min_depth = std::max(params->min_depth, 1u), min_count = std::max(params->min_alt_count, 1u);
    const unsigned cgrid = grid_for(L, BT, 1u << 20);
    if (L) {
        hipLaunchKernelGGL(call_kernel<false>, dim3(cgrid), dim3(BT), 0, st, lo, L, min_depth, min_count, params->min_alt_permille,
                           w.at<uint32_t>(o_counts), w.at<uint8_t>(o_ref), w.at<uint8_t>(o_cons), w.at<uint64_t>(o_nsite),
                           (polyhip_pileup_site *)nullptr);
        PH_HIP(hipGetLastError());
    }
    PH_HIP(scan_excl<uint64_t>(w.at<uint64_t>(o_nsite), w.at<uint64_t>(o_nsite), L, w.at<uint8_t>(o_scan), st));
    unsigned long long info[INFO_WORDS];
    uint64_t total = 0;
    if (n)
        PH_HIP(hipMemcpyAsync(err, w.at<uint8_t>(o_err), n * 4, hipMemcpyDeviceToHost, st));
    if (L) {
        PH_HIP(hipMemcpyAsync(counts, w.at<uint8_t>(o_counts), POLYHIP_PILEUP_CHANNELS * L * 4, hipMemcpyDeviceToHost, st));
        PH_HIP(hipMemcpyAsync(consensus, w.at<uint8_t>(o_cons), L, hipMemcpyDeviceToHost, st));
    }
    PH_HIP(hipMemcpyAsync(info, w.at<uint8_t>(o_info), sizeof info, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(&total, w.at<uint64_t>(o_nsite) + L, sizeof total, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    *nsites = total;
    t_info = polyhip_pileup_info{n, info[INFO_USED], info[INFO_SKIPPED], info[INFO_BAD], info[INFO_COLUMNS], info[INFO_EDGE], total};
    if (total > site_capacity)
        return set_error(POLYHIP_ERR_INVALID, "%s: the sites need %llu entries, the buffer holds %llu", who, (unsigned long long)total,
                         (unsigned long long)site_capacity);
    if (total == 0)
        return POLYHIP_OK;
    // only now, bounded by the caller's capacity: the sites themselves
    DevBuf dsites;
    PH_HIP(dsites.alloc(total * sizeof(polyhip_pileup_site)));
    hipLaunchKernelGGL(call_kernel<true>, dim3(cgrid), dim3(BT), 0, st, lo, L, min_depth, min_count, params->min_alt_permille,
                       w.at<uint32_t>(o_counts), w.at<uint8_t>(o_ref), w.at<uint8_t>(o_cons), w.at<uint64_t>(o_nsite),
                       dsites.as<polyhip_pileup_site>());
    PH_HIP(hipGetLastError());
    PH_HIP(hipMemcpyAsync(sites, dsites.p, total * sizeof(polyhip_pileup_site), hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    return POLYHIP_OK;
}

int polyhip_pileup_last_info(polyhip_pileup_info *info)
{
    PH_REQUIRE(info, "polyhip_pileup_last_info: null argument");
    *info = t_info;
    return POLYHIP_OK;
}

} // extern "C"
