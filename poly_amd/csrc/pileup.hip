// pileup.hip -- polyhip_pileup: what the mapped reads say about each text position: 16 integer counts, a consensus byte and
// the variant sites.  The definition is the comment above polyhip_pileup in include/polyhip.h; tests/pileup_oracle.py restates
// it in plain Python.
//
//   walk_kernel<false>  (pileup_walk.h) one wave per entry, 64 columns per step: err of the entry (the whole entry is judged
//                       before any add)
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
#include "pileup_walk.h"

namespace polyhip {
namespace {

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
