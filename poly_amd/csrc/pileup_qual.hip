// pileup_qual.hip -- polyhip_pileup_qual: polyhip_pileup with a minimum base quality and per-base quality sums.  The
// definition is the comment above polyhip_pileup_qual in include/polyhip.h; tests/pileup_qual_oracle.py restates it in plain
// Python.
//
//   walk_qual_kernel<false>  (pileup_walk.h) one wave per entry, 64 columns per step: err of the entry, then (only if nothing else applies)
//                            a sweep of the entry's whole quality string, 64 bytes per step, for err 7
//   walk_qual_kernel<true>   the same walk over the used entries: per counted base column one 32-bit atomic add to counts and,
//                            for A, C, G, T, one to qsum; D columns and events as in pileup.hip
//   call_kernel, scan_excl   pileup_call.h: the consensus and the sites from the (filtered) counts, unchanged
//
// It is pileup.hip's walk with one more running base: the index in the oriented read q of the next column with a != '-',
// carried from step to step like the text position, a lane's own being that plus the popcount of the a != '-' mask below
// the lane.  The quality of the column is one byte gathered from the entry's string at that index, counted from the other
// end on the reverse strand: either way the 64 lanes of a step read one contiguous run.  The kernel is a copy of its own so
// that polyhip_pileup's instantiation stays what it is.  Sums of integers do not depend on the order of the adds.
// The add pass issues two 32-bit atomics per counted A, C, G, T column.  One 64-bit atomic of (Q << 32) + 1 into a paired
// plane and a split pass was built and measured beside it: 0.2 ms less in the kernels, nothing at the call, 40 bytes of
// device memory more per position; it was not kept.
#include "device_prims.h"
#include "host_pipeline.h"
#include "pileup_call.h"
#include "pileup_walk.h"

namespace polyhip {
namespace {

thread_local polyhip_pileup_qual_info t_qinfo{};

} // namespace
} // namespace polyhip

using namespace polyhip;

extern "C" {

int polyhip_pileup_qual(const polyhip_pileup_qual_params *params, uint64_t n, const uint32_t *flags, const uint8_t *mapq,
                        const uint32_t *ref_start, const uint32_t *ref_end, const uint32_t *read_start, const uint8_t *alnA,
                        const uint8_t *alnB, const uint64_t *alnOff, const uint8_t *qual, const uint64_t *qualOff, const uint8_t *ref,
                        uint64_t ref_len, uint32_t *counts, uint32_t *qsum, uint8_t *consensus, uint64_t *nsites, polyhip_pileup_site *sites,
                        uint64_t site_capacity, uint32_t *err)
{
    const char *who = "polyhip_pileup_qual";
    PH_REQUIRE(params, "%s: null params", who);
    const polyhip_pileup_params &pb = params->base;
    PH_REQUIRE(pb.region_lo <= pb.region_hi, "%s: region_lo = %llu is above region_hi = %llu", who, (unsigned long long)pb.region_lo,
               (unsigned long long)pb.region_hi);
    PH_REQUIRE(pb.region_hi <= ref_len, "%s: region_hi = %llu is above ref_len = %llu", who, (unsigned long long)pb.region_hi,
               (unsigned long long)ref_len);
    PH_REQUIRE(pb.min_alt_permille <= 1000, "%s: min_alt_permille = %u, it is 0 to 1000", who, pb.min_alt_permille);
    PH_REQUIRE(params->min_base_qual <= MAX_Q, "%s: min_base_qual = %u, it is 0 to %u", who, params->min_base_qual, MAX_Q);
    PH_REQUIRE(params->qual_offset <= 255u - MAX_Q, "%s: qual_offset = %u, it is 0 to %u", who, params->qual_offset, 255u - MAX_Q);
    if (n > 0xFFFFFFFFull / MAX_Q)
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %llu entries, the quality sums are uint32 and hold fewer than 2^32 / %u of them", who,
                         (unsigned long long)n, MAX_Q);
    PH_REQUIRE(pb.min_mapq == 0 || mapq, "%s: min_mapq = %u needs mapq, which is null", who, pb.min_mapq);
    const uint64_t lo = pb.region_lo, L = pb.region_hi - pb.region_lo;
    PH_REQUIRE(ref && nsites && (sites || site_capacity == 0) && (L == 0 || (counts && qsum && consensus)), "%s: null argument", who);
    PH_REQUIRE(n == 0 || (flags && ref_start && ref_end && read_start && alnOff && qualOff && err &&
                          ((alnA && alnB) || alnOff[n] == alnOff[0]) && (qual || qualOff[n] == qualOff[0])),
               "%s: null argument", who);
    for (uint64_t i = 0; i < n; ++i)
        PH_REQUIRE(alnOff[i + 1] >= alnOff[i] && qualOff[i + 1] >= qualOff[i], "%s: offsets are not ascending", who);
    const uint64_t nbytes = n ? alnOff[n] - alnOff[0] : 0, qbytes = n ? qualOff[n] - qualOff[0] : 0;
    const bool by_mapq = pb.min_mapq > 0;
    t_qinfo = polyhip_pileup_qual_info{};
    *nsites = 0;

    HostStreams &hs = host_streams();
    PH_HIP(hs.init());
    hipStream_t st = hs.s[0];
    Arena w;
    const size_t o_flags = w.reserve(n * 4), o_mapq = w.reserve(by_mapq ? n : 0), o_rs = w.reserve(n * 4), o_re = w.reserve(n * 4),
                 o_qs = w.reserve(n * 4), o_a = w.reserve(nbytes), o_b = w.reserve(nbytes), o_off = w.reserve((n + 1) * 8),
                 o_q = w.reserve(qbytes), o_qoff = w.reserve((n + 1) * 8), o_ref = w.reserve(ref_len), o_err = w.reserve(n * 4),
                 o_counts = w.reserve(POLYHIP_PILEUP_CHANNELS * L * 4), o_qsum = w.reserve(POLYHIP_PILEUP_QSUM_PLANES * L * 4),
                 o_cons = w.reserve(L), o_nsite = w.reserve((L + 1) * 8), o_info = w.reserve(QINFO_WORDS * sizeof(unsigned long long)),
                 o_scan = w.reserve(scan_scratch_bytes<uint64_t>(L));
    PH_HIP(w.buf.alloc(w.used));
    SyncOnExit sync(st);
    const struct {
        size_t at;
        const void *src;
        size_t bytes;
    } in[] = {{o_flags, flags, n * 4}, {o_mapq, mapq, by_mapq ? n : 0}, {o_rs, ref_start, n * 4}, {o_re, ref_end, n * 4},
              {o_qs, read_start, n * 4}, {o_a, nbytes ? alnA + alnOff[0] : nullptr, nbytes}, {o_b, nbytes ? alnB + alnOff[0] : nullptr, nbytes},
              {o_off, alnOff, n ? (n + 1) * 8 : 0}, {o_q, qbytes ? qual + qualOff[0] : nullptr, qbytes},
              {o_qoff, qualOff, n ? (n + 1) * 8 : 0}, {o_ref, ref, ref_len}};
    for (const auto &x : in)
        if (x.bytes)
            PH_HIP(hipMemcpyAsync(w.at<uint8_t>(x.at), x.src, x.bytes, hipMemcpyHostToDevice, st));
    PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_info), 0, QINFO_WORDS * sizeof(unsigned long long), st));
    if (L) {
        PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_counts), 0, POLYHIP_PILEUP_CHANNELS * L * 4, st));
        PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_qsum), 0, POLYHIP_PILEUP_QSUM_PLANES * L * 4, st));
    }

    if (n) {
        const unsigned wgrid = grid_for(n, PU_WAVES, PU_MAX_BLOCKS);
        auto walk = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(wgrid), dim3(BT), 0, st, n, pb.min_mapq, params->min_base_qual, params->qual_offset, lo, L, ref_len,
                               w.at<uint32_t>(o_flags), w.at<uint8_t>(o_mapq), w.at<uint32_t>(o_rs), w.at<uint32_t>(o_re), w.at<uint32_t>(o_qs),
                               w.at<uint8_t>(o_a), w.at<uint8_t>(o_b), w.at<uint64_t>(o_off), w.at<uint8_t>(o_q), w.at<uint64_t>(o_qoff),
                               w.at<uint8_t>(o_ref), w.at<uint32_t>(o_err), w.at<uint32_t>(o_counts), w.at<uint32_t>(o_qsum),
                               w.at<unsigned long long>(o_info));
            return hipGetLastError();
        };
        PH_HIP(walk(walk_qual_kernel<false>));
        // with L == 0 no add lands anywhere, but the events at anchor -1 and the filtered bases are still counted
        PH_HIP(walk(walk_qual_kernel<true>));
    }
    const uint32_t min_depth = std::max(pb.min_depth, 1u), min_count = std::max(pb.min_alt_count, 1u);
    const unsigned cgrid = grid_for(L, BT, 1u << 20);
    if (L) {
        hipLaunchKernelGGL(call_kernel<false>, dim3(cgrid), dim3(BT), 0, st, lo, L, min_depth, min_count, pb.min_alt_permille,
                           w.at<uint32_t>(o_counts), w.at<uint8_t>(o_ref), w.at<uint8_t>(o_cons), w.at<uint64_t>(o_nsite),
                           (polyhip_pileup_site *)nullptr);
        PH_HIP(hipGetLastError());
    }
    PH_HIP(scan_excl<uint64_t>(w.at<uint64_t>(o_nsite), w.at<uint64_t>(o_nsite), L, w.at<uint8_t>(o_scan), st));
    unsigned long long info[QINFO_WORDS];
    uint64_t total = 0;
    if (n)
        PH_HIP(hipMemcpyAsync(err, w.at<uint8_t>(o_err), n * 4, hipMemcpyDeviceToHost, st));
    if (L) {
        PH_HIP(hipMemcpyAsync(counts, w.at<uint8_t>(o_counts), POLYHIP_PILEUP_CHANNELS * L * 4, hipMemcpyDeviceToHost, st));
        PH_HIP(hipMemcpyAsync(qsum, w.at<uint8_t>(o_qsum), POLYHIP_PILEUP_QSUM_PLANES * L * 4, hipMemcpyDeviceToHost, st));
        PH_HIP(hipMemcpyAsync(consensus, w.at<uint8_t>(o_cons), L, hipMemcpyDeviceToHost, st));
    }
    PH_HIP(hipMemcpyAsync(info, w.at<uint8_t>(o_info), sizeof info, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(&total, w.at<uint64_t>(o_nsite) + L, sizeof total, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    *nsites = total;
    t_qinfo = polyhip_pileup_qual_info{n, info[INFO_USED], info[INFO_SKIPPED], info[INFO_BAD], info[INFO_COLUMNS], info[INFO_EDGE], total,
                                       info[QINFO_FILTERED]};
    if (total > site_capacity)
        return set_error(POLYHIP_ERR_INVALID, "%s: the sites need %llu entries, the buffer holds %llu", who, (unsigned long long)total,
                         (unsigned long long)site_capacity);
    if (total == 0)
        return POLYHIP_OK;
    // only now, bounded by the caller's capacity: the sites themselves
    DevBuf dsites;
    PH_HIP(dsites.alloc(total * sizeof(polyhip_pileup_site)));
    hipLaunchKernelGGL(call_kernel<true>, dim3(cgrid), dim3(BT), 0, st, lo, L, min_depth, min_count, pb.min_alt_permille,
                       w.at<uint32_t>(o_counts), w.at<uint8_t>(o_ref), w.at<uint8_t>(o_cons), w.at<uint64_t>(o_nsite),
                       dsites.as<polyhip_pileup_site>());
    PH_HIP(hipGetLastError());
    PH_HIP(hipMemcpyAsync(sites, dsites.p, total * sizeof(polyhip_pileup_site), hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    return POLYHIP_OK;
}

int polyhip_pileup_qual_last_info(polyhip_pileup_qual_info *info)
{
    PH_REQUIRE(info, "polyhip_pileup_qual_last_info: null argument");
    *info = t_qinfo;
    return POLYHIP_OK;
}

} // extern "C"
