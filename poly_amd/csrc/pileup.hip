// pileup.hip -- polyhip_pileup: what the mapped reads say about each text position: 16 integer counts, a consensus byte and
// the variant sites; and polyhip_pileup_qual: the same with a minimum base quality and per-base quality sums.  The
// definitions are the comments above the two in include/polyhip.h; tests/pileup_oracle.py and tests/pileup_qual_oracle.py
// restate them in plain Python.  Both are one body, with qualities or without:
//
//   walk_entries        (pileup_walk.h) judges every entry, then walks the used ones again and adds them to the count planes
//                       (and, with qualities, to the qsum planes)
//   call_kernel<false>  (pileup_call.h) one lane per position: the consensus byte and the number of sites (uint64, for the scan)
//   scan_excl           site offsets; the total comes back to the host with counts, qsum, consensus and err
//   call_kernel<true>   the same pass, writing the sites at the scanned offsets (after the host compared total and capacity)
//
// With qualities the add pass issues two 32-bit atomics per counted A, C, G, T column.  One 64-bit atomic of (Q << 32) + 1
// into a paired plane and a split pass was built and measured beside it: 0.2 ms less in the kernels, nothing at the call,
// 40 bytes of device memory more per position; it was not kept.
#include "device_prims.h"
#include "host_pipeline.h"
#include "pileup_call.h"
#include "pileup_walk.h"

namespace polyhip {
namespace {

thread_local polyhip_pileup_info t_info{};
thread_local polyhip_pileup_qual_info t_qinfo{};

void set_info(bool with_q, const polyhip_pileup_qual_info &x)
{
    if (with_q)
        t_qinfo = x;
    else
        t_info = polyhip_pileup_info{x.entries, x.used, x.skipped_mapq, x.bad, x.columns, x.edge_events, x.sites};
}

// with_q == false: min_q, qbase and qsum are not looked at.  H: the caller's host arrays
int pileup(const char *who, const polyhip_pileup_params &pb, bool with_q, uint32_t min_q, uint32_t qbase, const Entries &H, const uint8_t *ref,
           uint64_t ref_len, uint32_t *counts, uint32_t *qsum, uint8_t *consensus, uint64_t *nsites, polyhip_pileup_site *sites,
           uint64_t site_capacity)
{
    const uint64_t n = H.n;
    if (int rc = check_region(who, pb.region_lo, pb.region_hi, ref_len))
        return rc;
    PH_REQUIRE(pb.min_alt_permille <= 1000, "%s: min_alt_permille = %u, it is 0 to 1000", who, pb.min_alt_permille);
    if (with_q) {
        if (int rc = check_qual_params(who, min_q, qbase))
            return rc;
        if (n > 0xFFFFFFFFull / MAX_Q)
            return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %llu entries, the quality sums are uint32 and hold fewer than 2^32 / %u of them",
                             who, (unsigned long long)n, MAX_Q);
    } else if (n >> 32) {
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %llu entries, the counts are uint32 and hold fewer than 2^32", who,
                         (unsigned long long)n);
    }
    PH_REQUIRE(pb.min_mapq == 0 || H.mapq, "%s: min_mapq = %u needs mapq, which is null", who, pb.min_mapq);
    const uint64_t lo = pb.region_lo, L = pb.region_hi - pb.region_lo;
    PH_REQUIRE(ref && nsites && (sites || site_capacity == 0) && (L == 0 || (counts && (qsum || !with_q) && consensus)), "%s: null argument",
               who);
    if (int rc = check_entries(who, H, with_q))
        return rc;
    set_info(with_q, {});
    *nsites = 0;

    HostStreams &hs = host_streams();
    PH_HIP(hs.init());
    hipStream_t st = hs.s[0];
    Arena w;
    const EntryStage stage(w, H, ref_len, pb.min_mapq > 0, with_q);
    const size_t info_bytes = (with_q ? QINFO_WORDS : INFO_WORDS) * sizeof(unsigned long long);
    const size_t o_counts = w.reserve(POLYHIP_PILEUP_CHANNELS * L * 4), o_qsum = w.reserve(with_q ? POLYHIP_PILEUP_QSUM_PLANES * L * 4 : 0),
                 o_cons = w.reserve(L), o_nsite = w.reserve((L + 1) * 8), o_info = w.reserve(info_bytes),
                 o_scan = w.reserve(scan_scratch_bytes<uint64_t>(L));
    PH_HIP(w.buf.alloc(w.used));
    SyncOnExit sync(st);
    Entries E;
    PH_HIP(stage.upload(w, ref, st, E));
    PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_info), 0, info_bytes, st));
    if (L) {
        PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_counts), 0, POLYHIP_PILEUP_CHANNELS * L * 4, st));
        if (with_q)
            PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_qsum), 0, POLYHIP_PILEUP_QSUM_PLANES * L * 4, st));
    }

    const WalkArgs W{lo, L, ref_len, stage.ref(w), min_q, qbase, w.at<uint32_t>(o_counts), w.at<uint32_t>(o_qsum),
                     w.at<unsigned long long>(o_info)};
    PH_HIP(walk_entries(E, W, false, with_q, st));
    // with L == 0 no add lands anywhere, but the events at anchor -1 and the filtered bases are still counted
    PH_HIP(walk_entries(E, W, true, with_q, st));
    const uint32_t min_depth = std::max(pb.min_depth, 1u), min_count = std::max(pb.min_alt_count, 1u);
    const unsigned cgrid = grid_for(L, BT, 1u << 20);
    if (L) {
        hipLaunchKernelGGL(call_kernel<false>, dim3(cgrid), dim3(BT), 0, st, lo, L, min_depth, min_count, pb.min_alt_permille, W.counts, W.ref,
                           w.at<uint8_t>(o_cons), w.at<uint64_t>(o_nsite), (polyhip_pileup_site *)nullptr);
        PH_HIP(hipGetLastError());
    }
    PH_HIP(scan_excl<uint64_t>(w.at<uint64_t>(o_nsite), w.at<uint64_t>(o_nsite), L, w.at<uint8_t>(o_scan), st));
    unsigned long long info[QINFO_WORDS] = {};
    uint64_t total = 0;
    if (n)
        PH_HIP(hipMemcpyAsync(H.err, E.err, n * 4, hipMemcpyDeviceToHost, st));
    if (L) {
        PH_HIP(hipMemcpyAsync(counts, W.counts, POLYHIP_PILEUP_CHANNELS * L * 4, hipMemcpyDeviceToHost, st));
        if (with_q)
            PH_HIP(hipMemcpyAsync(qsum, W.qsum, POLYHIP_PILEUP_QSUM_PLANES * L * 4, hipMemcpyDeviceToHost, st));
        PH_HIP(hipMemcpyAsync(consensus, w.at<uint8_t>(o_cons), L, hipMemcpyDeviceToHost, st));
    }
    PH_HIP(hipMemcpyAsync(info, W.info, info_bytes, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(&total, w.at<uint64_t>(o_nsite) + L, sizeof total, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    *nsites = total;
    set_info(with_q, {n, info[INFO_USED], info[INFO_SKIPPED], info[INFO_BAD], info[INFO_COLUMNS], info[INFO_EDGE], total, info[QINFO_FILTERED]});
    if (total > site_capacity)
        return set_error(POLYHIP_ERR_INVALID, "%s: the sites need %llu entries, the buffer holds %llu", who, (unsigned long long)total,
                         (unsigned long long)site_capacity);
    if (total == 0)
        return POLYHIP_OK;
    // only now, bounded by the caller's capacity: the sites themselves
    DevBuf dsites;
    PH_HIP(dsites.alloc(total * sizeof(polyhip_pileup_site)));
    hipLaunchKernelGGL(call_kernel<true>, dim3(cgrid), dim3(BT), 0, st, lo, L, min_depth, min_count, pb.min_alt_permille, W.counts, W.ref,
                       w.at<uint8_t>(o_cons), w.at<uint64_t>(o_nsite), dsites.as<polyhip_pileup_site>());
    PH_HIP(hipGetLastError());
    PH_HIP(hipMemcpyAsync(sites, dsites.p, total * sizeof(polyhip_pileup_site), hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    return POLYHIP_OK;
}

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
    const Entries H{n, params->min_mapq, flags, mapq, ref_start, ref_end, nullptr, alnA, alnB, alnOff, nullptr, nullptr, err, nullptr};
    return pileup(who, *params, false, 0, 0, H, ref, ref_len, counts, nullptr, consensus, nsites, sites, site_capacity);
}

int polyhip_pileup_last_info(polyhip_pileup_info *info)
{
    PH_REQUIRE(info, "polyhip_pileup_last_info: null argument");
    *info = t_info;
    return POLYHIP_OK;
}

int polyhip_pileup_qual(const polyhip_pileup_qual_params *params, uint64_t n, const uint32_t *flags, const uint8_t *mapq,
                        const uint32_t *ref_start, const uint32_t *ref_end, const uint32_t *read_start, const uint8_t *alnA,
                        const uint8_t *alnB, const uint64_t *alnOff, const uint8_t *qual, const uint64_t *qualOff, const uint8_t *ref,
                        uint64_t ref_len, uint32_t *counts, uint32_t *qsum, uint8_t *consensus, uint64_t *nsites, polyhip_pileup_site *sites,
                        uint64_t site_capacity, uint32_t *err)
{
    const char *who = "polyhip_pileup_qual";
    PH_REQUIRE(params, "%s: null params", who);
    const Entries H{n, params->base.min_mapq, flags, mapq, ref_start, ref_end, read_start, alnA, alnB, alnOff, qual, qualOff, err, nullptr};
    return pileup(who, params->base, true, params->min_base_qual, params->qual_offset, H, ref, ref_len, counts, qsum, consensus, nsites, sites,
                  site_capacity);
}

int polyhip_pileup_qual_last_info(polyhip_pileup_qual_info *info)
{
    PH_REQUIRE(info, "polyhip_pileup_qual_last_info: null argument");
    *info = t_qinfo;
    return POLYHIP_OK;
}

} // extern "C"
