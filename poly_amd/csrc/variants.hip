// variants.hip -- polyhip_call_variants: the mapped reads' events grouped into alleles (position, kind, length, bytes),
// left-aligned first, counted per strand, put to the pileup's thresholds and merged with the SNV records.  The definition is
// the comment above polyhip_call_variants in include/polyhip.h; tests/variants_oracle.py restates it in plain Python.
//
//   walk_entries          (pileup_walk.h) err of every entry, then the 16 count planes and, with qualities, the 8 qsum planes,
//                         on the device only
//   snv_kernel<false>     one lane per position: the depth and the number of SNV records of the position
//   event_kernel<false>   one wave per used entry, 64 columns per step, the pileup's walk (ColumnWalk) with its run-start masks.  For
//                         every run the wave finds its length (ballots over 64 columns at a time, the first column of another
//                         class from the complement mask) and its shift k (ballots over 64 steps t at a time, the first failing
//                         step from the complement mask; a shift longer than 64 goes round again), and judges it: long, open,
//                         edge, kept.  It counts the kept events of the region per entry and the info counters
//   scan_excl<uint64>     the first item of every entry; the total N goes to the host (more than 2^32 - 1 is refused)
//   event_kernel<true>    the same walk: item first[i] + (its rank among the entry's items) = key (pos - lo, kind, length), entry,
//                         first allele column, strand
//   wordkey_kernel, radix_sort   for w = ceil(longest insertion / 8) - 1 down to 0: bytes [8w, 8w + 8) of every item's allele as
//                         one big-endian word (0 for a deletion and behind the allele's end), a stable sort by it; none
//                         without insertions
//   mainkey_kernel, radix_sort   a stable sort by (pos - lo, kind, length): equal alleles now stand together, in record order
//   head_kernel           one lane per sorted item: does a new site (pos, kind) start here, does a new allele (the key, and for an
//                         insertion a comparison of all folded bytes with the item before: exact, no hash); is it strand 0
//   scan_excl<uint32> x 3 allele ids, site ids, forward items before
//   start_kernel          the first sorted item of every allele and of every site, placed by the scans
//   allele_kernel<false>  one lane per allele: count, forward count, site_events, the depth of its position -> does it pass,
//                         how many pool bytes does it need
//   scan_excl             the passing alleles before each allele; the pool bytes before it.  The totals go to the host, which
//                         compares them with the capacities
//   snv_kernel<true>      the SNV records of a position at (SNV records before the position) + (passing alleles before it: a
//                         binary search in the alleles' positions)
//   allele_kernel<true>   the record of a passing allele at (SNV records up to its position) + (passing alleles before it), its
//                         bytes into the pool
//
// Where a record or a byte goes is decided by scans and by the stable sort alone; the only atomics are the pileup's integer adds
// and the info counters.  Runs are about one in a hundred columns, so a wave that stops at each of its entry's runs costs
// little beside the walk; long runs and long shifts are rare and only slow their own entry.
#include "device_prims.h"
#include "host_pipeline.h"
#include "pileup_call.h"
#include "pileup_walk.h"

namespace polyhip {
namespace {

enum : int { VINFO_EVENTS = QINFO_WORDS, VINFO_LONG, VINFO_OPEN, VINFO_EDGE, VINFO_SHIFTED, VINFO_MAXINS, VINFO_WORDS };
constexpr int KEY_LOW_BITS = 9; // length (8 bits, 1..255), kind (1 bit: 0 insertion, 1 deletion); the position above them
constexpr uint32_t COL_REVERSE = 1u << 31; // columns stay below 2^28

// EMIT == false: depth[j] and nsnv[j] (L + 1 slots for the scan) are written.
// EMIT == true: nsnv (now the offsets) is read and the position's SNV records are written behind the passing alleles of the
// positions before it: apos[0 .. *nalleles) ascend, passoff[a] = the passing alleles before allele a.
template <bool EMIT>
__global__ __launch_bounds__(BT) void snv_kernel(uint64_t lo, uint64_t L, uint32_t min_depth, uint32_t min_count, uint32_t permille, uint32_t hom,
                                                 const uint32_t *__restrict__ counts, const uint32_t *__restrict__ qsum,
                                                 const uint8_t *__restrict__ ref, uint32_t *depth_out, uint64_t *nsnv,
                                                 const uint32_t *__restrict__ apos, const uint32_t *__restrict__ nalleles,
                                                 const uint32_t *__restrict__ passoff, polyhip_variant *__restrict__ out)
{
    for (uint64_t j = (uint64_t)blockIdx.x * BT + threadIdx.x; j < L; j += (uint64_t)gridDim.x * BT) {
        if (EMIT && nsnv[j + 1] == nsnv[j])
            continue;
        uint32_t fwd[4], two[6]; // an entry adds at most one to a cell and n < 2^32: no sum below overflows
#pragma unroll
        for (uint32_t k = 0; k < 6; ++k) {
            const uint32_t f = counts[k * L + j];
            two[k] = f + counts[(CH_STRAND + k) * L + j];
            if (k < 4)
                fwd[k] = f;
        }
        uint32_t depth = 0;
#pragma unroll
        for (uint32_t k = 0; k < 6; ++k)
            depth += two[k];
        const bool deep = depth >= min_depth;
        const uint32_t rb = ref[lo + j], rc = base_class(rb);
        uint64_t at = 0;
        if (EMIT) {
            uint32_t a0 = 0, a1 = nalleles ? *nalleles : 0u; // the first allele at a position >= j
            while (a0 < a1) {
                const uint32_t mid = a0 + (a1 - a0) / 2;
                if (apos[mid] < j)
                    a0 = mid + 1;
                else
                    a1 = mid;
            }
            at = nsnv[j] + (passoff ? passoff[a0] : 0u);
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const bool is = deep && k != rc && two[k] >= min_count && (uint64_t)two[k] * 1000u >= (uint64_t)permille * depth;
            if (!is)
                continue;
            if (EMIT) {
                polyhip_variant x;
                x.allele_off = 0;
                x.pos = (uint32_t)(lo + j);
                x.depth = depth;
                x.count = two[k];
                x.count_fwd = fwd[k];
                x.ref_count = rc < 4 ? two[rc < 4 ? rc : 0] : 0u;
                x.qsum = qsum ? qsum[k * L + j] + qsum[(4 + k) * L + j] : 0u;
                x.allele_len = 1;
                x.kind = 1;
                x.ref = (uint8_t)rb;
                x.alt = (uint8_t)"ACGT"[k];
                x.gt = (uint64_t)two[k] * 1000u >= (uint64_t)hom * depth ? 2 : 1;
                out[at] = x;
            }
            ++at;
        }
        if (!EMIT) {
            depth_out[j] = depth;
            nsnv[j] = at;
        }
    }
}

// EMIT == false: cnt[i] = the kept events of entry i in the region; the info counters are added to.
// EMIT == true: cnt (now the offsets) is read and the items are written.
template <bool EMIT>
__global__ __launch_bounds__(BT) void event_kernel(Entries E, uint32_t left_align, uint32_t max_indel, uint64_t lo, uint64_t L, uint64_t *cnt,
                                                   uint64_t *mkey, uint32_t *val, uint32_t *ent, uint32_t *col, unsigned long long *info)
{
    const int lane = threadIdx.x & 63;
    const uint64_t off0 = E.alnOff[0];
    uint64_t n_events = 0, n_long = 0, n_open = 0, n_edge = 0, n_shifted = 0; // of this wave's entries, the same in every lane
    uint32_t max_ins = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * PU_WAVES + (threadIdx.x >> 6); i < E.n; i += (uint64_t)gridDim.x * PU_WAVES) {
        if (EMIT ? cnt[i + 1] == cnt[i] : !entry_used(E, i)) {
            if (!EMIT && lane == 0)
                cnt[i] = 0;
            continue;
        }
        const uint32_t ncols = (uint32_t)(E.alnOff[i + 1] - E.alnOff[i]);
        const uint8_t *a = E.alnA + (E.alnOff[i] - off0), *b = E.alnB + (E.alnOff[i] - off0);
        const uint32_t reverse = E.flags[i] & 2u ? COL_REVERSE : 0u;
        ColumnWalk S(E.ref_start[i], 0);
        uint64_t slot = 0; // the entry's items so far
        for (uint32_t base = 0; base < ncols; base += 64) {
            S.load(a, b, base, ncols, lane);
            const uint64_t sI = S.sI(), sD = S.sD();
            for (uint64_t starts = sI | sD; starts; starts &= starts - 1) { // the wave takes the step's runs one after the other
                const int e = __ffsll((unsigned long long)starts) - 1;
                const bool ins = sI >> e & 1ull;
                const uint32_t c0 = base + (uint32_t)e;
                const uint64_t pe = __shfl(S.p, e, 64);
                uint32_t l = 0; // the run's columns: the first column of another class ends it
                for (uint32_t o = 0;; o += 64) {
                    const uint32_t cc = c0 + o + lane;
                    const uint64_t other = ~__ballot(cc < ncols && (ins ? b[cc] : a[cc]) == '-');
                    if (other) {
                        l = o + (uint32_t)(__ffsll((unsigned long long)other) - 1);
                        break;
                    }
                    if (o >= POLYHIP_VAR_MAX_INDEL) { // 320 columns and no end: longer than any max_indel
                        l = o + 64;
                        break;
                    }
                }
                if (l > max_indel) {
                    ++n_long;
                    continue;
                }
                uint32_t k = 0;
                if (left_align) {
                    const uint8_t *x = ins ? a : b;
                    for (uint32_t tb = 0;; tb += 64) { // 64 steps t at a time; lanes with t >= c0 have no column and fail
                        const uint32_t t = tb + lane;
                        bool ok = false;
                        if (t < c0) {
                            const uint32_t cc = c0 - 1 - t;
                            const uint32_t xa = a[cc], xb = b[cc];
                            ok = xa != '-' && xb != '-' && fold(xa) == fold(xb) && fold(x[cc]) == fold(x[cc + l]);
                        }
                        const uint64_t fail = ~__ballot(ok);
                        if (fail) {
                            k = tb + (uint32_t)(__ffsll((unsigned long long)fail) - 1);
                            break;
                        }
                    }
                    if (k == c0) {
                        ++n_open;
                        continue;
                    }
                }
                if (pe < 1ull + k) { // anchor pe - 1 - k is -1
                    ++n_edge;
                    continue;
                }
                const uint64_t anchor = pe - 1 - k;
                ++n_events;
                n_shifted += k ? 1u : 0u;
                if (anchor - lo < L) { // anchor < lo wraps to a value above L
                    if (EMIT) {
                        if (lane == 0) {
                            const uint64_t t = cnt[i] + slot;
                            mkey[t] = (anchor - lo) << KEY_LOW_BITS | (ins ? 0u : 256u) | l;
                            val[t] = (uint32_t)t;
                            ent[t] = (uint32_t)i;
                            col[t] = (c0 - k) | reverse;
                        }
                    } else if (ins) {
                        max_ins = std::max(max_ins, l);
                    }
                    ++slot;
                }
            }
            S.advance();
        }
        if (!EMIT && lane == 0)
            cnt[i] = slot;
    }
    if (!EMIT && lane == 0) {
        if (n_events)
            atomicAdd(&info[VINFO_EVENTS], (unsigned long long)n_events);
        if (n_long)
            atomicAdd(&info[VINFO_LONG], (unsigned long long)n_long);
        if (n_open)
            atomicAdd(&info[VINFO_OPEN], (unsigned long long)n_open);
        if (n_edge)
            atomicAdd(&info[VINFO_EDGE], (unsigned long long)n_edge);
        if (n_shifted)
            atomicAdd(&info[VINFO_SHIFTED], (unsigned long long)n_shifted);
        if (max_ins)
            atomicMax(&info[VINFO_MAXINS], (unsigned long long)max_ins);
    }
}

struct Items {
    uint64_t N;
    const uint64_t *mkey; // by item
    const uint32_t *ent, *col;
    const uint8_t *alnA;
    const uint64_t *alnOff;
};

__device__ __forceinline__ const uint8_t *allele_of(const Items &I, uint32_t t)
{
    return I.alnA + (I.alnOff[I.ent[t]] - I.alnOff[0]) + (I.col[t] & ~COL_REVERSE);
}

// key[s] = bytes [8w, 8w + 8) of the allele of item val[s], big-endian, folded; 0 for a deletion and behind the allele's end
__global__ __launch_bounds__(BT) void wordkey_kernel(Items I, uint32_t w, const uint32_t *__restrict__ val, uint64_t *key)
{
    for (uint64_t s = (uint64_t)blockIdx.x * BT + threadIdx.x; s < I.N; s += (uint64_t)gridDim.x * BT) {
        const uint32_t t = val[s];
        const uint64_t mk = I.mkey[t];
        const uint32_t l = (uint32_t)mk & 255u;
        uint64_t word = 0;
        if (!(mk & 256u) && 8 * w < l) {
            const uint8_t *x = allele_of(I, t);
            for (uint32_t q = 8 * w; q < std::min(8 * w + 8, l); ++q)
                word |= (uint64_t)fold(x[q]) << (8 * (7 - (q - 8 * w)));
        }
        key[s] = word;
    }
}

__global__ __launch_bounds__(BT) void mainkey_kernel(Items I, const uint32_t *__restrict__ val, uint64_t *key)
{
    for (uint64_t s = (uint64_t)blockIdx.x * BT + threadIdx.x; s < I.N; s += (uint64_t)gridDim.x * BT)
        key[s] = I.mkey[val[s]];
}

// ah[s]: a new allele starts at sorted item s; sh[s]: a new site (pos, kind); fw[s]: the item is of strand 0
__global__ __launch_bounds__(BT) void head_kernel(Items I, const uint64_t *__restrict__ key, const uint32_t *__restrict__ val, uint32_t *ah,
                                                  uint32_t *sh, uint32_t *fw)
{
    for (uint64_t s = (uint64_t)blockIdx.x * BT + threadIdx.x; s < I.N; s += (uint64_t)gridDim.x * BT) {
        const uint32_t t = val[s];
        const uint64_t k = key[s];
        bool site = true, allele = true;
        if (s) {
            const uint64_t kp = key[s - 1];
            site = (k >> 8) != (kp >> 8);
            allele = k != kp;
            if (!allele && !(k & 256u)) { // two insertions of one length behind one position: all bytes
                const uint8_t *x = allele_of(I, t), *y = allele_of(I, val[s - 1]);
                const uint32_t l = (uint32_t)k & 255u;
                for (uint32_t q = 0; q < l && !allele; ++q)
                    allele = fold(x[q]) != fold(y[q]);
            }
        }
        ah[s] = allele;
        sh[s] = site;
        fw[s] = I.col[t] & COL_REVERSE ? 0u : 1u;
    }
}

// aidx, sidx: the exclusive scans of ah, sh (N + 1 values).  astart[a] = the first sorted item of allele a, astart[alleles] = N;
// sstart the same for the sites
__global__ __launch_bounds__(BT) void start_kernel(uint64_t N, const uint32_t *__restrict__ aidx, const uint32_t *__restrict__ sidx,
                                                   uint32_t *astart, uint32_t *sstart)
{
    for (uint64_t s = (uint64_t)blockIdx.x * BT + threadIdx.x; s < N; s += (uint64_t)gridDim.x * BT) {
        if (aidx[s + 1] != aidx[s])
            astart[aidx[s]] = (uint32_t)s;
        if (sidx[s + 1] != sidx[s])
            sstart[sidx[s]] = (uint32_t)s;
        if (s == N - 1) {
            astart[aidx[N]] = (uint32_t)N;
            sstart[sidx[N]] = (uint32_t)N;
        }
    }
}

struct Alleles {
    uint64_t lo, N;
    uint32_t min_depth, min_count, permille, hom;
    const uint64_t *key;                          // sorted
    const uint32_t *val;
    const uint32_t *aidx, *sidx, *fwoff;          // N + 1 each
    const uint32_t *astart, *sstart;
    const uint32_t *depth;
    const uint8_t *ref;
};

// EMIT == false: pass[a], nbytes[a] and apos[a] of every allele a < aidx[N].
// EMIT == true: pass and nbytes (now the offsets) are read; the passing alleles' records and pool bytes are written.
template <bool EMIT>
__global__ __launch_bounds__(BT) void allele_kernel(Alleles A, Items I, uint32_t *pass, uint64_t *nbytes, uint32_t *apos,
                                                    const uint64_t *__restrict__ snvoff, polyhip_variant *__restrict__ out,
                                                    uint8_t *__restrict__ pool)
{
    const uint64_t na = A.aidx[A.N];
    for (uint64_t a = (uint64_t)blockIdx.x * BT + threadIdx.x; a < na; a += (uint64_t)gridDim.x * BT) {
        if (EMIT && pass[a + 1] == pass[a])
            continue;
        const uint32_t s0 = A.astart[a], s1 = A.astart[a + 1];
        const uint64_t k = A.key[s0];
        const uint64_t j = k >> KEY_LOW_BITS;
        const bool del = k & 256u;
        const uint32_t l = (uint32_t)k & 255u, count = s1 - s0, depth = A.depth[j];
        if (!EMIT) {
            const bool is = depth >= A.min_depth && count >= A.min_count && (uint64_t)count * 1000u >= (uint64_t)A.permille * depth;
            pass[a] = is;
            nbytes[a] = is && !del ? l : 0u;
            apos[a] = (uint32_t)j;
            continue;
        }
        const uint32_t site = A.sidx[s0 + 1] - 1, site_events = A.sstart[site + 1] - A.sstart[site];
        polyhip_variant x;
        x.allele_off = del ? 0 : nbytes[a];
        x.pos = (uint32_t)(A.lo + j);
        x.depth = depth;
        x.count = count;
        x.count_fwd = A.fwoff[s1] - A.fwoff[s0];
        x.ref_count = depth - std::min(depth, site_events);
        x.qsum = 0;
        x.allele_len = l;
        x.kind = del ? 3 : 2;
        x.ref = A.ref[A.lo + j];
        x.alt = 0;
        x.gt = (uint64_t)count * 1000u >= (uint64_t)A.hom * depth ? 2 : 1;
        out[snvoff[j + 1] + pass[a]] = x;
        if (!del) {
            const uint8_t *src = allele_of(I, A.val[s0]);
            uint8_t *dst = pool + nbytes[a];
            for (uint32_t q = 0; q < l; ++q)
                dst[q] = (uint8_t)fold(src[q]);
        }
    }
}

thread_local polyhip_variants_info t_vinfo{};

} // namespace
} // namespace polyhip

using namespace polyhip;

extern "C" {

int polyhip_call_variants(const polyhip_variants_params *params, uint64_t n, const uint32_t *flags, const uint8_t *mapq,
                          const uint32_t *ref_start, const uint32_t *ref_end, const uint32_t *read_start, const uint8_t *alnA,
                          const uint8_t *alnB, const uint64_t *alnOff, const uint8_t *qual, const uint64_t *qualOff, const uint8_t *ref,
                          uint64_t ref_len, uint64_t *nvariants, polyhip_variant *variants, uint64_t variant_capacity,
                          uint64_t *nallele_bytes, uint8_t *alleles, uint64_t allele_capacity, uint32_t *err)
{
    const char *who = "polyhip_call_variants";
    PH_REQUIRE(params, "%s: null params", who);
    const polyhip_pileup_qual_params &pq = params->base;
    const polyhip_pileup_params &pb = pq.base;
    if (int rc = check_region(who, pb.region_lo, pb.region_hi, ref_len))
        return rc;
    PH_REQUIRE(pb.min_alt_permille <= 1000, "%s: min_alt_permille = %u, it is 0 to 1000", who, pb.min_alt_permille);
    if (int rc = check_qual_params(who, pq.min_base_qual, pq.qual_offset))
        return rc;
    PH_REQUIRE(params->hom_permille <= 1000, "%s: hom_permille = %u, it is 0 to 1000", who, params->hom_permille);
    PH_REQUIRE(params->max_indel <= POLYHIP_VAR_MAX_INDEL, "%s: max_indel = %u, it is 0 to %u", who, params->max_indel, POLYHIP_VAR_MAX_INDEL);
    PH_REQUIRE(params->pad == 0, "%s: pad = %u, it is 0", who, params->pad);
    const bool with_q = qual != nullptr;
    PH_REQUIRE(with_q || pq.min_base_qual == 0, "%s: min_base_qual = %u needs qual, which is null", who, pq.min_base_qual);
    if (with_q ? n > 0xFFFFFFFFull / MAX_Q : n >> 32 != 0)
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %llu entries, %s", who, (unsigned long long)n,
                         with_q ? "the quality sums are uint32 and hold fewer than 2^32 / 93 of them" : "the counts are uint32 and hold fewer than 2^32");
    PH_REQUIRE(pb.min_mapq == 0 || mapq, "%s: min_mapq = %u needs mapq, which is null", who, pb.min_mapq);
    const uint64_t lo = pb.region_lo, L = pb.region_hi - pb.region_lo;
    PH_REQUIRE(ref && nvariants && nallele_bytes && (variants || variant_capacity == 0) && (alleles || allele_capacity == 0), "%s: null argument",
               who);
    const Entries H{n, pb.min_mapq, flags, mapq, ref_start, ref_end, read_start, alnA, alnB, alnOff, qual, qualOff, err, nullptr};
    if (int rc = check_entries(who, H, with_q))
        return rc;
    const uint32_t max_indel = params->max_indel ? params->max_indel : POLYHIP_VAR_MAX_INDEL;
    t_vinfo = polyhip_variants_info{};
    *nvariants = 0;
    *nallele_bytes = 0;

    HostStreams &hs = host_streams();
    PH_HIP(hs.init());
    hipStream_t st = hs.s[0];
    Arena w;
    const EntryStage stage(w, H, ref_len, pb.min_mapq > 0, with_q);
    const size_t o_counts = w.reserve(POLYHIP_PILEUP_CHANNELS * L * 4), o_qsum = w.reserve(with_q ? POLYHIP_PILEUP_QSUM_PLANES * L * 4 : 0),
                 o_depth = w.reserve(L * 4), o_nsnv = w.reserve((L + 1) * 8), o_cnt = w.reserve((n + 1) * 8),
                 o_info = w.reserve(VINFO_WORDS * sizeof(unsigned long long)),
                 o_scan = w.reserve(std::max(scan_scratch_bytes<uint64_t>(L), scan_scratch_bytes<uint64_t>(n)));
    PH_HIP(w.buf.alloc(w.used));
    SyncOnExit sync(st);
    Entries E;
    PH_HIP(stage.upload(w, ref, st, E));
    unsigned long long *d_info = w.at<unsigned long long>(o_info);
    PH_HIP(hipMemsetAsync(d_info, 0, VINFO_WORDS * sizeof(unsigned long long), st));
    if (L) {
        PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_counts), 0, POLYHIP_PILEUP_CHANNELS * L * 4, st));
        if (with_q)
            PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_qsum), 0, POLYHIP_PILEUP_QSUM_PLANES * L * 4, st));
    }
    uint32_t *d_counts = w.at<uint32_t>(o_counts), *d_qsum = with_q ? w.at<uint32_t>(o_qsum) : nullptr, *d_depth = w.at<uint32_t>(o_depth);
    uint64_t *d_nsnv = w.at<uint64_t>(o_nsnv), *d_cnt = w.at<uint64_t>(o_cnt);
    const uint8_t *d_ref = stage.ref(w);
    const unsigned wgrid = grid_for(n, PU_WAVES, PU_MAX_BLOCKS);
    const WalkArgs W{lo, L, ref_len, d_ref, pq.min_base_qual, pq.qual_offset, d_counts, d_qsum, d_info};
    PH_HIP(walk_entries(E, W, false, with_q, st));
    // with L == 0 no add lands anywhere, but the filtered bases are still counted
    PH_HIP(walk_entries(E, W, true, with_q, st));
    const uint32_t min_depth = std::max(pb.min_depth, 1u), min_count = std::max(pb.min_alt_count, 1u);
    const unsigned lgrid = grid_for(L, BT, 1u << 20);
    if (L) {
        hipLaunchKernelGGL(snv_kernel<false>, dim3(lgrid), dim3(BT), 0, st, lo, L, min_depth, min_count, pb.min_alt_permille, params->hom_permille,
                           d_counts, d_qsum, d_ref, d_depth, d_nsnv, (const uint32_t *)nullptr, (const uint32_t *)nullptr,
                           (const uint32_t *)nullptr, (polyhip_variant *)nullptr);
        PH_HIP(hipGetLastError());
    }
    PH_HIP(scan_excl<uint64_t>(d_nsnv, d_nsnv, L, w.at<uint8_t>(o_scan), st));
    if (n) {
        hipLaunchKernelGGL(event_kernel<false>, dim3(wgrid), dim3(BT), 0, st, E, params->left_align, max_indel, lo, L, d_cnt, (uint64_t *)nullptr,
                           (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, d_info);
        PH_HIP(hipGetLastError());
    }
    PH_HIP(scan_excl<uint64_t>(d_cnt, d_cnt, n, w.at<uint8_t>(o_scan), st));
    unsigned long long info[VINFO_WORDS];
    uint64_t N = 0, nsnv = 0;
    if (n)
        PH_HIP(hipMemcpyAsync(err, E.err, n * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(&N, d_cnt + n, sizeof N, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(&nsnv, d_nsnv + L, sizeof nsnv, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    t_vinfo.entries = n;
    t_vinfo.used = info[INFO_USED];
    t_vinfo.skipped_mapq = info[INFO_SKIPPED];
    t_vinfo.bad = info[INFO_BAD];
    t_vinfo.columns = info[INFO_COLUMNS];
    t_vinfo.edge_events = info[VINFO_EDGE];
    t_vinfo.filtered_bases = with_q ? info[QINFO_FILTERED] : 0;
    t_vinfo.events = info[VINFO_EVENTS];
    t_vinfo.long_events = info[VINFO_LONG];
    t_vinfo.open_events = info[VINFO_OPEN];
    t_vinfo.shifted_events = info[VINFO_SHIFTED];
    if (N > 0xFFFFFFFFull)
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %llu events in the region, one call holds at most 2^32 - 1: split the region", who,
                         (unsigned long long)N);

    // the items, their sorts, the alleles
    Arena x;
    const uint64_t nb = radix_blocks(N);
    const size_t o_ka = x.reserve(N * 8), o_kb = x.reserve(N * 8), o_va = x.reserve(N * 4), o_vb = x.reserve(N * 4), o_mkey = x.reserve(N * 8),
                 o_ent = x.reserve(N * 4), o_col = x.reserve(N * 4), o_hist = x.reserve((256 * nb + 1) * 4),
                 o_rscan = x.reserve(scan_scratch_bytes<uint32_t>(256 * nb)), o_aidx = x.reserve((N + 1) * 4), o_sidx = x.reserve((N + 1) * 4),
                 o_fw = x.reserve((N + 1) * 4), o_astart = x.reserve((N + 1) * 4), o_sstart = x.reserve((N + 1) * 4),
                 o_pass = x.reserve((N + 1) * 4), o_nbytes = x.reserve((N + 1) * 8), o_apos = x.reserve(N * 4),
                 o_xscan = x.reserve(scan_scratch_bytes<uint64_t>(N));
    uint64_t npass = 0, pool_bytes = 0;
    uint32_t nalleles = 0;
    uint64_t *ka = nullptr, *kb = nullptr;
    uint32_t *va = nullptr, *vb = nullptr;
    const unsigned ngrid = grid_for(N, BT, 1u << 20);
    Items I{};
    Alleles A{};
    if (N) {
        PH_HIP(x.buf.alloc(x.used));
        ka = x.at<uint64_t>(o_ka), kb = x.at<uint64_t>(o_kb), va = x.at<uint32_t>(o_va), vb = x.at<uint32_t>(o_vb);
        I = Items{N, x.at<uint64_t>(o_mkey), x.at<uint32_t>(o_ent), x.at<uint32_t>(o_col), E.alnA, E.alnOff};
        hipLaunchKernelGGL(event_kernel<true>, dim3(wgrid), dim3(BT), 0, st, E, params->left_align, max_indel, lo, L, d_cnt, x.at<uint64_t>(o_mkey),
                           va, x.at<uint32_t>(o_ent), x.at<uint32_t>(o_col), d_info);
        PH_HIP(hipGetLastError());
        const uint32_t words = ((uint32_t)info[VINFO_MAXINS] + 7) / 8;
        for (uint32_t wd = words; wd-- > 0;) {
            hipLaunchKernelGGL(wordkey_kernel, dim3(ngrid), dim3(BT), 0, st, I, wd, va, ka);
            PH_HIP(hipGetLastError());
            if (int rc = radix_sort(ka, va, kb, vb, N, 64, x.at<uint32_t>(o_hist), x.at<uint8_t>(o_rscan), st))
                return rc;
        }
        hipLaunchKernelGGL(mainkey_kernel, dim3(ngrid), dim3(BT), 0, st, I, va, ka);
        PH_HIP(hipGetLastError());
        if (int rc = radix_sort(ka, va, kb, vb, N, KEY_LOW_BITS + bits_for(L - 1), x.at<uint32_t>(o_hist), x.at<uint8_t>(o_rscan), st))
            return rc;
        uint32_t *aidx = x.at<uint32_t>(o_aidx), *sidx = x.at<uint32_t>(o_sidx), *fw = x.at<uint32_t>(o_fw);
        hipLaunchKernelGGL(head_kernel, dim3(ngrid), dim3(BT), 0, st, I, ka, va, aidx, sidx, fw);
        PH_HIP(hipGetLastError());
        PH_HIP(scan_excl<uint32_t>(aidx, aidx, N, x.at<uint8_t>(o_xscan), st));
        PH_HIP(scan_excl<uint32_t>(sidx, sidx, N, x.at<uint8_t>(o_xscan), st));
        PH_HIP(scan_excl<uint32_t>(fw, fw, N, x.at<uint8_t>(o_xscan), st));
        hipLaunchKernelGGL(start_kernel, dim3(ngrid), dim3(BT), 0, st, N, aidx, sidx, x.at<uint32_t>(o_astart), x.at<uint32_t>(o_sstart));
        PH_HIP(hipGetLastError());
        A = Alleles{lo,   N,    min_depth, min_count, pb.min_alt_permille, params->hom_permille, ka, va, aidx, sidx, fw, x.at<uint32_t>(o_astart),
                    x.at<uint32_t>(o_sstart), d_depth, d_ref};
        // the slots behind the last allele count as alleles that do not pass
        PH_HIP(hipMemsetAsync(x.at<uint8_t>(o_pass), 0, (N + 1) * 4, st));
        PH_HIP(hipMemsetAsync(x.at<uint8_t>(o_nbytes), 0, (N + 1) * 8, st));
        hipLaunchKernelGGL(allele_kernel<false>, dim3(ngrid), dim3(BT), 0, st, A, I, x.at<uint32_t>(o_pass), x.at<uint64_t>(o_nbytes),
                           x.at<uint32_t>(o_apos), (const uint64_t *)nullptr, (polyhip_variant *)nullptr, (uint8_t *)nullptr);
        PH_HIP(hipGetLastError());
        PH_HIP(scan_excl<uint32_t>(x.at<uint32_t>(o_pass), x.at<uint32_t>(o_pass), N, x.at<uint8_t>(o_xscan), st));
        PH_HIP(scan_excl<uint64_t>(x.at<uint64_t>(o_nbytes), x.at<uint64_t>(o_nbytes), N, x.at<uint8_t>(o_xscan), st));
        uint32_t np32 = 0;
        PH_HIP(hipMemcpyAsync(&nalleles, aidx + N, 4, hipMemcpyDeviceToHost, st));
        PH_HIP(hipMemcpyAsync(&np32, x.at<uint32_t>(o_pass) + N, 4, hipMemcpyDeviceToHost, st));
        PH_HIP(hipMemcpyAsync(&pool_bytes, x.at<uint64_t>(o_nbytes) + N, 8, hipMemcpyDeviceToHost, st));
        PH_HIP(hipStreamSynchronize(st));
        npass = np32;
    }
    const uint64_t total = nsnv + npass;
    *nvariants = total;
    *nallele_bytes = pool_bytes;
    t_vinfo.sites = total;
    t_vinfo.alleles = nalleles;
    t_vinfo.allele_bytes = pool_bytes;
    if (total > variant_capacity)
        return set_error(POLYHIP_ERR_INVALID, "%s: the variants need %llu entries, the buffer holds %llu", who, (unsigned long long)total,
                         (unsigned long long)variant_capacity);
    if (pool_bytes > allele_capacity)
        return set_error(POLYHIP_ERR_INVALID, "%s: the alleles need %llu bytes, the buffer holds %llu", who, (unsigned long long)pool_bytes,
                         (unsigned long long)allele_capacity);
    if (total == 0)
        return POLYHIP_OK;
    // only now, bounded by the caller's capacities: the records and the pool
    DevBuf dvar, dpool;
    PH_HIP(dvar.alloc(total * sizeof(polyhip_variant)));
    PH_HIP(dpool.alloc(pool_bytes));
    SyncOnExit sync_out(st);
    if (nsnv) {
        hipLaunchKernelGGL(snv_kernel<true>, dim3(lgrid), dim3(BT), 0, st, lo, L, min_depth, min_count, pb.min_alt_permille, params->hom_permille,
                           d_counts, d_qsum, d_ref, d_depth, d_nsnv, N ? x.at<uint32_t>(o_apos) : nullptr, N ? x.at<uint32_t>(o_aidx) + N : nullptr,
                           N ? x.at<uint32_t>(o_pass) : nullptr, dvar.as<polyhip_variant>());
        PH_HIP(hipGetLastError());
    }
    if (npass) {
        hipLaunchKernelGGL(allele_kernel<true>, dim3(ngrid), dim3(BT), 0, st, A, I, x.at<uint32_t>(o_pass), x.at<uint64_t>(o_nbytes),
                           x.at<uint32_t>(o_apos), d_nsnv, dvar.as<polyhip_variant>(), dpool.as<uint8_t>());
        PH_HIP(hipGetLastError());
    }
    PH_HIP(hipMemcpyAsync(variants, dvar.p, total * sizeof(polyhip_variant), hipMemcpyDeviceToHost, st));
    if (pool_bytes)
        PH_HIP(hipMemcpyAsync(alleles, dpool.p, pool_bytes, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    return POLYHIP_OK;
}

int polyhip_call_variants_last_info(polyhip_variants_info *info)
{
    PH_REQUIRE(info, "polyhip_call_variants_last_info: null argument");
    *info = t_vinfo;
    return POLYHIP_OK;
}

} // extern "C"
