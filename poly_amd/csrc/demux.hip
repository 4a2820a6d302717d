// demux.hip -- polyhip_demux_reads and polyhip_demux_pairs: the inline 5' barcode of every read of a pooled batch, and the batch
// grouped by sample.  The definition is the comment above the calls in include/polyhip.h; tests/demux_oracle.py restates it in
// plain Python.  All of it is integer work and no atomic decides an output byte.
//
//   match_kernel    one wave per read (grid-stride), steps 1-3 of the definition.  The first 128 bytes of the read are taken
//                   once, as eight ballots: for each of A, C, G, T the 128 positions that hold it (either case); they are the
//                   same in every lane, so the 64 positions from a start s on are scalar shifts.  A barcode is four such masks
//                   made by the host.  A lane takes every 64th barcode: it loads the four masks once, walks the starts 0 ..
//                   max_shift (four ANDs and a population count each) and keeps its own best (mismatches, barcode, start) and
//                   the best of its other barcodes in registers.  Nothing crosses lanes until the end, where the wave's
//                   minimum over (mismatches, barcode, start) is the choice and a second minimum, over each lane's best unless
//                   that is the chosen barcode and else its runner-up, is d2
//   assign_kernel   a lane per read or pair: the sample (pairs: the table), flags bit 2, the group key of the sort, the bytes
//                   each entry loses to the clip, the info counters
//   radix_sort      (device_prims.h) stable, by the group key alone, the index as the value: order
//   starts_kernel   a lane per group: sample_start by binary search in the sorted keys
//   place_kernel    a lane per output read: its kept length, in output order
//   scan_excl       (device_prims.h) the kept lengths -> out_off, per mate
//   gather_kernel   one wave per output read: r[a, m) and the same slice of its quality string to their places
#include "host_pipeline.h"
#include "read_batch.h"

namespace polyhip {
namespace {

constexpr int DX_WAVES = BT / 64; // reads a block works on at a time
constexpr uint32_t MAX_BARCODES = 4096, MIN_BARCODE = 4, MAX_BARCODE = 64, MAX_SHIFT = 63, MAX_SAMPLES = 65536;
constexpr uint32_t MAX_READ = 1u << 24; // as the trimmer's, whose batches these are; clip_extra stays below it too
constexpr uint32_t NONE = 0xFFFFFFFFu;
enum : uint32_t { F_NO_BARCODE = 1u, F_AMBIGUOUS = 2u, F_NOT_IN_SHEET = 4u };
enum : int { I_ASSIGNED = 0, I_EXACT = 1, I_NO_BARCODE = 2, I_AMBIGUOUS = 3, I_NOT_IN_SHEET = 4, I_BAD = 5, N_INFO = 6 };

struct Knobs {
    uint32_t max_shift, max_mismatches, min_margin, nbarcodes; // nbarcodes == 0: this mate is not judged against a set
};

// a barcode set on the device: barcode t has len[t] bytes; bit k of mask[4 * t + c] says that its byte k is "ACGT"[c]
struct DevSet {
    const uint64_t *mask;
    const uint32_t *len;
    uint32_t n;
};

__device__ __forceinline__ uint32_t wave_min(uint32_t v) { return ~dpp_wave_max(~v); }

// Steps 1-3 for read i of the batch; entry e = i * stride + phase of barcode / bstart / mism / flags / err (pairs: stride 2,
// phase = mate)
__global__ __launch_bounds__(BT) void match_kernel(uint64_t n, Knobs kn, DevBatch in, DevSet set, uint32_t stride, uint32_t phase,
                                                   uint32_t *__restrict__ barcode, uint32_t *__restrict__ bstart,
                                                   uint32_t *__restrict__ mism, uint32_t *__restrict__ flags,
                                                   uint32_t *__restrict__ err)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t off0 = in.off[0];
    for (uint64_t i = (uint64_t)blockIdx.x * DX_WAVES + (threadIdx.x >> 6); i < n; i += (uint64_t)gridDim.x * DX_WAVES) {
        const uint32_t m = (uint32_t)(in.off[i + 1] - in.off[i]);
        const uint8_t *r = in.reads + (in.off[i] - off0);
        // 1. judging: the lengths alone
        const uint32_t e = in.qual && in.qual_off[i + 1] - in.qual_off[i] != (uint64_t)m ? 1u : 0u;
        uint32_t best = NONE, best_t = NONE, best_s = NONE, second = NONE;
        if (e == 0 && kn.nbarcodes) {
            // 2. the read's first 128 bytes as four masks of 128 positions, the same in every lane
            const uint32_t c1 = lane + 64;
            const uint32_t x0 = lane < m ? base_code(r[lane]) : 0u, x1 = c1 < m ? base_code(r[c1]) : 0u;
            uint64_t lo[4], hi[4]; // bit k: byte k (k + 64) of the read is "ACGT"[c]
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t letter = "ACGT"[c];
                lo[c] = __ballot(x0 == letter);
                hi[c] = __ballot(x1 == letter);
            }
            const uint32_t last = kn.max_shift < m ? kn.max_shift : m; // no barcode fits behind it
            // this lane's barcodes in ascending order, each at the starts in ascending order: of equal distances the earlier
            // stays.  my: the best of them, my_2nd: the best of the others
            uint32_t my = NONE, my_t = 0, my_s = 0, my_2nd = NONE;
            for (uint32_t t = lane; t < kn.nbarcodes; t += 64) {
                const uint32_t p = set.len[t];
                const uint64_t *mk = set.mask + 4 * (uint64_t)t;
                const uint64_t m0 = mk[0], m1 = mk[1], m2 = mk[2], m3 = mk[3]; // loaded once for all the starts
                const uint64_t first_p = p >= 64 ? ~0ull : (1ull << p) - 1ull;
                uint32_t dt = NONE, st = 0;
                for (uint32_t s = 0; s <= last; ++s) { // the same s in every lane: the shifted masks are scalar work
                    uint64_t W[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        W[c] = s ? lo[c] >> s | hi[c] << (64 - s) : lo[c];
                    const uint64_t same = (W[0] & m0) | (W[1] & m1) | (W[2] & m2) | (W[3] & m3);
                    const uint32_t d = s + p <= m ? p - (uint32_t)__popcll(same & first_p) : NONE;
                    if (d < dt) {
                        dt = d;
                        st = s;
                    }
                }
                if (dt < my) {
                    my_2nd = my;
                    my = dt;
                    my_t = t;
                    my_s = st;
                } else if (dt < my_2nd) {
                    my_2nd = dt;
                }
            }
            // 3. the wave's smallest (d, barcode, start); d <= 64, barcode < 4096, start < 64
            const uint32_t top = wave_min(my != NONE ? my << 18 | my_t << 6 | my_s : NONE);
            if (top != NONE) {
                best = top >> 18;
                best_t = top >> 6 & 0xFFFu;
                best_s = top & 63u;
                // d2: the chosen barcode's lane gives the best of its other barcodes, every other lane its best
                second = wave_min(my_t != best_t ? my : my_2nd);
            }
        }
        if (lane == 0) {
            uint32_t f = 0;
            if (e == 0 && kn.nbarcodes) {
                if (best == NONE || best > kn.max_mismatches)
                    f = F_NO_BARCODE;
                else if (second != NONE && second - best < kn.min_margin)
                    f = F_AMBIGUOUS;
            }
            const bool has = e == 0 && kn.nbarcodes && f == 0;
            const uint64_t at = i * stride + phase;
            barcode[at] = has ? best_t : NONE;
            bstart[at] = has ? best_s : NONE;
            mism[at] = has ? best : NONE;
            flags[at] = f;
            err[at] = e;
        }
    }
}

// Steps 4 and 5 for read or pair i (nb = 1 or 2 entries): sample, flags bit 2, the key and value of the sort, the clip of each
// entry, the counters
__global__ __launch_bounds__(BT) void assign_kernel(uint64_t n, uint32_t nb, uint32_t nsamples, uint32_t clip, uint32_t clip_extra,
                                                    DevBatch in1, DevBatch in2, DevSet set1, DevSet set2,
                                                    const uint32_t *__restrict__ pair_sample, const uint32_t *__restrict__ barcode,
                                                    const uint32_t *__restrict__ bstart, const uint32_t *__restrict__ mism,
                                                    uint32_t *__restrict__ flags, const uint32_t *__restrict__ err,
                                                    uint32_t *__restrict__ sample, uint64_t *__restrict__ key, uint32_t *__restrict__ val,
                                                    uint32_t *__restrict__ cut, unsigned long long *info)
{
    __shared__ uint32_t s_info[N_INFO];
    if (threadIdx.x < N_INFO)
        s_info[threadIdx.x] = 0;
    __syncthreads();
    uint32_t cnt[N_INFO] = {0, 0, 0, 0, 0, 0};
    const uint64_t rounds = (n + (uint64_t)gridDim.x * BT - 1) / ((uint64_t)gridDim.x * BT); // whole waves stay together
    for (uint64_t k = 0; k < rounds; ++k) {
        const uint64_t i = (k * gridDim.x + blockIdx.x) * BT + threadIdx.x;
        if (i < n) {
            const uint64_t at = i * nb;
            const uint32_t b1 = barcode[at], b2 = nb == 2 ? barcode[at + 1] : NONE;
            const uint32_t bad1 = err[at], bad2 = nb == 2 ? err[at + 1] : 0u;
            bool ok = !bad1 && !bad2 && b1 != NONE && (set2.n == 0 || b2 != NONE);
            uint32_t smp = NONE, f1 = flags[at], f2 = nb == 2 ? flags[at + 1] : 0u;
            if (ok) {
                smp = set2.n ? pair_sample[(uint64_t)b1 * set2.n + b2] : b1;
                if (smp == NONE) {
                    ok = false;
                    f1 |= F_NOT_IN_SHEET;
                    f2 |= F_NOT_IN_SHEET;
                    flags[at] = f1;
                    flags[at + 1] = f2; // a table is a pair's
                }
            }
            sample[i] = smp;
            key[i] = ok ? (uint64_t)smp : (uint64_t)nsamples;
            val[i] = (uint32_t)i;
            const uint32_t m1 = (uint32_t)(in1.off[i + 1] - in1.off[i]);
            uint32_t a1 = ok && clip ? bstart[at] + set1.len[b1] + clip_extra : 0u; // < 64 + 64 + 2^24
            cut[at] = bad1 ? m1 : a1 < m1 ? a1 : m1;
            if (nb == 2) {
                const uint32_t m2 = (uint32_t)(in2.off[i + 1] - in2.off[i]);
                uint32_t a2 = ok && clip && b2 != NONE ? bstart[at + 1] + set2.len[b2] + clip_extra : 0u;
                cut[at + 1] = bad2 ? m2 : a2 < m2 ? a2 : m2;
            }
            cnt[I_ASSIGNED] += ok ? nb : 0u;
            cnt[I_EXACT] += (b1 != NONE && mism[at] == 0 ? 1u : 0u) + (b2 != NONE && mism[at + 1] == 0 ? 1u : 0u);
            cnt[I_NO_BARCODE] += (f1 & F_NO_BARCODE ? 1u : 0u) + (f2 & F_NO_BARCODE ? 1u : 0u);
            cnt[I_AMBIGUOUS] += (f1 & F_AMBIGUOUS ? 1u : 0u) + (f2 & F_AMBIGUOUS ? 1u : 0u);
            cnt[I_NOT_IN_SHEET] += (f1 & F_NOT_IN_SHEET ? 1u : 0u) + (f2 & F_NOT_IN_SHEET ? 1u : 0u);
            cnt[I_BAD] += (bad1 ? 1u : 0u) + (bad2 ? 1u : 0u);
        }
    }
#pragma unroll
    for (int c = 0; c < N_INFO; ++c)
        add_info(s_info, c, cnt[c]);
    __syncthreads(); // one atomic per block and counter that has something
    if (threadIdx.x < N_INFO && s_info[threadIdx.x])
        atomicAdd(&info[threadIdx.x], (unsigned long long)s_info[threadIdx.x]);
}

// sample_start[k] = the number of sorted keys below k, k = 0..nsamples + 1
__global__ __launch_bounds__(BT) void starts_kernel(uint64_t n, uint32_t nsamples, const uint64_t *__restrict__ sorted,
                                                    uint64_t *__restrict__ sample_start)
{
    const uint32_t k = blockIdx.x * BT + threadIdx.x;
    if (k > nsamples + 1)
        return;
    uint64_t lo = 0, hi = n; // the first j with sorted[j] >= k
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (sorted[mid] < (uint64_t)k)
            lo = mid + 1;
        else
            hi = mid;
    }
    sample_start[k] = lo;
}

// kept[j] = what output read j keeps, for the scan
__global__ __launch_bounds__(BT) void place_kernel(uint64_t n, DevBatch in, uint32_t stride, uint32_t phase,
                                                   const uint32_t *__restrict__ order, const uint32_t *__restrict__ cut,
                                                   uint64_t *__restrict__ kept)
{
    for (uint64_t j = (uint64_t)blockIdx.x * BT + threadIdx.x; j < n; j += (uint64_t)gridDim.x * BT) {
        const uint64_t i = order[j];
        kept[j] = (in.off[i + 1] - in.off[i]) - (uint64_t)cut[i * stride + phase];
    }
}

// output read j is input read order[j] without its first cut bytes, and the same of its quality string
__global__ __launch_bounds__(BT) void gather_kernel(uint64_t n, DevBatch in, uint32_t stride, uint32_t phase,
                                                    const uint32_t *__restrict__ order, const uint32_t *__restrict__ cut,
                                                    const uint64_t *__restrict__ out_off, uint8_t *__restrict__ out_reads,
                                                    uint8_t *__restrict__ out_qual)
{
    const int lane = threadIdx.x & 63;
    const uint64_t off0 = in.off[0], qoff0 = in.qual ? in.qual_off[0] : 0;
    for (uint64_t j = (uint64_t)blockIdx.x * DX_WAVES + (threadIdx.x >> 6); j < n; j += (uint64_t)gridDim.x * DX_WAVES) {
        const uint64_t dst = out_off[j], len = out_off[j + 1] - dst;
        if (len == 0)
            continue;
        const uint64_t i = order[j];
        const uint32_t a = cut[i * stride + phase];
        const uint8_t *r = in.reads + (in.off[i] - off0) + a;
        for (uint64_t c = lane; c < len; c += 64)
            out_reads[dst + c] = r[c];
        if (in.qual) {
            const uint8_t *q = in.qual + (in.qual_off[i] - qoff0) + a; // a kept read's quality string is as long as the read
            for (uint64_t c = lane; c < len; c += 64)
                out_qual[dst + c] = q[c];
        }
    }
}

// a barcode set as the caller hands it over
struct HostSet {
    const uint8_t *bytes;
    const uint32_t *off;
    uint32_t n;
};

thread_local polyhip_demux_info t_info{};

// both calls: nb = 1 (entry i is read i) or 2 (entries 2i, 2i + 1 are the mates of pair i)
int demux_batches(const char *who, const polyhip_demux_params *params, const HostSet *sets, const uint32_t *pair_sample, HostBatch *hb,
                  int nb, uint64_t n, uint32_t *barcode, uint32_t *bstart, uint32_t *mism, uint32_t *flags, uint32_t *err,
                  uint32_t *sample, uint32_t *order, uint64_t *sample_start)
{
    PH_REQUIRE(params, "%s: null params", who);
    const polyhip_demux_params &p = *params;
    PH_REQUIRE(p.max_shift <= MAX_SHIFT, "%s: max_shift = %u, at most %u", who, p.max_shift, MAX_SHIFT);
    PH_REQUIRE(p.max_mismatches <= MAX_BARCODE, "%s: max_mismatches = %u, a barcode has at most %u bytes", who, p.max_mismatches,
               MAX_BARCODE);
    PH_REQUIRE(p.clip <= 1, "%s: clip = %u, it is 0 or 1", who, p.clip);
    PH_REQUIRE(p.clip_extra < MAX_READ, "%s: clip_extra = %u, it stays below 2^24", who, p.clip_extra);
    PH_REQUIRE(p.nsamples >= 1 && p.nsamples <= MAX_SAMPLES, "%s: nsamples = %u, it is 1..%u", who, p.nsamples, MAX_SAMPLES);
    PH_REQUIRE(sets[0].n >= 1 && sets[0].n <= MAX_BARCODES, "%s: %u barcodes, a set holds 1..%u", who, sets[0].n, MAX_BARCODES);
    PH_REQUIRE(nb == 1 || sets[1].n <= MAX_BARCODES, "%s: %u barcodes in set 2, at most %u", who, sets[1].n, MAX_BARCODES);
    for (int q = 0; q < nb; ++q) {
        const HostSet &b = sets[q];
        PH_REQUIRE(b.n == 0 || (b.bytes && b.off), "%s: null barcodes (set %d)", who, q + 1);
        for (uint32_t t = 0; t < b.n; ++t) {
            const uint32_t len = b.off[t + 1] >= b.off[t] ? b.off[t + 1] - b.off[t] : 0u;
            PH_REQUIRE(len >= MIN_BARCODE && len <= MAX_BARCODE, "%s: barcode %u of set %d has %u bytes, a barcode has %u..%u", who, t, q + 1,
                       len, MIN_BARCODE, MAX_BARCODE);
            for (uint32_t k = 0; k < len; ++k) {
                const uint8_t c = b.bytes[b.off[t] + k];
                PH_REQUIRE(c == 'A' || c == 'C' || c == 'G' || c == 'T',
                           "%s: barcode %u of set %d has byte 0x%02x at %u, barcodes are upper-case ACGT", who, t, q + 1, c, k);
            }
        }
    }
    const bool table = nb == 2 && sets[1].n > 0;
    PH_REQUIRE(table || p.nsamples == sets[0].n, "%s: nsamples = %u, but without a table the %u barcodes are the samples", who, p.nsamples,
               sets[0].n);
    if (table) {
        PH_REQUIRE(pair_sample, "%s: null pair_sample", who);
        const uint64_t cells = (uint64_t)sets[0].n * sets[1].n;
        for (uint64_t c = 0; c < cells; ++c)
            PH_REQUIRE(pair_sample[c] < p.nsamples || pair_sample[c] == NONE, "%s: pair_sample[%llu] = %u, nsamples is %u", who,
                       (unsigned long long)c, pair_sample[c], p.nsamples);
    }
    const bool with_qual = hb[0].qual != nullptr;
    for (int q = 0; q < nb; ++q)
        PH_REQUIRE((hb[q].qual != nullptr) == (hb[q].qual_off != nullptr) && (hb[q].qual != nullptr) == (hb[q].out_qual != nullptr),
                   "%s: qual, qual_off and out_qual come together or not at all", who);
    PH_REQUIRE(nb == 1 || (hb[1].qual != nullptr) == with_qual, "%s: qualities of one mate only", who);
    PH_REQUIRE(barcode && bstart && mism && flags && err && sample && order && sample_start, "%s: null argument", who);
    for (int q = 0; q < nb; ++q)
        PH_REQUIRE(hb[q].out_reads && hb[q].out_off && (n == 0 || (hb[q].reads && hb[q].off)), "%s: null argument", who);
    for (int q = 0; q < nb; ++q)
        for (uint64_t i = 0; i < n; ++i)
            PH_REQUIRE(hb[q].off[i + 1] >= hb[q].off[i] && (!with_qual || hb[q].qual_off[i + 1] >= hb[q].qual_off[i]),
                       "%s: offsets are not ascending", who);
    for (int q = 0; q < nb; ++q)
        for (uint64_t i = 0; i < n; ++i)
            if (hb[q].off[i + 1] - hb[q].off[i] >= MAX_READ)
                return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: read %llu has %llu bytes, a read holds fewer than 2^24", who,
                                 (unsigned long long)i, (unsigned long long)(hb[q].off[i + 1] - hb[q].off[i]));
    if (n >> 32)
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %llu reads, order holds 32-bit indices", who, (unsigned long long)n);
    t_info = polyhip_demux_info{};
    if (n == 0) {
        for (int q = 0; q < nb; ++q)
            hb[q].out_off[0] = 0;
        std::fill(sample_start, sample_start + p.nsamples + 2, 0ull);
        return POLYHIP_OK;
    }

    HostStreams &hs = host_streams();
    PH_HIP(hs.init());
    hipStream_t st = hs.s[0];
    const uint64_t entries = n * (uint64_t)nb, sblocks = radix_blocks(n);
    uint64_t rbytes[2] = {0, 0}, qbytes[2] = {0, 0};
    size_t o_reads[2], o_off[2], o_qual[2], o_qoff[2], o_oreads[2], o_oqual[2], o_mask[2] = {0, 0}, o_len[2] = {0, 0};
    Arena w;
    for (int q = 0; q < nb; ++q) {
        rbytes[q] = hb[q].off[n] - hb[q].off[0];
        qbytes[q] = with_qual ? hb[q].qual_off[n] - hb[q].qual_off[0] : 0;
        o_reads[q] = w.reserve(rbytes[q]);
        o_off[q] = w.reserve((n + 1) * 8);
        o_qual[q] = w.reserve(qbytes[q]);
        o_qoff[q] = w.reserve(with_qual ? (n + 1) * 8 : 0);
        o_oreads[q] = w.reserve(rbytes[q]);
        o_oqual[q] = w.reserve(with_qual ? rbytes[q] : 0);
        o_mask[q] = w.reserve((size_t)sets[q].n * 32);
        o_len[q] = w.reserve((size_t)sets[q].n * 4);
    }
    const uint64_t cells = table ? (uint64_t)sets[0].n * sets[1].n : 0;
    const size_t o_table = w.reserve(cells * 4), o_kept = w.reserve((n + 1) * 8 * nb), o_barcode = w.reserve(entries * 4),
                 o_bstart = w.reserve(entries * 4), o_mism = w.reserve(entries * 4), o_flags = w.reserve(entries * 4),
                 o_err = w.reserve(entries * 4), o_cut = w.reserve(entries * 4), o_sample = w.reserve(n * 4), o_ka = w.reserve(n * 8),
                 o_kb = w.reserve(n * 8), o_va = w.reserve(n * 4), o_vb = w.reserve(n * 4), o_hist = w.reserve((256 * sblocks + 1) * 4),
                 o_scan = w.reserve(std::max(scan_scratch_bytes<uint64_t>(n), scan_scratch_bytes<uint32_t>(256 * sblocks))),
                 o_starts = w.reserve(((size_t)p.nsamples + 2) * 8), o_info = w.reserve(N_INFO * 8);
    PH_HIP(w.buf.alloc(w.used));
    SyncOnExit sync(st);
    std::vector<uint64_t> mask[2]; // per barcode and letter of ACGT: the positions that hold it
    std::vector<uint32_t> len[2];
    DevSet ds[2] = {{nullptr, nullptr, 0}, {nullptr, nullptr, 0}};
    for (int q = 0; q < nb; ++q) {
        const HostSet &b = sets[q];
        if (b.n == 0)
            continue;
        mask[q].assign(4 * (size_t)b.n, 0);
        len[q].assign(b.n, 0);
        for (uint32_t t = 0; t < b.n; ++t) {
            len[q][t] = b.off[t + 1] - b.off[t];
            for (uint32_t k = 0; k < len[q][t]; ++k) {
                const uint8_t c = b.bytes[b.off[t] + k];
                mask[q][4 * t + (c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3)] |= 1ull << k;
            }
        }
        PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_mask[q]), mask[q].data(), (size_t)b.n * 32, hipMemcpyHostToDevice, st));
        PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_len[q]), len[q].data(), (size_t)b.n * 4, hipMemcpyHostToDevice, st));
        ds[q] = DevSet{w.at<uint64_t>(o_mask[q]), w.at<uint32_t>(o_len[q]), b.n};
    }
    if (table)
        PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_table), pair_sample, cells * 4, hipMemcpyHostToDevice, st));
    PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_info), 0, N_INFO * 8, st));
    DevBatch db[2] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};
    for (int q = 0; q < nb; ++q) {
        if (rbytes[q])
            PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_reads[q]), hb[q].reads + hb[q].off[0], rbytes[q], hipMemcpyHostToDevice, st));
        PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_off[q]), hb[q].off, (n + 1) * 8, hipMemcpyHostToDevice, st));
        if (qbytes[q])
            PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_qual[q]), hb[q].qual + hb[q].qual_off[0], qbytes[q], hipMemcpyHostToDevice, st));
        if (with_qual)
            PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_qoff[q]), hb[q].qual_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
        db[q] = DevBatch{w.at<uint8_t>(o_reads[q]), with_qual ? w.at<uint8_t>(o_qual[q]) : nullptr, w.at<uint64_t>(o_off[q]),
                         with_qual ? w.at<uint64_t>(o_qoff[q]) : nullptr};
    }
    uint32_t *d_barcode = w.at<uint32_t>(o_barcode), *d_bstart = w.at<uint32_t>(o_bstart), *d_mism = w.at<uint32_t>(o_mism),
             *d_flags = w.at<uint32_t>(o_flags), *d_err = w.at<uint32_t>(o_err), *d_cut = w.at<uint32_t>(o_cut),
             *d_sample = w.at<uint32_t>(o_sample);
    unsigned long long *d_info = w.at<unsigned long long>(o_info);
    uint64_t *d_kept = w.at<uint64_t>(o_kept), *d_starts = w.at<uint64_t>(o_starts);

    const unsigned wgrid = grid_for(n, DX_WAVES, 256 * 32), lgrid = grid_for(n, BT, 512);
    for (int q = 0; q < nb; ++q) {
        const Knobs kn{p.max_shift, p.max_mismatches, p.min_margin, ds[q].n};
        hipLaunchKernelGGL(match_kernel, dim3(wgrid), dim3(BT), 0, st, n, kn, db[q], ds[q], (uint32_t)nb, (uint32_t)q, d_barcode, d_bstart,
                           d_mism, d_flags, d_err);
        PH_HIP(hipGetLastError());
    }
    uint64_t *ka = w.at<uint64_t>(o_ka), *kb = w.at<uint64_t>(o_kb);
    uint32_t *va = w.at<uint32_t>(o_va), *vb = w.at<uint32_t>(o_vb);
    hipLaunchKernelGGL(assign_kernel, dim3(lgrid), dim3(BT), 0, st, n, (uint32_t)nb, p.nsamples, p.clip, p.clip_extra, db[0], db[1], ds[0],
                       ds[1], table ? w.at<uint32_t>(o_table) : (const uint32_t *)nullptr, d_barcode, d_bstart, d_mism, d_flags, d_err,
                       d_sample, ka, va, d_cut, d_info);
    PH_HIP(hipGetLastError());
    const int rc = radix_sort(ka, va, kb, vb, n, bits_for(p.nsamples), w.at<uint32_t>(o_hist), w.at<uint8_t>(o_scan), st);
    if (rc != POLYHIP_OK)
        return rc;
    hipLaunchKernelGGL(starts_kernel, dim3(grid_for((uint64_t)p.nsamples + 2)), dim3(BT), 0, st, n, p.nsamples, ka, d_starts);
    PH_HIP(hipGetLastError());
    for (int q = 0; q < nb; ++q) {
        uint64_t *d_ooff = d_kept + (uint64_t)q * (n + 1); // scanned in place
        hipLaunchKernelGGL(place_kernel, dim3(lgrid), dim3(BT), 0, st, n, db[q], (uint32_t)nb, (uint32_t)q, va, d_cut, d_ooff);
        PH_HIP(hipGetLastError());
        PH_HIP(scan_excl<uint64_t>(d_ooff, d_ooff, n, w.at<uint8_t>(o_scan), st));
        hipLaunchKernelGGL(gather_kernel, dim3(wgrid), dim3(BT), 0, st, n, db[q], (uint32_t)nb, (uint32_t)q, va, d_cut, d_ooff,
                           w.at<uint8_t>(o_oreads[q]), with_qual ? w.at<uint8_t>(o_oqual[q]) : (uint8_t *)nullptr);
        PH_HIP(hipGetLastError());
        PH_HIP(hipMemcpyAsync(hb[q].out_off, d_ooff, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    }
    unsigned long long info[N_INFO];
    PH_HIP(hipMemcpyAsync(barcode, d_barcode, entries * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(bstart, d_bstart, entries * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(mism, d_mism, entries * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(flags, d_flags, entries * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(err, d_err, entries * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(sample, d_sample, n * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(order, va, n * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(sample_start, d_starts, ((size_t)p.nsamples + 2) * 8, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st)); // out_off[n] says how many bytes were kept
    uint64_t bytes_in = 0, bytes_out = 0;
    for (int q = 0; q < nb; ++q) {
        const uint64_t kept = hb[q].out_off[n];
        bytes_in += rbytes[q];
        bytes_out += kept;
        if (kept) {
            PH_HIP(hipMemcpyAsync(hb[q].out_reads, w.at<uint8_t>(o_oreads[q]), kept, hipMemcpyDeviceToHost, st));
            if (with_qual)
                PH_HIP(hipMemcpyAsync(hb[q].out_qual, w.at<uint8_t>(o_oqual[q]), kept, hipMemcpyDeviceToHost, st));
        }
    }
    PH_HIP(hipStreamSynchronize(st));
    t_info = polyhip_demux_info{entries,           info[I_ASSIGNED],       info[I_EXACT], info[I_NO_BARCODE],
                                info[I_AMBIGUOUS], info[I_NOT_IN_SHEET], info[I_BAD],   bytes_in,
                                bytes_out};
    return POLYHIP_OK;
}

} // namespace
} // namespace polyhip

using namespace polyhip;

extern "C" {

int polyhip_demux_reads(const polyhip_demux_params *params, const uint8_t *barcodes, const uint32_t *barcode_off, uint32_t nbarcodes,
                        const uint8_t *reads, const uint64_t *off, const uint8_t *qual, const uint64_t *qual_off, uint64_t nreads,
                        uint32_t *barcode, uint32_t *bstart, uint32_t *mism, uint32_t *flags, uint32_t *err, uint32_t *sample,
                        uint32_t *order, uint64_t *sample_start, uint8_t *out_reads, uint8_t *out_qual, uint64_t *out_off)
{
    const HostSet sets[2] = {{barcodes, barcode_off, nbarcodes}, {nullptr, nullptr, 0}};
    HostBatch hb[1] = {{reads, off, qual, qual_off, out_reads, out_qual, out_off}};
    return demux_batches("polyhip_demux_reads", params, sets, nullptr, hb, 1, nreads, barcode, bstart, mism, flags, err, sample, order,
                         sample_start);
}

int polyhip_demux_pairs(const polyhip_demux_params *params, const uint8_t *barcodes1, const uint32_t *barcode_off1, uint32_t nbarcodes1,
                        const uint8_t *barcodes2, const uint32_t *barcode_off2, uint32_t nbarcodes2, const uint32_t *pair_sample,
                        const uint8_t *reads1, const uint64_t *off1, const uint8_t *qual1, const uint64_t *qual_off1,
                        const uint8_t *reads2, const uint64_t *off2, const uint8_t *qual2, const uint64_t *qual_off2, uint64_t npairs,
                        uint32_t *barcode, uint32_t *bstart, uint32_t *mism, uint32_t *flags, uint32_t *err, uint32_t *sample,
                        uint32_t *order, uint64_t *sample_start, uint8_t *out_reads1, uint8_t *out_qual1, uint64_t *out_off1,
                        uint8_t *out_reads2, uint8_t *out_qual2, uint64_t *out_off2)
{
    const HostSet sets[2] = {{barcodes1, barcode_off1, nbarcodes1}, {barcodes2, barcode_off2, nbarcodes2}};
    HostBatch hb[2] = {{reads1, off1, qual1, qual_off1, out_reads1, out_qual1, out_off1},
                       {reads2, off2, qual2, qual_off2, out_reads2, out_qual2, out_off2}};
    return demux_batches("polyhip_demux_pairs", params, sets, pair_sample, hb, 2, npairs, barcode, bstart, mism, flags, err, sample, order,
                         sample_start);
}

int polyhip_demux_last_info(polyhip_demux_info *info)
{
    PH_REQUIRE(info, "polyhip_demux_last_info: null argument");
    *info = t_info;
    return POLYHIP_OK;
}

} // extern "C"
