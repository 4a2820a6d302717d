// trim.hip -- polyhip_trim_reads and polyhip_trim_pairs: quality ends, 3' adapters and the overlap of two mates cut off a packed
// batch of reads before it is mapped.  The definition is the comment above the calls in include/polyhip.h; tests/trim_oracle.py
// restates it in plain Python.  All of it is integer work and no atomic decides an output byte.
//
//   decide_kernel   one wave per read (grid-stride), steps 1-3 of the definition:
//                   judge: the quality string in 64-column steps, length and range;
//                   quality_walk, once from each end: per step an inclusive wave scan of (cut-off - Q) on top of a carry, a
//                   ballot for the first negative sum, and the wave's greatest sum with the first lane that holds it;
//                   adapters: a lane per start s, 64 starts a step.  The 128 read bytes a step can touch are taken once, as
//                   eight ballots: for each of A, C, G, T the 128 positions that hold it (either case), of which a lane
//                   keeps the 64 from its own start on.  An adapter is four such masks made by the host, so its
//                   mismatches at all 64 starts are four ANDs and a population count; the step runs down the adapters and
//                   the search ends at the first step that holds a hit: the smallest s wins
//   pair_kernel     one wave per pair, a lane per candidate insert I from min(m1, m2) down, 64 a step, with the same masks: 64
//                   bytes of mate 1 against 128 of mate 2's reverse complement at a time; ends at the first step that holds a
//                   qualifying I: the greatest wins
//   finish_kernel   a lane per entry: step 4 (min_len), the kept length for the scan, the info counters
//   scan_excl       (device_prims.h) the kept lengths -> out_off, per mate
//   gather_kernel   one wave per read: r[a, b) and the same slice of its quality string to their places
#include "host_pipeline.h"
#include "read_batch.h"

namespace polyhip {
namespace {

constexpr int TR_WAVES = BT / 64; // reads a block works on at a time
constexpr uint32_t MAX_ADAPTERS = 255, MAX_ADAPTER = 64;
constexpr uint32_t MAX_READ = 1u << 24; // the running sums of the quality walks are int32: 93 * 2^24 < 2^31
enum : uint32_t { F_QUAL_3P = 1u, F_QUAL_5P = 2u, F_ADAPTER = 4u, F_SHORT = 8u, F_OVERLAP = 16u };
enum : int { I_CUT_3P = 0, I_CUT_5P = 1, I_ADAPTER = 2, I_OVERLAP = 3, I_SHORT = 4, I_BAD = 5, N_INFO = 6 };

struct Knobs {
    uint32_t qual_offset, min_qual_5p, min_qual_3p, adapter_err_pct, min_overlap, nadapters;
};

// the complement's letter, 0xFF for every other byte: never equal to a base_code
__device__ __forceinline__ uint32_t complement_code(uint32_t c)
{
    const uint32_t u = c & ~0x20u;
    return u == 'A' ? 'T' : u == 'T' ? 'A' : u == 'C' ? 'G' : u == 'G' ? 'C' : 0xFFu;
}

// The walk of step 2 from one end of q[0, m): position j of the walk is byte j (from_end: byte m - 1 - j).  Returns how many
// bytes the end loses: one more than the j at which the running sum first reached its greatest value, 0 if that is not > 0.
// Every lane of the wave calls it with the same arguments.
__device__ __forceinline__ uint32_t quality_walk(const uint8_t *q, uint32_t m, uint32_t qual_offset, uint32_t cutoff, bool from_end,
                                                 int lane)
{
    int carry = 0, best = 0;
    uint32_t ncut = 0;
    for (uint32_t base = 0; base < m; base += 64) {
        const uint32_t j = base + lane;
        const bool v = j < m;
        const int d = v ? (int)cutoff - (int)((uint32_t)q[from_end ? m - 1 - j : j] - qual_offset) : 0;
        const int s = carry + (int)dpp_incl_scan((uint32_t)d);
        const uint64_t stop = __ballot(!v || s < 0);                                   // the walk ends before the first of these
        const uint64_t live = stop ? lanes_below(__ffsll((long long)stop) - 1) : ~0ull; // s >= 0 in all of them
        const bool in = live >> lane & 1ull;
        const uint32_t key = in ? (uint32_t)s ^ 0x80000000u : 0u;
        const uint32_t top = dpp_wave_max(key);
        const uint64_t holders = __ballot(in && key == top);
        if (holders && (int)(top ^ 0x80000000u) > best) { // strictly: among equal sums the first j stays
            best = (int)(top ^ 0x80000000u);
            ncut = base + (uint32_t)__ffsll((long long)holders);
        }
        if (stop)
            break;
        carry = __builtin_amdgcn_readlane(s, 63);
    }
    return ncut;
}

// Steps 1-3 for read i of the batch; entry e = i * stride + phase of start / end / flags / err (pairs: stride 2, phase = mate)
// adapter t: ad_len[t] bytes; bit k of ad_mask[4 * t + c] says that its byte k is "ACGT"[c]
__global__ __launch_bounds__(BT) void decide_kernel(uint64_t n, Knobs kn, DevBatch in, const uint64_t *__restrict__ ad_mask,
                                                    const uint32_t *__restrict__ ad_len, uint32_t stride, uint32_t phase,
                                                    uint32_t *__restrict__ start, uint32_t *__restrict__ end,
                                                    uint32_t *__restrict__ flags, uint32_t *__restrict__ err)
{
    const int lane = threadIdx.x & 63;
    const uint64_t off0 = in.off[0], qoff0 = in.qual ? in.qual_off[0] : 0;
    for (uint64_t i = (uint64_t)blockIdx.x * TR_WAVES + (threadIdx.x >> 6); i < n; i += (uint64_t)gridDim.x * TR_WAVES) {
        const uint32_t m = (uint32_t)(in.off[i + 1] - in.off[i]);
        const uint8_t *r = in.reads + (in.off[i] - off0);
        const uint8_t *q = nullptr;
        uint32_t e = 0, a = 0, b = m, f = 0;
        // 1. judging: the whole quality string before anything else looks at the read
        if (in.qual) {
            const uint64_t qm = in.qual_off[i + 1] - in.qual_off[i];
            q = in.qual + (in.qual_off[i] - qoff0);
            if (qm != (uint64_t)m) {
                e = 1;
            } else {
                bool bad = false;
                for (uint32_t base = 0; base < m; base += 64) {
                    const uint32_t c = base + lane;
                    const uint32_t x = c < m ? q[c] : kn.qual_offset;
                    bad |= x < kn.qual_offset || x > kn.qual_offset + 93u;
                }
                if (__ballot(bad))
                    e = 2;
            }
        }
        if (e == 0) {
            // 2. quality ends, both on the read as it came
            if (kn.min_qual_3p)
                b = m - quality_walk(q, m, kn.qual_offset, kn.min_qual_3p, true, lane);
            if (kn.min_qual_5p)
                a = quality_walk(q, m, kn.qual_offset, kn.min_qual_5p, false, lane);
            if (a >= b)
                a = b = 0;
            f = (b < m ? F_QUAL_3P : 0u) | (a > 0 ? F_QUAL_5P : 0u);
            // 3. 3' adapters on r[a, b): 64 starts a step, the step's 128 bytes as four masks of 128 positions
            if (kn.nadapters) {
                for (uint32_t base = a; base < b; base += 64) {
                    const uint32_t c0 = base + lane, c1 = c0 + 64;
                    const uint32_t x0 = c0 < b ? base_code(r[c0]) : 0u, x1 = c1 < b ? base_code(r[c1]) : 0u;
                    uint64_t W[4]; // bit k: byte s + k of the read is "ACGT"[c], for this lane's start s
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const uint32_t letter = "ACGT"[c];
                        const uint64_t lo = __ballot(x0 == letter), hi = __ballot(x1 == letter);
                        W[c] = lane ? lo >> lane | hi << (64 - lane) : lo;
                    }
                    const uint32_t s = base + lane, room = s < b ? b - s : 0u;
                    uint32_t hit_lane = 64, hit_t = 0;
                    for (uint32_t t = 0; t < kn.nadapters; ++t) {
                        const uint32_t p = ad_len[t];
                        const uint32_t L = p < room ? p : room;
                        const uint64_t same = (W[0] & ad_mask[4 * t]) | (W[1] & ad_mask[4 * t + 1]) | (W[2] & ad_mask[4 * t + 2]) |
                                              (W[3] & ad_mask[4 * t + 3]);
                        const uint64_t first_L = L >= 64 ? ~0ull : (1ull << L) - 1ull;
                        const uint32_t mism = L - (uint32_t)__popcll(same & first_L);
                        const uint64_t hits = __ballot(L >= kn.min_overlap && 100u * mism <= kn.adapter_err_pct * L);
                        const uint32_t first = hits ? (uint32_t)__ffsll((long long)hits) - 1u : 64u;
                        if (first < hit_lane) { // a tie goes to the lowest adapter index
                            hit_lane = first;
                            hit_t = t;
                        }
                    }
                    if (hit_lane < 64) {
                        b = base + hit_lane;
                        f |= F_ADAPTER | hit_t << 8;
                        break;
                    }
                }
            }
        }
        if (lane == 0) {
            const uint64_t at = i * stride + phase;
            start[at] = e ? 0u : a;
            end[at] = e ? 0u : b;
            flags[at] = e ? 0u : f;
            err[at] = e;
        }
    }
}

// Step P for pair i, entries 2i and 2i + 1, on the mates as they came
__global__ __launch_bounds__(BT) void pair_kernel(uint64_t npairs, uint32_t pair_min_overlap, uint32_t pair_err_pct, DevBatch in1,
                                                  DevBatch in2, uint32_t *__restrict__ start, uint32_t *__restrict__ end,
                                                  uint32_t *__restrict__ flags, const uint32_t *__restrict__ err)
{
    const int lane = threadIdx.x & 63;
    const uint64_t off1 = in1.off[0], off2 = in2.off[0];
    for (uint64_t i = (uint64_t)blockIdx.x * TR_WAVES + (threadIdx.x >> 6); i < npairs; i += (uint64_t)gridDim.x * TR_WAVES) {
        if (err[2 * i] | err[2 * i + 1] | ((flags[2 * i] | flags[2 * i + 1]) & F_ADAPTER))
            continue;
        const uint32_t m1 = (uint32_t)(in1.off[i + 1] - in1.off[i]), m2 = (uint32_t)(in2.off[i + 1] - in2.off[i]);
        const uint32_t top = m1 < m2 ? m1 : m2;
        const uint8_t *r1 = in1.reads + (in1.off[i] - off1), *r2 = in2.reads + (in2.off[i] - off2);
        uint32_t found = 0;
        for (uint32_t base = 0; base + pair_min_overlap <= top; base += 64) {
            const bool v = base + lane + pair_min_overlap <= top;
            const uint32_t I = v ? top - base - lane : 0u, widest = top - base; // lane 0's, the step's greatest
            // Insert I says that r1[0, I) is the last I bytes of the reverse complement V of mate 2, V[x] = comp(r2[m2 - 1 - x]):
            // r1[k] meets V[k + m2 - I], and m2 - I = d0 + lane.  So, 64 bytes of r1 at a time, the masks of decide_kernel's
            // adapter search: r1's chunk is the "adapter", the 128 bytes of V from d0 + kk on are the "read"
            const uint32_t d0 = m2 - widest;
            uint32_t match = 0;
            for (uint32_t kk = 0; kk < widest; kk += 64) {
                const uint32_t k1 = kk + lane, v0 = d0 + kk + lane, v1 = v0 + 64;
                const uint32_t x = k1 < widest ? base_code(r1[k1]) : 0u;
                const uint32_t y0 = v0 < m2 ? complement_code(r2[m2 - 1 - v0]) : 0xFFu;
                const uint32_t y1 = v1 < m2 ? complement_code(r2[m2 - 1 - v1]) : 0xFFu;
                uint64_t same = 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint32_t letter = "ACGT"[c];
                    const uint64_t mine = __ballot(x == letter), lo = __ballot(y0 == letter), hi = __ballot(y1 == letter);
                    same |= (lane ? lo >> lane | hi << (64 - lane) : lo) & mine;
                }
                const uint32_t left = I > kk ? I - kk : 0u; // of this chunk, the bytes that belong to insert I
                match += (uint32_t)__popcll(same & (left >= 64 ? ~0ull : (1ull << left) - 1ull));
            }
            const uint32_t mism = I - match;
            const uint64_t hits = __ballot(v && 100u * mism <= pair_err_pct * I);
            if (hits) {
                found = top - base - ((uint32_t)__ffsll((long long)hits) - 1u);
                break;
            }
        }
        if (found && lane < 2) {
            const uint64_t at = 2 * i + lane;
            const uint32_t a = start[at], b = end[at];
            if (found < b) {
                const bool gone = a >= found;
                start[at] = gone ? 0u : a;
                end[at] = gone ? 0u : found;
                flags[at] |= F_OVERLAP;
            }
        }
    }
}

// Step 4, the kept length of every entry where the scan wants it (pairs: mate 1's n + 1 slots, then mate 2's), the counters
__global__ __launch_bounds__(BT) void finish_kernel(uint64_t entries, uint32_t stride, uint64_t n, uint32_t min_len,
                                                    const uint32_t *__restrict__ start, const uint32_t *__restrict__ end,
                                                    uint32_t *__restrict__ flags, const uint32_t *__restrict__ err,
                                                    uint64_t *__restrict__ kept, unsigned long long *info)
{
    __shared__ uint32_t s_info[N_INFO];
    if (threadIdx.x < N_INFO)
        s_info[threadIdx.x] = 0;
    __syncthreads();
    uint32_t c3 = 0, c5 = 0, cad = 0, cov = 0, csh = 0, cbad = 0;
    const uint64_t rounds = (entries + (uint64_t)gridDim.x * BT - 1) / ((uint64_t)gridDim.x * BT); // whole waves stay together
    for (uint64_t k = 0; k < rounds; ++k) {
        const uint64_t e = (k * gridDim.x + blockIdx.x) * BT + threadIdx.x;
        if (e < entries) {
            uint32_t f = flags[e];
            const uint32_t len = end[e] - start[e], bad = err[e] != 0;
            if (!bad && len < min_len) {
                f |= F_SHORT;
                flags[e] = f;
            }
            kept[stride == 2 ? (e & 1) * (n + 1) + (e >> 1) : e] = bad || (f & F_SHORT) ? 0ull : (uint64_t)len;
            c3 += f & F_QUAL_3P ? 1u : 0u;
            c5 += f & F_QUAL_5P ? 1u : 0u;
            cad += f & F_ADAPTER ? 1u : 0u;
            cov += f & F_OVERLAP ? 1u : 0u;
            csh += f & F_SHORT ? 1u : 0u;
            cbad += bad;
        }
    }
    add_info(s_info, I_CUT_3P, c3);
    add_info(s_info, I_CUT_5P, c5);
    add_info(s_info, I_ADAPTER, cad);
    add_info(s_info, I_OVERLAP, cov);
    add_info(s_info, I_SHORT, csh);
    add_info(s_info, I_BAD, cbad);
    __syncthreads(); // one atomic per block and counter that has something
    if (threadIdx.x < N_INFO && s_info[threadIdx.x])
        atomicAdd(&info[threadIdx.x], (unsigned long long)s_info[threadIdx.x]);
}

// read i's kept bytes, and those of its quality string, to out_off[i]
__global__ __launch_bounds__(BT) void gather_kernel(uint64_t n, DevBatch in, uint32_t stride, uint32_t phase,
                                                    const uint32_t *__restrict__ start, const uint64_t *__restrict__ out_off,
                                                    uint8_t *__restrict__ out_reads, uint8_t *__restrict__ out_qual)
{
    const int lane = threadIdx.x & 63;
    const uint64_t off0 = in.off[0], qoff0 = in.qual ? in.qual_off[0] : 0;
    for (uint64_t i = (uint64_t)blockIdx.x * TR_WAVES + (threadIdx.x >> 6); i < n; i += (uint64_t)gridDim.x * TR_WAVES) {
        const uint64_t dst = out_off[i], len = out_off[i + 1] - dst;
        if (len == 0)
            continue;
        const uint32_t a = start[i * stride + phase];
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

thread_local polyhip_trim_info t_info{};

// both calls: nb = 1 (entry i is read i) or 2 (entries 2i, 2i + 1 are the mates of pair i)
int trim_batches(const char *who, const polyhip_trim_params *params, const uint8_t *adapters, const uint32_t *adapter_off,
                 uint32_t nadapters, HostBatch *hb, int nb, uint64_t n, uint32_t *start, uint32_t *end, uint32_t *flags,
                 uint32_t *err)
{
    PH_REQUIRE(params, "%s: null params", who);
    const polyhip_trim_params &p = *params;
    PH_REQUIRE(p.qual_offset <= 162, "%s: qual_offset = %u, qual_offset + 93 must fit a byte", who, p.qual_offset);
    PH_REQUIRE(p.min_qual_5p <= 93, "%s: min_qual_5p = %u, a quality is 0..93", who, p.min_qual_5p);
    PH_REQUIRE(p.min_qual_3p <= 93, "%s: min_qual_3p = %u, a quality is 0..93", who, p.min_qual_3p);
    PH_REQUIRE(p.adapter_err_pct <= 100, "%s: adapter_err_pct = %u, it is 0..100", who, p.adapter_err_pct);
    PH_REQUIRE(p.min_overlap >= 1, "%s: min_overlap = 0, a hit has at least one byte", who);
    PH_REQUIRE(p.pair_err_pct <= 100, "%s: pair_err_pct = %u, it is 0..100", who, p.pair_err_pct);
    PH_REQUIRE(nadapters <= MAX_ADAPTERS, "%s: %u adapters, at most %u", who, nadapters, MAX_ADAPTERS);
    PH_REQUIRE(nadapters == 0 || (adapters && adapter_off), "%s: null adapters", who);
    for (uint32_t t = 0; t < nadapters; ++t) {
        PH_REQUIRE(adapter_off[t + 1] > adapter_off[t], "%s: adapter %u is empty", who, t);
        const uint32_t len = adapter_off[t + 1] - adapter_off[t];
        PH_REQUIRE(len <= MAX_ADAPTER, "%s: adapter %u has %u bytes, at most %u", who, t, len, MAX_ADAPTER);
        for (uint32_t k = 0; k < len; ++k) {
            const uint8_t c = adapters[adapter_off[t] + k];
            PH_REQUIRE(c == 'A' || c == 'C' || c == 'G' || c == 'T', "%s: adapter %u has byte 0x%02x at %u, adapters are upper-case ACGT",
                       who, t, c, k);
        }
    }
    const bool with_qual = hb[0].qual != nullptr;
    for (int q = 0; q < nb; ++q)
        PH_REQUIRE(!(p.min_qual_5p || p.min_qual_3p) || hb[q].qual, "%s: a quality cut-off without qualities (qual is NULL)", who);
    for (int q = 0; q < nb; ++q)
        PH_REQUIRE((hb[q].qual != nullptr) == (hb[q].qual_off != nullptr), "%s: qual and qual_off come together or not at all", who);
    PH_REQUIRE(nb == 1 || (hb[1].qual != nullptr) == with_qual, "%s: qualities of one mate only", who);
    for (int q = 0; q < nb; ++q)
        PH_REQUIRE((hb[q].out_qual != nullptr) == (hb[q].qual != nullptr), "%s: out_qual is given exactly when qual is", who);
    PH_REQUIRE(start && end && flags && err, "%s: null argument", who);
    for (int q = 0; q < nb; ++q)
        PH_REQUIRE(hb[q].out_reads && hb[q].out_off && (n == 0 || (hb[q].reads && hb[q].off)), "%s: null argument", who);
    for (int q = 0; q < nb; ++q)
        for (uint64_t i = 0; i < n; ++i)
            PH_REQUIRE(hb[q].off[i + 1] >= hb[q].off[i] && (!with_qual || hb[q].qual_off[i + 1] >= hb[q].qual_off[i]),
                       "%s: offsets are not ascending", who);
    for (int q = 0; q < nb; ++q)
        for (uint64_t i = 0; i < n; ++i)
            if (hb[q].off[i + 1] - hb[q].off[i] >= MAX_READ)
                return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: read %llu has %llu bytes, the running sums are 32-bit and hold fewer than 2^24",
                                 who, (unsigned long long)i, (unsigned long long)(hb[q].off[i + 1] - hb[q].off[i]));
    t_info = polyhip_trim_info{};
    if (n == 0) {
        for (int q = 0; q < nb; ++q)
            hb[q].out_off[0] = 0;
        return POLYHIP_OK;
    }

    HostStreams &hs = host_streams();
    PH_HIP(hs.init());
    hipStream_t st = hs.s[0];
    const uint64_t entries = n * (uint64_t)nb;
    uint64_t rbytes[2] = {0, 0}, qbytes[2] = {0, 0};
    size_t o_reads[2], o_off[2], o_qual[2], o_qoff[2], o_oreads[2], o_oqual[2];
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
    }
    const size_t o_kept = w.reserve((n + 1) * 8 * nb), o_start = w.reserve(entries * 4), o_end = w.reserve(entries * 4),
                 o_flags = w.reserve(entries * 4), o_err = w.reserve(entries * 4), o_ad = w.reserve(nadapters * 32),
                 o_adlen = w.reserve(nadapters * 4), o_scan = w.reserve(scan_scratch_bytes<uint64_t>(n)),
                 o_info = w.reserve(N_INFO * 8);
    PH_HIP(w.buf.alloc(w.used));
    SyncOnExit sync(st);
    std::vector<uint64_t> ad_mask(4 * (size_t)nadapters, 0); // per adapter and letter of ACGT: the positions that hold it
    std::vector<uint32_t> ad_len(nadapters, 0);
    for (uint32_t t = 0; t < nadapters; ++t) {
        ad_len[t] = adapter_off[t + 1] - adapter_off[t];
        for (uint32_t k = 0; k < ad_len[t]; ++k) {
            const uint8_t c = adapters[adapter_off[t] + k];
            ad_mask[4 * t + (c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3)] |= 1ull << k;
        }
    }
    if (nadapters) {
        PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_ad), ad_mask.data(), nadapters * 32, hipMemcpyHostToDevice, st));
        PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_adlen), ad_len.data(), nadapters * 4, hipMemcpyHostToDevice, st));
    }
    PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_info), 0, N_INFO * 8, st));
    DevBatch db[2];
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
    uint32_t *d_start = w.at<uint32_t>(o_start), *d_end = w.at<uint32_t>(o_end), *d_flags = w.at<uint32_t>(o_flags),
             *d_err = w.at<uint32_t>(o_err);
    unsigned long long *d_info = w.at<unsigned long long>(o_info);
    uint64_t *d_kept = w.at<uint64_t>(o_kept);

    const Knobs kn{p.qual_offset, p.min_qual_5p, p.min_qual_3p, p.adapter_err_pct, p.min_overlap, nadapters};
    const unsigned wgrid = grid_for(n, TR_WAVES, 256 * 32);
    for (int q = 0; q < nb; ++q) {
        hipLaunchKernelGGL(decide_kernel, dim3(wgrid), dim3(BT), 0, st, n, kn, db[q], w.at<uint64_t>(o_ad), w.at<uint32_t>(o_adlen),
                           (uint32_t)nb, (uint32_t)q, d_start, d_end, d_flags, d_err);
        PH_HIP(hipGetLastError());
    }
    if (nb == 2 && p.pair_min_overlap) {
        hipLaunchKernelGGL(pair_kernel, dim3(wgrid), dim3(BT), 0, st, n, p.pair_min_overlap, p.pair_err_pct, db[0], db[1], d_start, d_end,
                           d_flags, d_err);
        PH_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(finish_kernel, dim3(grid_for(entries, BT, 512)), dim3(BT), 0, st, entries, (uint32_t)nb, n, p.min_len, d_start,
                       d_end, d_flags, d_err, d_kept, d_info);
    PH_HIP(hipGetLastError());
    for (int q = 0; q < nb; ++q) {
        uint64_t *d_ooff = d_kept + (uint64_t)q * (n + 1); // scanned in place
        PH_HIP(scan_excl<uint64_t>(d_ooff, d_ooff, n, w.at<uint8_t>(o_scan), st));
        hipLaunchKernelGGL(gather_kernel, dim3(wgrid), dim3(BT), 0, st, n, db[q], (uint32_t)nb, (uint32_t)q, d_start, d_ooff,
                           w.at<uint8_t>(o_oreads[q]), with_qual ? w.at<uint8_t>(o_oqual[q]) : (uint8_t *)nullptr);
        PH_HIP(hipGetLastError());
        PH_HIP(hipMemcpyAsync(hb[q].out_off, d_ooff, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    }
    unsigned long long info[N_INFO];
    PH_HIP(hipMemcpyAsync(start, d_start, entries * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(end, d_end, entries * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(flags, d_flags, entries * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(err, d_err, entries * 4, hipMemcpyDeviceToHost, st));
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
    t_info = polyhip_trim_info{entries,         bytes_in,        bytes_out,     info[I_CUT_3P], info[I_CUT_5P],
                               info[I_ADAPTER], info[I_OVERLAP], info[I_SHORT], info[I_BAD]};
    return POLYHIP_OK;
}

} // namespace
} // namespace polyhip

using namespace polyhip;

extern "C" {

int polyhip_trim_reads(const polyhip_trim_params *params, const uint8_t *adapters, const uint32_t *adapter_off, uint32_t nadapters,
                       const uint8_t *reads, const uint64_t *off, const uint8_t *qual, const uint64_t *qual_off, uint64_t nreads,
                       uint32_t *start, uint32_t *end, uint32_t *flags, uint32_t *err, uint8_t *out_reads, uint8_t *out_qual,
                       uint64_t *out_off)
{
    HostBatch hb[1] = {{reads, off, qual, qual_off, out_reads, out_qual, out_off}};
    return trim_batches("polyhip_trim_reads", params, adapters, adapter_off, nadapters, hb, 1, nreads, start, end, flags, err);
}

int polyhip_trim_pairs(const polyhip_trim_params *params, const uint8_t *adapters, const uint32_t *adapter_off, uint32_t nadapters,
                       const uint8_t *reads1, const uint64_t *off1, const uint8_t *qual1, const uint64_t *qual_off1,
                       const uint8_t *reads2, const uint64_t *off2, const uint8_t *qual2, const uint64_t *qual_off2, uint64_t npairs,
                       uint32_t *start, uint32_t *end, uint32_t *flags, uint32_t *err, uint8_t *out_reads1, uint8_t *out_qual1,
                       uint64_t *out_off1, uint8_t *out_reads2, uint8_t *out_qual2, uint64_t *out_off2)
{
    HostBatch hb[2] = {{reads1, off1, qual1, qual_off1, out_reads1, out_qual1, out_off1},
                       {reads2, off2, qual2, qual_off2, out_reads2, out_qual2, out_off2}};
    return trim_batches("polyhip_trim_pairs", params, adapters, adapter_off, nadapters, hb, 2, npairs, start, end, flags, err);
}

int polyhip_trim_last_info(polyhip_trim_info *info)
{
    PH_REQUIRE(info, "polyhip_trim_last_info: null argument");
    *info = t_info;
    return POLYHIP_OK;
}

} // extern "C"
