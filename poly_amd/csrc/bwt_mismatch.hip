// bwt_mismatch.hip -- search/bwt with up to k substitutions (k <= 4) on gfx950: Count and Locate of every position of
// the sequence whose Hamming distance to the pattern is at most k (no counterpart in the reference).
//
//   hits(P, k) = { (p, d) : 0 <= p <= n - m,  d = #{ j : S[p + j] != P[j] } <= k }
//
// Search: a backward search with backtracking over the Index of bwt.hip.  A node is (symbols left i, rows [s, e),
// mismatches d); its children extend by the pattern's own byte at cost 0 and, while d < k, by every other symbol of the
// sequence's alphabet at cost 1.  '$' is never a child, so a row of a live node never runs through the end of T: matches
// are inside the sequence and a pattern longer than it dies on its own.  A node with i == 0 is a leaf: e - s positions at
// distance d.  Different paths spell different strings, so no position is reached twice.
//
// Mapping: one pattern per lane, one node expansion per lane and loop trip, so the occurrence reads of a wave are issued
// together; a lane that finishes its pattern takes the next one of its grid stride in the same trip.
// Stack: k + 1 frames per lane in LDS (word-major, so a wave's accesses to one word are conflict free), never m: frame
// d holds the node that walks the cost-0 path at distance d, and the cost-1 children it branched off one level below:
//   nucleotide layout: one occ_nuc4 per range end gives all four children; the match child replaces the node in its
//     frame, the other three wait in frame d + 1 as intervals;
//   general layout: sigma can be 255, so frame d + 1 keeps the parent's interval and a symbol cursor, and every trip
//     computes one child (two occ_gen).
// Locate: the count pass gives the per-pattern totals and their scan `first`; a second search writes (pattern << B | SA[r],
// d) for every row of every leaf into the pattern's segment (a leaf of WIDE rows or more is written by the whole wave),
// and the LSD radix sort of device_prims.h orders them by (pattern, position) over the significant bits.
#include "bwt_index.h"
#include "device_prims.h"

namespace polyhip {
namespace {

constexpr int MT = 128;        // threads per block of the search kernel (its LDS stack: 35 KB at k = 4)
// rows from which a leaf is written by the wave instead of its lane.  Not tuned: a narrower leaf is written serially by
// its lane while the other lanes of the wave wait, a wide one costs the wave one loop trip each; neither cost nor the
// value 16 has been measured against another.
constexpr uint32_t WIDE = 16;

// frame words.  The node: CI symbols left, rows [CS, CE) (live iff CS < CE).  The waiting cost-1 children: PI their
// symbols left, CUR the next code to try; nucleotide: PS/PE[4] their intervals (the match code's is empty); general: SKIP
// the match code, [PS, PE) the parent's rows.
enum { CI = 0, CS = 1, CE = 2, PI = 3, CUR = 4, PS = 5, PE = 9, SKIP = 5, GPS = 6, GPE = 7 };
template <int LAYOUT> constexpr int frame_words() { return LAYOUT == 0 ? 13 : 8; }
template <int LAYOUT> size_t stack_bytes(uint32_t k) { return (size_t)(k + 1) * (frame_words<LAYOUT>() + 1) * MT * sizeof(uint32_t); }

enum { ACT_DONE = 0, ACT_EXPAND = 1, ACT_TRY = 2, ACT_LEAF = 3 };

__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v += __shfl_down(v, d, 64);
    return v;
}

// EMIT == false: counts[p * (k + 1) + d] and err[p] for every pattern, info[0..3] += nodes visited (expanded ones and
//   leaves), distinct occurrence lines / blocks read by the expansions, leaves, positions.
// EMIT == true: keys / vals [first[p] .. first[p + 1]) = (p << pos_bits | SA[r], d) of every leaf row, in search order.
template <int LAYOUT, bool EMIT>
__global__ __launch_bounds__(MT) void mismatch_kernel(Index x, const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off,
                                                      uint64_t npat, uint32_t k, uint32_t *__restrict__ counts,
                                                      uint32_t *__restrict__ err, const uint64_t *__restrict__ first,
                                                      const uint32_t *__restrict__ sa, uint64_t *__restrict__ keys,
                                                      uint32_t *__restrict__ vals, int pos_bits, unsigned long long *__restrict__ info)
{
    extern __shared__ uint32_t lds[];
    __shared__ uint8_t code[256];
    __shared__ uint8_t byte_of[256];
    __shared__ uint32_t Cs[256];
    for (int t = threadIdx.x; t < 256; t += MT) {
        code[t] = x.dense[t];
        Cs[t] = x.C[t];
        byte_of[t] = 0;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 256; t += MT)
        if (code[t] != 0xFFu)
            byte_of[code[t]] = (uint8_t)t;
    __syncthreads();

    constexpr int FW = frame_words<LAYOUT>();
#define FR(f, w) lds[((f) * FW + (w)) * MT + threadIdx.x]
#define CNT(d) lds[((k + 1) * FW + (d)) * MT + threadIdx.x]
    const uint32_t nsym = LAYOUT == 0 ? 4u : x.sigma;
    const uint32_t n = x.N - 1;
    const uint64_t stride = (uint64_t)gridDim.x * MT;
    const int lane = threadIdx.x & 63;
    uint64_t p = blockIdx.x * (uint64_t)MT + threadIdx.x;
    uint64_t a = 0, wr = 0;
    int f = -1; // the top frame; -1 between patterns
    uint64_t n_nodes = 0, n_lines = 0, n_leaves = 0, n_hits = 0;

    for (;;) {
        // ---- pick this trip's work: the next node to expand, child to compute or leaf to write (LDS only) ----
        int act = ACT_DONE;
        uint32_t ni = 0, ns = 0, ne = 0, sym = 0;
        for (;;) {
            if (f < 0) {
                if (p >= npat)
                    break;
                a = off[p];
                const uint64_t m = off[p + 1] - a;
                if (!EMIT)
                    err[p] = m ? 0u : 1u;
                if (m == 0 || m > n) { // nothing to search: no hits
                    if (!EMIT)
                        for (uint32_t d = 0; d <= k; ++d)
                            counts[p * (k + 1) + d] = 0;
                    p += stride;
                    continue;
                }
                f = 0;
                FR(0, CI) = (uint32_t)m;
                FR(0, CS) = 0;
                FR(0, CE) = x.N;
                FR(0, CUR) = nsym; // the root has no waiting children
                if (LAYOUT != 0)
                    FR(0, SKIP) = 0xFFu;
                if (EMIT)
                    wr = first[p];
                else
                    for (uint32_t d = 0; d <= k; ++d)
                        CNT(d) = 0;
            }
            const uint32_t cs = FR(f, CS), ce = FR(f, CE);
            if (cs < ce) {
                const uint32_t ci = FR(f, CI);
                if (ci == 0) { // a leaf
                    FR(f, CE) = 0;
                    ++n_nodes;
                    ++n_leaves;
                    n_hits += ce - cs;
                    if (EMIT) {
                        act = ACT_LEAF;
                        ns = cs;
                        ne = ce;
                        break;
                    }
                    CNT(f) += ce - cs;
                    continue;
                }
                act = ACT_EXPAND;
                ni = ci;
                ns = cs;
                ne = ce;
                break;
            }
            uint32_t cur = FR(f, CUR);
            if (LAYOUT == 0) {
                if (cur < 4u) {
                    FR(f, CUR) = cur + 1;
                    FR(f, CI) = FR(f, PI);
                    FR(f, CS) = FR(f, PS + cur);
                    FR(f, CE) = FR(f, PE + cur);
                    continue;
                }
            } else {
                if (cur == FR(f, SKIP))
                    ++cur;
                if (cur < nsym) {
                    FR(f, CUR) = cur + 1;
                    act = ACT_TRY;
                    sym = cur;
                    ni = FR(f, PI);
                    ns = FR(f, GPS);
                    ne = FR(f, GPE);
                    break;
                }
            }
            if (--f < 0) { // the pattern is through
                if (!EMIT)
                    for (uint32_t d = 0; d <= k; ++d)
                        counts[p * (k + 1) + d] = CNT(d);
                p += stride;
            }
        }
        if (__ballot(act != ACT_DONE) == 0)
            break;

        // ---- leaves (locate): (pattern, position) keys into the pattern's segment ----
        if (EMIT) {
            const bool leaf = act == ACT_LEAF;
            const uint32_t w = ne - ns;
            if (leaf && w < WIDE)
                for (uint32_t r = ns; r < ne; ++r, ++wr) {
                    keys[wr] = (p << pos_bits) | sa[r];
                    vals[wr] = (uint32_t)f;
                }
            uint64_t wide = __ballot(leaf && w >= WIDE);
            while (wide) { // the whole wave writes one lane's leaf
                const int src = __ffsll((unsigned long long)wide) - 1;
                wide &= wide - 1;
                const uint32_t bs = __shfl(ns, src, 64), be = __shfl(ne, src, 64), bd = (uint32_t)__shfl(f, src, 64);
                const uint64_t bw = __shfl(wr, src, 64), bp = __shfl(p, src, 64);
                for (uint64_t r = (uint64_t)bs + lane; r < be; r += 64) {
                    keys[bw + (r - bs)] = (bp << pos_bits) | sa[r];
                    vals[bw + (r - bs)] = bd;
                }
            }
            if (leaf && w >= WIDE)
                wr += w;
        }

        // ---- one expansion per lane: two occurrence reads, the wave's issued together ----
        if (LAYOUT == 0) {
            if (act == ACT_EXPAND) {
                const uint32_t c = code[pat[a + ni - 1]]; // 0xFF: '$' or a byte the sequence lacks -- no cost-0 child
                const uint4 os = occ_nuc4(x, ns), oe = occ_nuc4(x, ne);
                ++n_nodes;
                n_lines += ns / NUC_SYMS == ne / NUC_SYMS ? 1 : 2; // both ends in one line: the second read hits it
                const uint32_t s0 = Cs[0] + os.x, s1 = Cs[1] + os.y, s2 = Cs[2] + os.z, s3 = Cs[3] + os.w;
                const uint32_t e0 = Cs[0] + oe.x, e1 = Cs[1] + oe.y, e2 = Cs[2] + oe.z, e3 = Cs[3] + oe.w;
                const uint32_t ms = c == 0 ? s0 : c == 1 ? s1 : c == 2 ? s2 : s3;
                const uint32_t me = c == 0 ? e0 : c == 1 ? e1 : c == 2 ? e2 : e3;
                FR(f, CI) = ni - 1;
                FR(f, CS) = c < 4u ? ms : 0u;
                FR(f, CE) = c < 4u ? me : 0u;
                if ((uint32_t)f < k) {
                    const int g = f + 1;
                    FR(g, CS) = 0;
                    FR(g, CE) = 0;
                    FR(g, PI) = ni - 1;
                    FR(g, CUR) = 0;
                    FR(g, PS + 0) = s0;
                    FR(g, PS + 1) = s1;
                    FR(g, PS + 2) = s2;
                    FR(g, PS + 3) = s3;
                    FR(g, PE + 0) = c == 0 ? s0 : e0;
                    FR(g, PE + 1) = c == 1 ? s1 : e1;
                    FR(g, PE + 2) = c == 2 ? s2 : e2;
                    FR(g, PE + 3) = c == 3 ? s3 : e3;
                    f = g;
                }
            }
        } else {
            uint32_t c = sym;
            uint8_t b = 0;
            if (act == ACT_EXPAND) {
                b = pat[a + ni - 1];
                c = code[b];
                ++n_nodes;
            } else if (act == ACT_TRY) {
                b = byte_of[sym];
            }
            const bool read = act == ACT_TRY || (act == ACT_EXPAND && c != 0xFFu);
            uint32_t rs = 0, re = 0;
            if (read) {
                rs = Cs[c] + occ_gen(x, c, b, ns);
                re = Cs[c] + occ_gen(x, c, b, ne);
                n_lines += ns / GEN_ROWS == ne / GEN_ROWS ? 1 : 2;
            }
            if (act == ACT_EXPAND) {
                FR(f, CI) = ni - 1;
                FR(f, CS) = rs;
                FR(f, CE) = re;
                if ((uint32_t)f < k) {
                    const int g = f + 1;
                    FR(g, CS) = 0;
                    FR(g, CE) = 0;
                    FR(g, PI) = ni - 1;
                    FR(g, CUR) = 0;
                    FR(g, SKIP) = c;
                    FR(g, GPS) = ns;
                    FR(g, GPE) = ne;
                    f = g;
                }
            } else if (act == ACT_TRY) {
                FR(f, CI) = ni;
                FR(f, CS) = rs;
                FR(f, CE) = re;
            }
        }
    }
#undef FR
#undef CNT
    if (!EMIT) {
        n_nodes = wave_sum(n_nodes);
        n_lines = wave_sum(n_lines);
        n_leaves = wave_sum(n_leaves);
        n_hits = wave_sum(n_hits);
        if (lane == 0) {
            atomicAdd(&info[0], (unsigned long long)n_nodes);
            atomicAdd(&info[1], (unsigned long long)n_lines);
            atomicAdd(&info[2], (unsigned long long)n_leaves);
            atomicAdd(&info[3], (unsigned long long)n_hits);
        }
    }
}

__global__ __launch_bounds__(BT) void mismatch_totals_kernel(const uint32_t *__restrict__ counts, uint64_t npat, uint32_t k,
                                                             uint64_t *__restrict__ tot)
{
    for (uint64_t p = blockIdx.x * (uint64_t)BT + threadIdx.x; p < npat; p += (uint64_t)gridDim.x * BT) {
        uint64_t s = 0;
        for (uint32_t d = 0; d <= k; ++d)
            s += counts[p * (k + 1) + d];
        tot[p] = s;
    }
}

__global__ __launch_bounds__(BT) void mismatch_unpack_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                             uint64_t total, int pos_bits, uint32_t *__restrict__ pos,
                                                             uint8_t *__restrict__ mm)
{
    const uint64_t mask = (1ull << pos_bits) - 1;
    for (uint64_t i = blockIdx.x * (uint64_t)BT + threadIdx.x; i < total; i += (uint64_t)gridDim.x * BT) {
        pos[i] = (uint32_t)(keys[i] & mask);
        mm[i] = (uint8_t)vals[i];
    }
}

thread_local polyhip_bwt_mismatch_info t_info{};

// the count pass: d_counts[npat * (k + 1)], d_err[npat]; d_info[4] must be zero on entry
int search_launch(const BwtHandle *h, const uint8_t *d_pat, const uint64_t *d_off, uint64_t npat, uint32_t k, uint32_t *d_counts,
                  uint32_t *d_err, unsigned long long *d_info, hipStream_t st)
{
    if (npat == 0)
        return POLYHIP_OK;
    if (h->x.layout == 0)
        hipLaunchKernelGGL((mismatch_kernel<0, false>), dim3(grid_for(npat, MT)), dim3(MT), stack_bytes<0>(k), st, h->x, d_pat, d_off,
                           npat, k, d_counts, d_err, (const uint64_t *)nullptr, (const uint32_t *)nullptr, (uint64_t *)nullptr,
                           (uint32_t *)nullptr, 0, d_info);
    else
        hipLaunchKernelGGL((mismatch_kernel<1, false>), dim3(grid_for(npat, MT)), dim3(MT), stack_bytes<1>(k), st, h->x, d_pat, d_off,
                           npat, k, d_counts, d_err, (const uint64_t *)nullptr, (const uint32_t *)nullptr, (uint64_t *)nullptr,
                           (uint32_t *)nullptr, 0, d_info);
    PH_HIP(hipGetLastError());
    return POLYHIP_OK;
}

// d_first[0..npat] = exclusive scan of the per-pattern totals of d_counts (scratch: scan_scratch_bytes<uint64_t>(npat))
int first_launch(const uint32_t *d_counts, uint64_t npat, uint32_t k, uint64_t *d_first, uint8_t *scratch, hipStream_t st)
{
    hipLaunchKernelGGL(mismatch_totals_kernel, dim3(grid_for(npat)), dim3(BT), 0, st, d_counts, npat, k, d_first);
    PH_HIP(hipGetLastError());
    PH_HIP(scan_excl<uint64_t>(d_first, d_first, npat, scratch, st));
    return POLYHIP_OK;
}

int pos_bits_of(const BwtHandle *h) { return bits_for(h->n); }

// the locate pass: the second search fills ka / va [0, total), the sort orders them, d_pos / d_mm receive the result.
// ka, kb: total uint64 each; va, vb: total uint32 each; hist: 256 * radix_blocks(total) + 1 uint32; scratch: the scan's.
int locate_launch(const BwtHandle *h, const uint8_t *d_pat, const uint64_t *d_off, uint64_t npat, uint32_t k, const uint64_t *d_first,
                  uint64_t total, uint64_t *ka, uint32_t *va, uint64_t *kb, uint32_t *vb, uint32_t *hist, uint8_t *scratch,
                  uint32_t *d_pos, uint8_t *d_mm, hipStream_t st)
{
    const int B = pos_bits_of(h);
    if (h->x.layout == 0)
        hipLaunchKernelGGL((mismatch_kernel<0, true>), dim3(grid_for(npat, MT)), dim3(MT), stack_bytes<0>(k), st, h->x, d_pat, d_off,
                           npat, k, (uint32_t *)nullptr, (uint32_t *)nullptr, d_first, (const uint32_t *)h->d_sa, ka, va, B,
                           (unsigned long long *)nullptr);
    else
        hipLaunchKernelGGL((mismatch_kernel<1, true>), dim3(grid_for(npat, MT)), dim3(MT), stack_bytes<1>(k), st, h->x, d_pat, d_off,
                           npat, k, (uint32_t *)nullptr, (uint32_t *)nullptr, d_first, (const uint32_t *)h->d_sa, ka, va, B,
                           (unsigned long long *)nullptr);
    PH_HIP(hipGetLastError());
    if (int r = radix_sort(ka, va, kb, vb, total, B + bits_for(npat - 1), hist, scratch, st))
        return r;
    hipLaunchKernelGGL(mismatch_unpack_kernel, dim3(grid_for(total)), dim3(BT), 0, st, ka, va, total, B, d_pos, d_mm);
    PH_HIP(hipGetLastError());
    return POLYHIP_OK;
}

bool offsets_ok(const uint64_t *off, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i])
            return false;
    return true;
}

// what both entry points upload and run first: the patterns, the count pass and the info
struct CountPass {
    DevBuf dp, doff, dcounts, derr, dinfo;
    int run(const BwtHandle *h, const uint8_t *pat, const uint64_t *off, uint64_t npat, uint32_t k, hipStream_t st)
    {
        const uint64_t nbytes = off[npat];
        PH_HIP(dp.alloc(nbytes));
        PH_HIP(doff.alloc((npat + 1) * sizeof(uint64_t)));
        PH_HIP(dcounts.alloc(npat * (k + 1) * sizeof(uint32_t)));
        PH_HIP(derr.alloc(npat * sizeof(uint32_t)));
        PH_HIP(dinfo.alloc(4 * sizeof(unsigned long long)));
        if (nbytes)
            PH_HIP(hipMemcpyAsync(dp.p, pat, nbytes, hipMemcpyHostToDevice, st));
        PH_HIP(hipMemcpyAsync(doff.p, off, (npat + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        PH_HIP(hipMemsetAsync(dinfo.p, 0, 4 * sizeof(unsigned long long), st));
        return search_launch(h, dp.as<uint8_t>(), doff.as<uint64_t>(), npat, k, dcounts.as<uint32_t>(), derr.as<uint32_t>(),
                             dinfo.as<unsigned long long>(), st);
    }
};

void keep_info(uint64_t npat, const unsigned long long *v)
{
    t_info.patterns = npat;
    t_info.nodes = v[0];
    t_info.occ_lines = v[1];
    t_info.leaves = v[2];
    t_info.hits = v[3];
}

} // namespace
} // namespace polyhip

using namespace polyhip;

extern "C" {

int polyhip_bwt_count_mismatch(const polyhip_bwt *hp, const uint8_t *pat, const uint64_t *off, uint64_t npat, uint32_t k,
                               uint32_t *counts, uint32_t *err)
{
    if (k > POLYHIP_BWT_MAX_MISMATCHES)
        return set_error(POLYHIP_ERR_UNSUPPORTED, "polyhip_bwt_count_mismatch: k = %u, at most %u mismatches are supported", k,
                         POLYHIP_BWT_MAX_MISMATCHES);
    PH_REQUIRE(hp, "polyhip_bwt_count_mismatch: null handle");
    t_info = polyhip_bwt_mismatch_info{};
    if (npat == 0)
        return POLYHIP_OK;
    PH_REQUIRE(off && counts && err && (pat || off[npat] == off[0]), "polyhip_bwt_count_mismatch: null argument");
    PH_REQUIRE(offsets_ok(off, npat), "polyhip_bwt_count_mismatch: offsets are not ascending");
    const BwtHandle *h = as_h(hp);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    hipStream_t st = h->stream;
    CountPass cp;
    SyncOnExit sync(st);
    if (int r = cp.run(h, pat, off, npat, k, st))
        return r;
    unsigned long long info[4];
    PH_HIP(hipMemcpyAsync(counts, cp.dcounts.p, npat * (k + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(err, cp.derr.p, npat * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(info, cp.dinfo.p, sizeof info, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    keep_info(npat, info);
    return POLYHIP_OK;
}

int polyhip_bwt_locate_mismatch(const polyhip_bwt *hp, const uint8_t *pat, const uint64_t *off, uint64_t npat, uint32_t k,
                                uint64_t *first, uint32_t *pos, uint8_t *mm, uint64_t capacity, uint32_t *err)
{
    if (k > POLYHIP_BWT_MAX_MISMATCHES)
        return set_error(POLYHIP_ERR_UNSUPPORTED, "polyhip_bwt_locate_mismatch: k = %u, at most %u mismatches are supported", k,
                         POLYHIP_BWT_MAX_MISMATCHES);
    PH_REQUIRE(hp && first, "polyhip_bwt_locate_mismatch: null argument");
    t_info = polyhip_bwt_mismatch_info{};
    if (npat == 0) {
        first[0] = 0;
        return POLYHIP_OK;
    }
    PH_REQUIRE(off && err && (pat || off[npat] == off[0]), "polyhip_bwt_locate_mismatch: null argument");
    PH_REQUIRE(capacity == 0 || (pos && mm), "polyhip_bwt_locate_mismatch: null output");
    PH_REQUIRE(offsets_ok(off, npat), "polyhip_bwt_locate_mismatch: offsets are not ascending");
    const BwtHandle *h = as_h(hp);
    PH_REQUIRE(pos_bits_of(h) + bits_for(npat - 1) <= 64, "polyhip_bwt_locate_mismatch: %llu patterns are too many for one call",
               (unsigned long long)npat);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    hipStream_t st = h->stream;
    CountPass cp;
    DevBuf dfirst, dscan, dka, dkb, dva, dvb, dhist, dscr, dpos, dmm;
    PH_HIP(dfirst.alloc((npat + 1) * sizeof(uint64_t)));
    PH_HIP(dscan.alloc(scan_scratch_bytes<uint64_t>(npat)));
    SyncOnExit sync(st);
    if (int r = cp.run(h, pat, off, npat, k, st))
        return r;
    if (int r = first_launch(cp.dcounts.as<uint32_t>(), npat, k, dfirst.as<uint64_t>(), dscan.as<uint8_t>(), st))
        return r;
    unsigned long long info[4];
    PH_HIP(hipMemcpyAsync(first, dfirst.p, (npat + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(err, cp.derr.p, npat * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(info, cp.dinfo.p, sizeof info, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    keep_info(npat, info);
    const uint64_t total = first[npat];
    if (total > capacity)
        return set_error(POLYHIP_ERR_INVALID, "polyhip_bwt_locate_mismatch: the hits need %llu entries, the buffers hold %llu",
                         (unsigned long long)total, (unsigned long long)capacity);
    if (total == 0)
        return POLYHIP_OK;
    // only now, bounded by the caller's capacity: the sort's two (key, value) buffers, its histogram and the result
    const uint64_t hist_items = 256 * radix_blocks(total) + 1;
    PH_HIP(dka.alloc(total * sizeof(uint64_t)));
    PH_HIP(dkb.alloc(total * sizeof(uint64_t)));
    PH_HIP(dva.alloc(total * sizeof(uint32_t)));
    PH_HIP(dvb.alloc(total * sizeof(uint32_t)));
    PH_HIP(dhist.alloc(hist_items * sizeof(uint32_t)));
    PH_HIP(dscr.alloc(scan_scratch_bytes<uint32_t>(hist_items)));
    PH_HIP(dpos.alloc(total * sizeof(uint32_t)));
    PH_HIP(dmm.alloc(total));
    if (int r = locate_launch(h, cp.dp.as<uint8_t>(), cp.doff.as<uint64_t>(), npat, k, dfirst.as<uint64_t>(), total, dka.as<uint64_t>(),
                              dva.as<uint32_t>(), dkb.as<uint64_t>(), dvb.as<uint32_t>(), dhist.as<uint32_t>(), dscr.as<uint8_t>(),
                              dpos.as<uint32_t>(), dmm.as<uint8_t>(), st))
        return r;
    PH_HIP(hipMemcpyAsync(pos, dpos.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(mm, dmm.p, total, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    return POLYHIP_OK;
}

int polyhip_bwt_mismatch_last_info(polyhip_bwt_mismatch_info *info)
{
    PH_REQUIRE(info, "polyhip_bwt_mismatch_last_info: null argument");
    *info = t_info;
    return POLYHIP_OK;
}

} // extern "C"
