// map_reads.hip -- place reads on an indexed text: FM-index seeds, diagonal clusters, SmithWaterman extension.
//
// The definition (include/polyhip.h, polyhip_map_reads) per read r of m bytes, strand s (q = r, or its reverse complement):
//   seeds at offsets 0, S, 2S .. while o + L <= m; a seed's occurrences p (its SA interval; none when it holds '$' or a byte
//   the text lacks; dropped and counted when more than max_occ) give hits on the diagonals d = p - o; per strand the hits
//   sorted by d are cut greedily into clusters [d0, d0 + W]; all clusters ordered by (votes desc, s, d0), the first C kept;
//   each kept one is extended by SmithWaterman(q, T[max(0, d0 - W), min(n, dmax + m + W))); the best score wins, ties to
//   the lowest rank.
// Pipeline per chunk of reads (the chunk is what the workspace holds in the worst case, max_occ hits per seed):
//   map_seed_kernel     one lane per (read, strand, seed): backward search straight on the read's bytes (strand 1 through
//                       the complement table, last byte first), interval start + width
//   scan_excl           hit offsets; the total comes back to the host (grid of the sort)
//   map_expand_kernel   64-bit keys (read * 2 + strand) << dbits | (d + max_len), one lane per seed
//   radix_sort          the LSD radix sort of device_prims.h over the key's significant bits (scan_excl comes from there too)
//   map_cluster_kernel  one wave per read: greedy clusters by ballots over 64 sorted hits at a time, the kept candidates
//                       held rank per lane (insertion by one ballot), windows out
//   scan_excl           candidate -> pair offsets; the pair count comes back to the host
//   map_pairs_kernel / map_gather_kernel   the packed A batch (strand-oriented read copies) and B batch (windows of T)
//   polyhip_sw_align_batch_dev             the existing per-pair-B SmithWaterman, strings in fixed-stride slots
//   map_reduce_kernel   one wave per read: first error, best and second score, coordinates from the strings' gap counts
//   map_strings_kernel  the chosen pair's strings packed behind the previous chunk's
// polyhip_map_reads_affine (Gotoh's affine gaps in the extension) shares everything up to the gather, then:
//   k3a::score_pass     the affine score pass (sw_affine.h) on all pairs
//   map_reduce_kernel<true>   the same reduction without the strings' part; a flag per mapped read
//   scan_excl           read -> winner slots; the winners' count comes back to the host
//   map_winners_kernel / map_wgather_kernel   the winners' scores, end cells and sequences as a compact batch
//   k3a::traceback_pass the affine traceback of the winners only, in sub-chunks whose direction words fit the cap
//   map_finish_kernel   ref_start / read_start from the winner's strings, string lengths, traced cells
//   map_strings_kernel  as above, from the winners' slots
// polyhip_map_pairs (paired-end reads: mates interleaved into one batch of 2 * npairs reads) runs the affine candidate pass, then:
//   pair_reduce_kernel   one wave per pair: the best proper combination of the mates' candidates, or the rescue requests
//   rescue_plan_kernel / rescue_gather_kernel   the requests as a second pair batch: the mate beside the window its partner implies
//   k3a::score_pass      on that batch
//   pair_resolve_kernel  one wave per pair: the rescue's success test and tie rule, the per-mate outputs, tlen, the winners' sources
//   pair_winners_kernel / pair_wgather_kernel   the winners from either batch; the traceback, finish and strings steps as above
// polyhip_map_reads_refs / polyhip_map_pairs_refs (a reference of several contigs, refs.hip: one index over their concatenation
// C and start[0..k]) are the affine and the paired call with the REFS instantiations of four kernels and two kernels of their own:
//   map_count_refs_kernel / map_expand_refs_kernel   hits in two passes: an occurrence that straddles a boundary is no hit and
//                       the runs per seed must stay dense, so the first pass counts what each seed keeps (binary search of
//                       every located p over start[]) and the second writes keys with the contig above the local diagonal
//   map_cluster_kernel<true>   the diagonal field is wide enough for k0 + W, so clusters split at contigs by themselves;
//                       windows are clipped to the contig and kept as positions in C with the contig beside them (crid)
//   everything between (gathers, score pass, winners, traceback, finish) works on positions in C and is shared unchanged
//   map_reduce_kernel<true, true> / pair_resolve_kernel<true>   rid out, ref_end made local (ref_start follows from it)
//   pair_reduce_kernel<true>   proper only within one contig; the rescue window clipped to the anchor's contig
#include "bwt_index.h"
#include "device_prims.h"
#include "sw_affine.h"
#include "sw_scoring.h"

namespace polyhip {
namespace {

constexpr uint32_t MAP_MAX_LEN = 4096, MAP_MAX_BAND = 1024, MAP_MAX_CAND = 64; // the per-pair-B kernels' limits; a wave's lanes
constexpr uint64_t MAP_CHUNK = 256;                                              // chunks are multiples of this many reads
constexpr uint64_t MAP_TB_PAIRS = 131072; // pairs whose traceback workspace is held at once (the aligner loops beyond)
constexpr size_t MAP_WORK_CAP = 8ull << 30;

struct MapShape {
    uint32_t L, S, max_occ, W, C, strands;
    uint32_t ns;      // seed slots per (read, strand): seeds of a read of max_len bytes
    uint32_t max_len; // also the diagonal bias: d + max_len >= 0
    uint32_t dbits;   // bits of a biased diagonal
    uint64_t n;       // text length
    // a reference set (polyhip_map_*_refs; k = 0: one text): contigs, bits of a contig number, bits of a key below the
    // (read, strand) field, and the most reads whose keys fit 64 bits (0: no such limit)
    uint32_t k, cbits, kbits;
    uint64_t rcap;
};

// what the kernels of the refs calls see of the set besides the shape: start[0..k], the kept candidates' contigs, and
// where the per-entry contig goes.  All null in the single-text calls, whose instantiations never read them.
struct RefView {
    const uint32_t *start;
    uint32_t *crid;
    uint32_t *o_rid;
};

enum {
    CNT_SEEDS = 0, CNT_OVER = 1, CNT_CLUSTERS = 2, CNT_MAPPED = 3, CNT_TBCELLS = 4, CNT_PROPER = 5, CNT_RESCUED = 6, CNT_STRADDLE = 7,
    CNT_N = 8
};

// transform.complementTable (transform.go:78-109): IUPAC letters in both cases, every other byte -> 0x00
__device__ __forceinline__ uint32_t dna_complement(uint32_t b)
{
    const bool lower = b >= 'a' && b <= 'z';
    const uint32_t c = dna_complement_upper(lower ? b - 32 : b);
    return c && lower ? c + 32 : c;
}

__device__ __forceinline__ void count_add(unsigned long long *cnt, uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v)
        atomicAdd(cnt, (unsigned long long)v);
}

// One lane per seed slot.  start / width = the seed's rows of the index; width 0 for a slot past the read's last seed, a
// seed without occurrences and a seed with more than max_occ.
template <int LAYOUT>
__global__ __launch_bounds__(BT) void map_seed_kernel(Index x, const uint8_t *__restrict__ reads, const uint64_t *__restrict__ off,
                                                      uint64_t nslots, MapShape g, uint32_t *__restrict__ start,
                                                      uint32_t *__restrict__ width, unsigned long long *__restrict__ cnt)
{
    __shared__ uint8_t code[256];
    __shared__ uint8_t cmp[256];
    __shared__ uint32_t Cs[256];
    code[threadIdx.x] = x.dense[threadIdx.x];
    cmp[threadIdx.x] = (uint8_t)dna_complement(threadIdx.x);
    Cs[threadIdx.x] = x.C[threadIdx.x];
    __syncthreads();
    uint32_t nseeds = 0, nover = 0;
    const uint64_t span = (uint64_t)gridDim.x * BT;
    for (uint64_t base = blockIdx.x * (uint64_t)BT; base < nslots; base += span) {
        const uint64_t slot = base + threadIdx.x;
        if (slot < nslots) {
            const uint32_t k = (uint32_t)(slot % g.ns);
            const uint64_t rs = slot / g.ns;
            const uint32_t strand = (uint32_t)(rs % g.strands);
            const uint64_t r = rs / g.strands;
            const uint64_t a = off[r], m = off[r + 1] - a;
            const uint64_t o = (uint64_t)k * g.S;
            uint32_t s = 0, e = 0;
            if (m <= g.max_len && o + g.L <= m) {
                ++nseeds;
                e = x.N;
                // q[o + j] for j = L - 1 .. 0: strand 1 reads the read forwards through the complement table
                const uint8_t *p = strand ? reads + a + (m - o - g.L) : reads + a + o + (g.L - 1);
                for (uint32_t j = 0; j < g.L && s < e; ++j) {
                    const uint8_t raw = strand ? p[j] : *(p - j);
                    const uint8_t ch = strand ? cmp[raw] : raw;
                    const uint32_t c = code[ch];
                    if (ch == NULL_CHAR || c == 0xFFu) {
                        s = e = 0;
                        break;
                    }
                    if (LAYOUT == 0) {
                        s = Cs[c] + occ_nuc(x, c, s);
                        e = Cs[c] + occ_nuc(x, c, e);
                    } else {
                        s = Cs[c] + occ_gen(x, c, ch, s);
                        e = Cs[c] + occ_gen(x, c, ch, e);
                    }
                }
            }
            uint32_t w = e > s ? e - s : 0;
            if (w > g.max_occ) {
                ++nover;
                w = 0;
            }
            start[slot] = s;
            width[slot] = w;
        }
    }
    count_add(cnt + CNT_SEEDS, nseeds);
    count_add(cnt + CNT_OVER, nover);
}

// One lane per seed slot: its hits as keys (read * 2 + strand) << dbits | (p - o + max_len), value p
__global__ __launch_bounds__(BT) void map_expand_kernel(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ start,
                                                        const uint32_t *__restrict__ first, uint64_t nslots, MapShape g,
                                                        uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    for (uint64_t slot = blockIdx.x * (uint64_t)BT + threadIdx.x; slot < nslots; slot += (uint64_t)gridDim.x * BT) {
        const uint32_t f = first[slot], w = first[slot + 1] - f;
        if (w == 0)
            continue;
        const uint32_t k = (uint32_t)(slot % g.ns);
        const uint64_t rs = slot / g.ns;
        const uint64_t r = rs / g.strands, strand = rs % g.strands;
        const uint64_t hi = (r * 2 + strand) << g.dbits;
        const uint64_t bias = (uint64_t)g.max_len - (uint64_t)k * g.S; // >= 0: a seed starts inside the read
        const uint32_t s = start[slot];
        for (uint32_t t = 0; t < w; ++t) {
            const uint32_t p = sa[s + t];
            keys[f + t] = hi | ((uint64_t)p + bias);
            vals[f + t] = p;
        }
    }
}

// ---- hits on a reference set -----------------------------------------------------------------------------------------------
// the contig of position p < start[k]: start[c] <= p < start[c + 1]
__device__ __forceinline__ uint32_t find_contig(const uint32_t *__restrict__ start, uint32_t k, uint32_t p)
{
    uint32_t lo = 0, hi = k;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (start[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Occurrences that straddle a boundary are no hits, and the sort, first[] and the cluster kernel want dense per-seed runs:
// two passes.  The counting pass, one lane per seed slot: width[slot] keeps the seed's rows, first[slot] (the rows on
// entry) becomes the occurrences that lie inside one contig; the dropped ones are counted.
__global__ __launch_bounds__(BT) void map_count_refs_kernel(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ start,
                                                            uint64_t nslots, MapShape g, const uint32_t *__restrict__ cstart,
                                                            uint32_t *__restrict__ first, uint32_t *__restrict__ width,
                                                            unsigned long long *__restrict__ cnt)
{
    uint32_t dropped = 0;
    const uint64_t span = (uint64_t)gridDim.x * BT;
    for (uint64_t base = blockIdx.x * (uint64_t)BT; base < nslots; base += span) {
        const uint64_t slot = base + threadIdx.x;
        if (slot < nslots) {
            const uint32_t w = first[slot], s = start[slot];
            uint32_t kept = 0;
            for (uint32_t t = 0; t < w; ++t) {
                const uint32_t p = sa[s + t];
                const uint32_t c = find_contig(cstart, g.k, p);
                kept += p + g.L <= cstart[c + 1];
            }
            width[slot] = w;
            first[slot] = kept;
            dropped += w - kept;
        }
    }
    count_add(cnt + CNT_STRADDLE, dropped);
}

// The write pass: a slot's kept hits as keys ((read * 2 + strand) << cbits | c) << dbits | (p - start_c - o + max_len)
__global__ __launch_bounds__(BT) void map_expand_refs_kernel(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ start,
                                                             const uint32_t *__restrict__ width, const uint32_t *__restrict__ first,
                                                             uint64_t nslots, MapShape g, const uint32_t *__restrict__ cstart,
                                                             uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    for (uint64_t slot = blockIdx.x * (uint64_t)BT + threadIdx.x; slot < nslots; slot += (uint64_t)gridDim.x * BT) {
        uint32_t f = first[slot];
        const uint32_t end = first[slot + 1], w = width[slot];
        if (f == end)
            continue;
        const uint32_t k = (uint32_t)(slot % g.ns);
        const uint64_t rs = slot / g.ns;
        const uint64_t r = rs / g.strands, strand = rs % g.strands;
        const uint64_t hi = (r * 2 + strand) << g.cbits;
        const uint64_t bias = (uint64_t)g.max_len - (uint64_t)k * g.S; // >= 0: a seed starts inside the read
        const uint32_t s = start[slot];
        for (uint32_t t = 0; t < w && f < end; ++t) {
            const uint32_t p = sa[s + t];
            const uint32_t c = find_contig(cstart, g.k, p), b = cstart[c];
            if (p + g.L > cstart[c + 1])
                continue;
            keys[f] = ((hi | c) << g.dbits) | ((uint64_t)(p - b) + bias);
            vals[f] = p;
            ++f;
        }
    }
}

// One wave per read over its sorted hits.  Lane i holds the candidate of rank i: a new cluster goes behind every kept one
// with at least its votes (clusters arrive in (strand, d0) order, which is the order among equal votes).
// REFS: the keys hold the contig above the local diagonal, in a field wide enough that k0 + W never carries into it, so
// clusters split at contigs without a test and arrive in (strand, contig, d0) order; a window is clipped to its contig and
// kept in C's coordinates (clo = start_c + lo), with the contig beside it.
template <bool REFS>
__global__ __launch_bounds__(BT) void map_cluster_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ first,
                                                         const uint64_t *__restrict__ off, uint64_t nreads, MapShape g,
                                                         uint32_t *__restrict__ ncand, uint32_t *__restrict__ cvotes,
                                                         uint32_t *__restrict__ cstrand, uint32_t *__restrict__ clo,
                                                         uint32_t *__restrict__ chi, RefView rv, unsigned long long *__restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    const uint64_t dmask = (1ull << g.dbits) - 1;
    const uint32_t cmask = REFS ? (1u << g.cbits) - 1 : 0u;
    for (uint64_t r = (blockIdx.x * (uint64_t)BT + threadIdx.x) / 64; r < nreads; r += (uint64_t)gridDim.x * (BT / 64)) {
        const int64_t m = (int64_t)(off[r + 1] - off[r]);
        uint32_t votes = 0, cs = 0, ncl = 0, cc = 0;
        uint64_t d0k = 0, dmaxk = 0; // biased diagonals
        for (uint32_t strand = 0; strand < g.strands; ++strand) {
            const uint64_t s0 = (r * g.strands + strand) * g.ns;
            uint32_t pos = first[s0];
            const uint32_t end = first[s0 + g.ns];
            while (pos < end) {
                const uint64_t k0 = keys[pos], lim = k0 + g.W;
                uint32_t n = 0;
                for (;;) { // the hits are sorted: those within the band are a prefix of each 64
                    const uint64_t i = (uint64_t)pos + n + lane;
                    const bool in = i < end && keys[i] <= lim;
                    const uint32_t c = (uint32_t)__popcll(__ballot(in));
                    n += c;
                    if (c < 64)
                        break;
                }
                const uint64_t k1 = keys[pos + n - 1];
                const int at = __popcll(__ballot(votes >= n)); // free lanes hold 0 votes, n >= 1
                const uint32_t uv = __shfl_up(votes, 1, 64), us = __shfl_up(cs, 1, 64);
                const uint64_t ud0 = __shfl_up(d0k, 1, 64), ud1 = __shfl_up(dmaxk, 1, 64);
                const uint32_t uc = REFS ? __shfl_up(cc, 1, 64) : 0u;
                if (lane > at) {
                    votes = uv, cs = us, d0k = ud0, dmaxk = ud1;
                    if (REFS)
                        cc = uc;
                } else if (lane == at) {
                    votes = n, cs = strand, d0k = k0 & dmask, dmaxk = k1 & dmask;
                    if (REFS)
                        cc = (uint32_t)(k0 >> g.dbits) & cmask;
                }
                ++ncl;
                pos += n;
            }
        }
        const uint32_t nc = min(ncl, g.C);
        if ((uint32_t)lane < nc) {
            const int64_t d0 = (int64_t)d0k - g.max_len, d1 = (int64_t)dmaxk - g.max_len;
            const int64_t lo_ = d0 - (int64_t)g.W, hi_ = d1 + m + (int64_t)g.W;
            const int64_t base = REFS ? (int64_t)rv.start[cc] : 0;
            const int64_t len = REFS ? (int64_t)rv.start[cc + 1] - base : (int64_t)g.n;
            const int64_t lo = lo_ > 0 ? lo_ : 0, hi = hi_ < len ? hi_ : len;
            const uint64_t o = r * g.C + lane;
            cvotes[o] = votes;
            cstrand[o] = cs;
            clo[o] = (uint32_t)(base + lo);
            chi[o] = (uint32_t)(base + hi);
            if (REFS)
                rv.crid[o] = cc;
        }
        if (lane == 0) {
            ncand[r] = nc;
            if (ncl)
                atomicAdd(cnt + CNT_CLUSTERS, (unsigned long long)ncl);
        }
    }
}

// One lane per (read, rank): the pair's read and the lengths of its A and B (scanned into offsets afterwards)
__global__ __launch_bounds__(BT) void map_pairs_kernel(const uint32_t *__restrict__ pfirst, const uint64_t *__restrict__ off,
                                                       const uint32_t *__restrict__ clo, const uint32_t *__restrict__ chi,
                                                       uint64_t nreads, uint32_t C, uint32_t *__restrict__ pread,
                                                       uint64_t *__restrict__ lenA, uint64_t *__restrict__ lenB)
{
    const uint64_t total = nreads * C;
    for (uint64_t i = blockIdx.x * (uint64_t)BT + threadIdx.x; i < total; i += (uint64_t)gridDim.x * BT) {
        const uint64_t r = i / C;
        const uint32_t rank = (uint32_t)(i - r * C), p0 = pfirst[r];
        if (rank >= pfirst[r + 1] - p0)
            continue;
        pread[p0 + rank] = (uint32_t)r;
        lenA[p0 + rank] = off[r + 1] - off[r];
        lenB[p0 + rank] = chi[i] - clo[i];
    }
}

// One wave per pair: A = the read on the candidate's strand, B = its window of the text
__global__ __launch_bounds__(BT) void map_gather_kernel(const uint8_t *__restrict__ reads, const uint64_t *__restrict__ off,
                                                        const uint8_t *__restrict__ text, const uint32_t *__restrict__ pread,
                                                        const uint32_t *__restrict__ pfirst, const uint32_t *__restrict__ cstrand,
                                                        const uint32_t *__restrict__ clo, uint32_t C, uint64_t npairs,
                                                        const uint64_t *__restrict__ offA, const uint64_t *__restrict__ offB,
                                                        uint8_t *__restrict__ A, uint8_t *__restrict__ B)
{
    __shared__ uint8_t cmp[256];
    cmp[threadIdx.x] = (uint8_t)dna_complement(threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (uint64_t p = (blockIdx.x * (uint64_t)BT + threadIdx.x) / 64; p < npairs; p += (uint64_t)gridDim.x * (BT / 64)) {
        const uint32_t r = pread[p];
        const uint64_t c = (uint64_t)r * C + (p - pfirst[r]);
        const uint8_t *src = reads + off[r];
        const uint64_t m = offA[p + 1] - offA[p], lb = offB[p + 1] - offB[p];
        uint8_t *da = A + offA[p], *db = B + offB[p];
        if (cstrand[c]) {
            for (uint64_t i = lane; i < m; i += 64)
                da[i] = cmp[src[m - 1 - i]];
        } else {
            for (uint64_t i = lane; i < m; i += 64)
                da[i] = src[i];
        }
        const uint8_t *t = text + clo[c];
        for (uint64_t i = lane; i < lb; i += 64)
            db[i] = t[i];
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v += __shfl_xor(v, d, 64);
    return v;
}

// One wave per read, lane i = its candidate of rank i.  slen / best: the chosen pair's string length (0 unmapped) and index.
// AFFINE: no strings exist yet: ref_start / read_start and slen are left to map_finish_kernel (0 here, which is what an
// unmapped read keeps), and wmap[r] = 1 for a mapped read.
// REFS: clo is a position in C; the entry gets its candidate's contig and a ref_end inside it.
template <bool AFFINE, bool REFS = false>
__global__ __launch_bounds__(BT) void map_reduce_kernel(const uint32_t *__restrict__ pfirst, const uint64_t *__restrict__ off, uint64_t nreads,
                                                        MapShape g, int64_t min_score, const int64_t *__restrict__ pscore,
                                                        const uint32_t *__restrict__ pendA, const uint32_t *__restrict__ pendB,
                                                        const uint32_t *__restrict__ perr, const uint32_t *__restrict__ plen,
                                                        const uint8_t *__restrict__ slotA, const uint8_t *__restrict__ slotB, uint32_t stride,
                                                        const uint32_t *__restrict__ cvotes, const uint32_t *__restrict__ cstrand,
                                                        const uint32_t *__restrict__ clo, int64_t *__restrict__ o_score,
                                                        int64_t *__restrict__ o_second, uint32_t *__restrict__ o_flags,
                                                        uint32_t *__restrict__ o_votes, uint32_t *__restrict__ o_rs, uint32_t *__restrict__ o_re,
                                                        uint32_t *__restrict__ o_qs, uint32_t *__restrict__ o_qe, uint32_t *__restrict__ o_err,
                                                        uint64_t *__restrict__ slen, uint32_t *__restrict__ best, uint32_t *__restrict__ wmap,
                                                        RefView rv, unsigned long long *__restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    uint32_t nmapped = 0;
    for (uint64_t r = (blockIdx.x * (uint64_t)BT + threadIdx.x) / 64; r < nreads; r += (uint64_t)gridDim.x * (BT / 64)) {
        const uint32_t p0 = pfirst[r], nc = pfirst[r + 1] - p0;
        const bool have = (uint32_t)lane < nc;
        const int64_t sc = have ? pscore[p0 + lane] : INT64_MIN;
        const uint32_t er = have ? perr[p0 + lane] : 0u;
        const uint64_t bad = __ballot(er != 0);
        uint32_t err = off[r + 1] - off[r] > g.max_len ? 0xFFFFFFFFu : 0u;
        if (bad)
            err = __shfl(er, __ffsll((unsigned long long)bad) - 1, 64);
        // the highest score, ties to the lowest rank
        int64_t bs = sc;
        int bi = lane;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int64_t os = __shfl_xor(bs, d, 64);
            const int oi = __shfl_xor(bi, d, 64);
            if (os > bs || (os == bs && oi < bi))
                bs = os, bi = oi;
        }
        int64_t second = have && lane != bi ? sc : 0; // 0 without another candidate
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int64_t other = __shfl_xor(second, d, 64);
            second = other > second ? other : second;
        }
        const bool mapped = nc > 0 && err == 0 && bs >= min_score;
        uint32_t len = 0, ga = 0, gb = 0;
        const uint32_t bp = p0 + (uint32_t)bi;
        if (!AFFINE && mapped) {
            len = plen[bp];
            const uint8_t *sa_ = slotA + (uint64_t)bp * stride + (stride - len), *sb_ = slotB + (uint64_t)bp * stride + (stride - len);
            for (uint32_t i = lane; i < len; i += 64) {
                ga += sa_[i] != '-';
                gb += sb_[i] != '-';
            }
            ga = wave_sum(ga);
            gb = wave_sum(gb);
        }
        if (lane == 0) {
            const uint64_t c = r * g.C + (uint32_t)bi;
            uint32_t eA = mapped ? pendA[bp] : 0u, eB = mapped ? clo[c] + pendB[bp] : 0u;
            if (REFS) {
                const uint32_t id = mapped ? rv.crid[c] : 0u;
                eB -= mapped ? rv.start[id] : 0u;
                rv.o_rid[r] = id;
            }
            o_score[r] = mapped ? bs : 0;
            o_second[r] = mapped ? second : 0;
            o_flags[r] = mapped ? 1u | (cstrand[c] << 1) : 0u;
            o_votes[r] = mapped ? cvotes[c] : 0u;
            o_re[r] = eB;
            o_rs[r] = eB - gb;
            o_qe[r] = eA;
            o_qs[r] = eA - ga;
            o_err[r] = err;
            slen[r] = len;
            best[r] = bp;
            if (AFFINE)
                wmap[r] = mapped;
            nmapped += mapped;
        }
    }
    count_add(cnt + CNT_MAPPED, nmapped);
}

// One wave per read: alnOff[r] = *base + soff[r]; the chosen pair's strings go there when they fit the buffers whole
__global__ __launch_bounds__(BT) void map_strings_kernel(const uint64_t *__restrict__ soff, const uint32_t *__restrict__ best, uint64_t nreads,
                                                         const uint8_t *__restrict__ slotA, const uint8_t *__restrict__ slotB, uint32_t stride,
                                                         const uint64_t *__restrict__ base, uint64_t *__restrict__ alnOff,
                                                         uint8_t *__restrict__ outA, uint8_t *__restrict__ outB, uint64_t capacity)
{
    const int lane = threadIdx.x & 63;
    for (uint64_t r = (blockIdx.x * (uint64_t)BT + threadIdx.x) / 64; r < nreads; r += (uint64_t)gridDim.x * (BT / 64)) {
        const uint64_t o = *base + soff[r], len = soff[r + 1] - soff[r];
        if (lane == 0)
            alnOff[r] = o;
        if (len == 0 || o + len > capacity)
            continue;
        const uint64_t src = (uint64_t)best[r] * stride + (stride - len);
        for (uint64_t i = lane; i < len; i += 64) {
            outA[o + i] = slotA[src + i];
            outB[o + i] = slotB[src + i];
        }
    }
}

// after a chunk's strings: the running total, which is also alnOff's last entry
__global__ void map_advance_kernel(uint64_t *__restrict__ base, const uint64_t *__restrict__ chunk_total, uint64_t *__restrict__ alnOff_end)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t t = *base + *chunk_total;
        *base = t;
        *alnOff_end = t;
    }
}

// ---- the affine path's own kernels ----------------------------------------------------------------------------------------
// One lane per read: a mapped read's winning pair becomes pair wfirst[r] of the compact batch the traceback runs on
__global__ __launch_bounds__(BT) void map_winners_kernel(const uint32_t *__restrict__ wfirst, const uint32_t *__restrict__ best,
                                                         uint64_t nreads, const uint64_t *__restrict__ offA, const uint64_t *__restrict__ offB,
                                                         const int64_t *__restrict__ pscore, const uint32_t *__restrict__ pendA,
                                                         const uint32_t *__restrict__ pendB, uint32_t *__restrict__ wsrc,
                                                         uint64_t *__restrict__ wlenA, uint64_t *__restrict__ wlenB,
                                                         int64_t *__restrict__ wscore, uint32_t *__restrict__ wendA,
                                                         uint32_t *__restrict__ wendB, uint32_t *__restrict__ werr)
{
    for (uint64_t r = blockIdx.x * (uint64_t)BT + threadIdx.x; r < nreads; r += (uint64_t)gridDim.x * BT) {
        const uint32_t q = wfirst[r];
        if (wfirst[r + 1] == q)
            continue;
        const uint32_t p = best[r];
        wsrc[q] = p;
        wlenA[q] = offA[p + 1] - offA[p];
        wlenB[q] = offB[p + 1] - offB[p];
        wscore[q] = pscore[p];
        wendA[q] = pendA[p];
        wendB[q] = pendB[p];
        werr[q] = 0u; // a mapped read has no candidate with an error
    }
}

// One wave per winner: its A and B copied out of the pair batch
__global__ __launch_bounds__(BT) void map_wgather_kernel(const uint32_t *__restrict__ wsrc, uint64_t nwin, const uint64_t *__restrict__ offA,
                                                         const uint64_t *__restrict__ offB, const uint8_t *__restrict__ A,
                                                         const uint8_t *__restrict__ B, const uint64_t *__restrict__ woffA,
                                                         const uint64_t *__restrict__ woffB, uint8_t *__restrict__ wA, uint8_t *__restrict__ wB)
{
    const int lane = threadIdx.x & 63;
    for (uint64_t q = (blockIdx.x * (uint64_t)BT + threadIdx.x) / 64; q < nwin; q += (uint64_t)gridDim.x * (BT / 64)) {
        const uint32_t p = wsrc[q];
        const uint64_t la = woffA[q + 1] - woffA[q], lb = woffB[q + 1] - woffB[q];
        const uint8_t *sa_ = A + offA[p], *sb_ = B + offB[p];
        uint8_t *da = wA + woffA[q], *db = wB + woffB[q];
        for (uint64_t i = lane; i < la; i += 64)
            da[i] = sa_[i];
        for (uint64_t i = lane; i < lb; i += 64)
            db[i] = sb_[i];
    }
}

// every pair of a traceback sub-chunk owns the direction words of the largest window: no planning from scores
__global__ __launch_bounds__(BT) void map_diroff_kernel(uint64_t *__restrict__ dirOff, uint64_t n, uint64_t words)
{
    for (uint64_t q = blockIdx.x * (uint64_t)BT + threadIdx.x; q < n; q += (uint64_t)gridDim.x * BT)
        dirOff[q] = q * words;
}

// One wave per read, after the winners' traceback: coordinates from the strings' gap counts, the string's length, and
// best[r] = the winner's slot for map_strings_kernel.  An unmapped read keeps what map_reduce_kernel<true> wrote.
__global__ __launch_bounds__(BT) void map_finish_kernel(const uint32_t *__restrict__ wfirst, uint64_t nreads, const uint32_t *__restrict__ wlen,
                                                        const uint8_t *__restrict__ slotA, const uint8_t *__restrict__ slotB, uint32_t stride,
                                                        const int64_t *__restrict__ wscore, const uint32_t *__restrict__ wendA,
                                                        const uint32_t *__restrict__ wendB, int smax, int ge,
                                                        const uint32_t *__restrict__ o_re, const uint32_t *__restrict__ o_qe,
                                                        uint32_t *__restrict__ o_rs, uint32_t *__restrict__ o_qs, uint64_t *__restrict__ slen,
                                                        uint32_t *__restrict__ best, unsigned long long *__restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    unsigned long long cells = 0;
    for (uint64_t r = (blockIdx.x * (uint64_t)BT + threadIdx.x) / 64; r < nreads; r += (uint64_t)gridDim.x * (BT / 64)) {
        const uint32_t q = wfirst[r];
        if (wfirst[r + 1] == q)
            continue;
        const uint32_t len = wlen[q];
        const uint8_t *sa_ = slotA + (uint64_t)q * stride + (stride - len), *sb_ = slotB + (uint64_t)q * stride + (stride - len);
        uint32_t ga = 0, gb = 0;
        for (uint32_t i = lane; i < len; i += 64) {
            ga += sa_[i] != '-';
            gb += sb_[i] != '-';
        }
        ga = wave_sum(ga);
        gb = wave_sum(gb);
        if (lane == 0) {
            o_rs[r] = o_re[r] - gb;
            o_qs[r] = o_qe[r] - ga;
            slen[r] = len;
            best[r] = q;
            cells += (unsigned long long)wendA[q] * k3a::window_cols(wendA[q], wendB[q], wscore[q], smax, ge);
        }
    }
    if (lane == 0 && cells)
        atomicAdd(cnt + CNT_TBCELLS, cells);
}

// ---- polyhip_map_pairs' own kernels ---------------------------------------------------------------------------------------
// mates in one packed batch: read 2i = mate 1 of pair i, read 2i + 1 = mate 2.  One lane per pair: the lengths (scanned
// into offsets afterwards) ...
__global__ __launch_bounds__(BT) void pair_lens_kernel(const uint64_t *__restrict__ off1, const uint64_t *__restrict__ off2, uint64_t npairs,
                                                       uint64_t *__restrict__ len)
{
    for (uint64_t i = blockIdx.x * (uint64_t)BT + threadIdx.x; i < npairs; i += (uint64_t)gridDim.x * BT) {
        len[2 * i] = off1[i + 1] - off1[i];
        len[2 * i + 1] = off2[i + 1] - off2[i];
    }
}

// ... and one wave per mate: its bytes
__global__ __launch_bounds__(BT) void pair_interleave_kernel(const uint8_t *__restrict__ reads1, const uint64_t *__restrict__ off1,
                                                             const uint8_t *__restrict__ reads2, const uint64_t *__restrict__ off2,
                                                             uint64_t nreads, const uint64_t *__restrict__ off, uint8_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    for (uint64_t r = (blockIdx.x * (uint64_t)BT + threadIdx.x) / 64; r < nreads; r += (uint64_t)gridDim.x * (BT / 64)) {
        const uint8_t *src = r & 1 ? reads2 + off2[r >> 1] : reads1 + off1[r >> 1];
        const uint64_t o = off[r], m = off[r + 1] - o;
        for (uint64_t i = lane; i < m; i += 64)
            out[o + i] = src[i];
    }
}

struct PairShape {
    int64_t min_insert, max_insert;
    uint32_t rescue;
};

// a (strand, left, length) and b: the insert when they are a proper combination (forward-reverse, neither end of the
// forward mate beyond the reverse mate's, insert within the bounds), else -1
__device__ __forceinline__ int64_t proper_insert(uint32_t sa, int64_t la, int64_t ma, uint32_t sb, int64_t lb, int64_t mb, const PairShape &q)
{
    if (sa == sb)
        return -1;
    const int64_t lf = sa ? lb : la, rf = sa ? lb + mb : la + ma; // the mate on strand 0
    const int64_t lr = sa ? la : lb, rr = sa ? la + ma : lb + mb; // the mate on strand 1
    const int64_t ins = rr - lf;
    return lf <= lr && rf <= rr && ins >= q.min_insert && ins <= q.max_insert ? ins : -1;
}

// What one wave knows of a mate, lane i = its candidate of rank i
struct MateCands {
    uint32_t nc, err, strand;
    int64_t m, score, left; // left = lo + endB - endA: where q[0] lands along the end cell's diagonal
    int bi;                 // the single-read winner's rank ...
    bool mapped, usable;    // ... which exists; this lane's candidate is usable
    uint32_t rid;           // REFS: the candidate's contig (left is a position in C)
};

template <bool REFS>
__device__ __forceinline__ MateCands load_mate(uint64_t r, int lane, const uint32_t *__restrict__ pfirst, const uint64_t *__restrict__ off,
                                               const MapShape &g, int64_t min_score, const int64_t *__restrict__ pscore,
                                               const uint32_t *__restrict__ pendA, const uint32_t *__restrict__ pendB,
                                               const uint32_t *__restrict__ perr, const uint32_t *__restrict__ cstrand,
                                               const uint32_t *__restrict__ clo, const RefView &rv)
{
    MateCands c;
    const uint32_t p0 = pfirst[r];
    c.nc = pfirst[r + 1] - p0;
    c.m = (int64_t)(off[r + 1] - off[r]);
    const bool have = (uint32_t)lane < c.nc;
    c.score = have ? pscore[p0 + lane] : INT64_MIN;
    const uint32_t er = have ? perr[p0 + lane] : 0u;
    const uint64_t bad = __ballot(er != 0);
    c.err = (uint64_t)c.m > g.max_len ? 0xFFFFFFFFu : 0u;
    if (bad)
        c.err = __shfl(er, __ffsll((unsigned long long)bad) - 1, 64);
    c.strand = have ? cstrand[r * g.C + lane] : 0u;
    c.left = have ? (int64_t)clo[r * g.C + lane] + (int64_t)pendB[p0 + lane] - (int64_t)pendA[p0 + lane] : 0;
    c.rid = REFS && have ? rv.crid[r * g.C + lane] : 0u;
    int64_t bs = c.score;
    int bi = lane;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t os = __shfl_xor(bs, d, 64);
        const int oi = __shfl_xor(bi, d, 64);
        if (os > bs || (os == bs && oi < bi))
            bs = os, bi = oi;
    }
    c.bi = bi;
    c.mapped = c.nc > 0 && c.err == 0 && bs >= min_score;
    c.usable = have && c.err == 0 && c.score >= min_score;
    return c;
}

// One wave per pair, after the candidates' score pass.  The proper combinations (k1, k2) are spread over the lanes, 64 at
// a time, each lane fetching its two candidates from the lanes that hold them; the best has the highest sum, then the
// smallest k1, then the smallest k2, which is the smallest k1 * nc2 + k2.  Out: err of both mates; choice = the rank
// pairing chose, or without a proper combination the single-read winner's (-1: none); proper / insert of the pair; and
// then the rescue requests, kept under the mate to rescue: rvalid = 1, the query's strand, the clipped window.
// REFS: a combination is proper only within one contig (projections are positions in C, so their differences are the local
// ones), and a rescue window is clipped to the anchor's contig.
template <bool REFS>
__global__ __launch_bounds__(BT) void pair_reduce_kernel(const uint32_t *__restrict__ pfirst, const uint64_t *__restrict__ off, uint64_t npairs,
                                                         MapShape g, PairShape q, int64_t min_score, const int64_t *__restrict__ pscore,
                                                         const uint32_t *__restrict__ pendA, const uint32_t *__restrict__ pendB,
                                                         const uint32_t *__restrict__ perr, const uint32_t *__restrict__ cstrand,
                                                         const uint32_t *__restrict__ clo, uint32_t *__restrict__ o_err,
                                                         int32_t *__restrict__ choice, uint32_t *__restrict__ proper,
                                                         int64_t *__restrict__ ptlen, uint32_t *__restrict__ rvalid,
                                                         uint32_t *__restrict__ rstrand, uint32_t *__restrict__ rlo, uint32_t *__restrict__ rhi,
                                                         RefView rv)
{
    const int lane = threadIdx.x & 63;
    for (uint64_t i = (blockIdx.x * (uint64_t)BT + threadIdx.x) / 64; i < npairs; i += (uint64_t)gridDim.x * (BT / 64)) {
        const MateCands a = load_mate<REFS>(2 * i, lane, pfirst, off, g, min_score, pscore, pendA, pendB, perr, cstrand, clo, rv);
        const MateCands b = load_mate<REFS>(2 * i + 1, lane, pfirst, off, g, min_score, pscore, pendA, pendB, perr, cstrand, clo, rv);
        int64_t bsum = INT64_MIN, bins = 0;
        uint32_t bt = 0xFFFFFFFFu;
        const uint32_t ncomb = a.err == 0 && b.err == 0 ? a.nc * b.nc : 0u;
        for (uint32_t t0 = 0; t0 < ncomb; t0 += 64) {
            const uint32_t t = t0 + lane;
            const bool in = t < ncomb;
            const int k1 = in ? (int)(t / b.nc) : 0, k2 = in ? (int)(t % b.nc) : 0;
            const int64_t s1 = __shfl(a.score, k1, 64), s2 = __shfl(b.score, k2, 64);
            const int64_t l1 = __shfl(a.left, k1, 64), l2 = __shfl(b.left, k2, 64);
            const uint32_t d1 = __shfl(a.strand, k1, 64), d2 = __shfl(b.strand, k2, 64);
            const int u1 = __shfl((int)a.usable, k1, 64), u2 = __shfl((int)b.usable, k2, 64);
            const bool same = !REFS || __shfl(a.rid, k1, 64) == __shfl(b.rid, k2, 64);
            const int64_t ins = in && u1 && u2 && same ? proper_insert(d1, l1, a.m, d2, l2, b.m, q) : -1;
            if (ins >= 0 && s1 + s2 > bsum) // t ascends within a lane: the first of equal sums stays
                bsum = s1 + s2, bins = ins, bt = t;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int64_t os = __shfl_xor(bsum, d, 64), oi = __shfl_xor(bins, d, 64);
            const uint32_t ot = __shfl_xor(bt, d, 64);
            if (ot != 0xFFFFFFFFu && (bt == 0xFFFFFFFFu || os > bsum || (os == bsum && ot < bt)))
                bsum = os, bins = oi, bt = ot;
        }
        const bool found = bt != 0xFFFFFFFFu;
        // the anchors of a rescue: each mate's single-read winner, fetched from the lane that holds it
        const int64_t la = __shfl(a.left, a.bi, 64), lb = __shfl(b.left, b.bi, 64);
        const uint32_t sa = __shfl(a.strand, a.bi, 64), sb = __shfl(b.strand, b.bi, 64);
        const uint32_t ca = __shfl(a.rid, a.bi, 64), cb = __shfl(b.rid, b.bi, 64);
        if (lane == 0) {
            o_err[2 * i] = a.err;
            o_err[2 * i + 1] = b.err;
            choice[2 * i] = found ? (int32_t)(bt / b.nc) : a.mapped ? a.bi : -1;
            choice[2 * i + 1] = found ? (int32_t)(bt % b.nc) : b.mapped ? b.bi : -1;
            proper[i] = found;
            ptlen[i] = found ? bins : 0;
        }
        if (lane < 2) { // lane 0: mate 1 anchors the rescue of mate 2; lane 1: the other way round
            const bool anchored = lane == 0 ? a.mapped : b.mapped;
            const uint32_t s = lane == 0 ? sa : sb, ey = lane == 0 ? b.err : a.err;
            const int64_t left = lane == 0 ? la : lb, mx = lane == 0 ? a.m : b.m, my = lane == 0 ? b.m : a.m;
            const int64_t W = g.W;
            int64_t wlo = s == 0 ? left + q.min_insert - my - W : left + mx - q.max_insert - W;
            int64_t whi = s == 0 ? left + q.max_insert + W : left + mx - q.min_insert + my + W;
            const uint32_t cx = lane == 0 ? ca : cb; // (0 without an anchor: any contig will do, nothing is asked)
            const int64_t blo = REFS ? (int64_t)rv.start[cx] : 0, bhi = REFS ? (int64_t)rv.start[cx + 1] : (int64_t)g.n;
            wlo = wlo > blo ? wlo : blo;
            whi = whi < bhi ? whi : bhi;
            const bool ask = !found && q.rescue && anchored && ey == 0 && my >= 1 && wlo < whi;
            const uint64_t y = 2 * i + 1 - lane;
            rvalid[y] = ask;
            rstrand[y] = s ^ 1u;
            rlo[y] = ask ? (uint32_t)wlo : 0u;
            rhi[y] = ask ? (uint32_t)whi : 0u;
        }
    }
}

// One lane per mate with a request: request rfirst[y] of the rescue batch, its lengths (scanned into offsets afterwards)
__global__ __launch_bounds__(BT) void rescue_plan_kernel(const uint32_t *__restrict__ rfirst, const uint64_t *__restrict__ off, uint64_t nreads,
                                                         const uint32_t *__restrict__ rlo, const uint32_t *__restrict__ rhi,
                                                         uint32_t *__restrict__ rread, uint64_t *__restrict__ lenA, uint64_t *__restrict__ lenB)
{
    for (uint64_t y = blockIdx.x * (uint64_t)BT + threadIdx.x; y < nreads; y += (uint64_t)gridDim.x * BT) {
        const uint32_t j = rfirst[y];
        if (rfirst[y + 1] == j)
            continue;
        rread[j] = (uint32_t)y;
        lenA[j] = off[y + 1] - off[y];
        lenB[j] = rhi[y] - rlo[y];
    }
}

// One wave per request: A = the mate on the strand its anchor implies, B = the window of the text
__global__ __launch_bounds__(BT) void rescue_gather_kernel(const uint8_t *__restrict__ reads, const uint64_t *__restrict__ off,
                                                           const uint8_t *__restrict__ text, const uint32_t *__restrict__ rread,
                                                           const uint32_t *__restrict__ rstrand, const uint32_t *__restrict__ rlo, uint64_t nreq,
                                                           const uint64_t *__restrict__ offA, const uint64_t *__restrict__ offB,
                                                           uint8_t *__restrict__ A, uint8_t *__restrict__ B)
{
    __shared__ uint8_t cmp[256];
    cmp[threadIdx.x] = (uint8_t)dna_complement(threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (uint64_t j = (blockIdx.x * (uint64_t)BT + threadIdx.x) / 64; j < nreq; j += (uint64_t)gridDim.x * (BT / 64)) {
        const uint32_t y = rread[j];
        const uint8_t *src = reads + off[y];
        const uint64_t m = offA[j + 1] - offA[j], lb = offB[j + 1] - offB[j];
        uint8_t *da = A + offA[j], *db = B + offB[j];
        if (rstrand[y]) {
            for (uint64_t i = lane; i < m; i += 64)
                da[i] = cmp[src[m - 1 - i]];
        } else {
            for (uint64_t i = lane; i < m; i += 64)
                da[i] = src[i];
        }
        const uint8_t *t = text + rlo[y];
        for (uint64_t i = lane; i < lb; i += 64)
            db[i] = t[i];
    }
}

constexpr uint32_t SRC_RESCUE = 0x80000000u; // a winner's source: a pair of the candidate batch, or (this bit) of the rescue batch

// One wave per pair, after the rescue score pass (rfirst is all zero when there was none).  Applies the success test and
// the tie rule of the rescue, then writes every per-mate output but ref_start / read_start (map_finish_kernel's, from the
// strings), tlen, wmap = 1 for a mapped mate and src = where its alignment is.
// REFS: every mate gets its contig (a rescued one its anchor's) and a ref_end inside it.
template <bool REFS>
__global__ __launch_bounds__(BT) void pair_resolve_kernel(const uint32_t *__restrict__ pfirst, const uint64_t *__restrict__ off, uint64_t npairs,
                                                          MapShape g, PairShape q, int64_t min_score, const int64_t *__restrict__ pscore,
                                                          const uint32_t *__restrict__ pendA, const uint32_t *__restrict__ pendB,
                                                          const uint32_t *__restrict__ cvotes, const uint32_t *__restrict__ cstrand,
                                                          const uint32_t *__restrict__ clo, const int32_t *__restrict__ choice,
                                                          const uint32_t *__restrict__ proper, const int64_t *__restrict__ ptlen,
                                                          const uint32_t *__restrict__ rfirst, const uint32_t *__restrict__ rstrand,
                                                          const uint32_t *__restrict__ rlo, const int64_t *__restrict__ rscore,
                                                          const uint32_t *__restrict__ rendA, const uint32_t *__restrict__ rendB,
                                                          const uint32_t *__restrict__ rerr, int64_t *__restrict__ o_score,
                                                          int64_t *__restrict__ o_second, uint32_t *__restrict__ o_flags,
                                                          uint32_t *__restrict__ o_votes, uint32_t *__restrict__ o_rs, uint32_t *__restrict__ o_re,
                                                          uint32_t *__restrict__ o_qs, uint32_t *__restrict__ o_qe, int64_t *__restrict__ o_tlen,
                                                          uint64_t *__restrict__ slen, uint32_t *__restrict__ src, uint32_t *__restrict__ wmap,
                                                          RefView rv, unsigned long long *__restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    uint32_t nmapped = 0, nproper = 0, nrescued = 0;
    for (uint64_t i = (blockIdx.x * (uint64_t)BT + threadIdx.x) / 64; i < npairs; i += (uint64_t)gridDim.x * (BT / 64)) {
        const bool paired = proper[i] != 0;
        int64_t tlen = ptlen[i];
        int resc = -1; // the mate that is placed by a rescue (0 or 1)
        if (!paired && q.rescue) {
            int64_t best = INT64_MIN;
            for (int yy = 1; yy >= 0; --yy) { // the attempt anchored on mate 1 first: it keeps a tie
                const uint64_t y = 2 * i + yy, x = 2 * i + 1 - yy;
                const uint32_t j = rfirst[y];
                if (rfirst[y + 1] == j || rerr[j] != 0 || rscore[j] < min_score)
                    continue;
                const uint32_t px = pfirst[x] + (uint32_t)choice[x];
                const uint64_t cx = x * g.C + (uint32_t)choice[x];
                const int64_t la = (int64_t)clo[cx] + (int64_t)pendB[px] - (int64_t)pendA[px];
                const int64_t ly = (int64_t)rlo[y] + (int64_t)rendB[j] - (int64_t)rendA[j];
                const int64_t ins = proper_insert(cstrand[cx], la, (int64_t)(off[x + 1] - off[x]), rstrand[y], ly,
                                                  (int64_t)(off[y + 1] - off[y]), q);
                if (ins >= 0 && pscore[px] + rscore[j] > best)
                    best = pscore[px] + rscore[j], resc = yy, tlen = ins;
            }
        }
        for (int x = 0; x < 2; ++x) {
            const uint64_t r = 2 * i + x;
            const uint32_t p0 = pfirst[r], nc = pfirst[r + 1] - p0;
            const int ch = choice[r];
            const bool rescued = resc == x, mapped = rescued || ch >= 0;
            // second: the best of the kept candidates but the chosen one (a rescued mate chose none of them)
            int64_t second = (uint32_t)lane < nc && (rescued || lane != ch) ? pscore[p0 + lane] : INT64_MIN;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const int64_t other = __shfl_xor(second, d, 64);
                second = other > second ? other : second;
            }
            if (second == INT64_MIN)
                second = 0;
            if (lane == 0) {
                const uint32_t pair_bits = paired || resc >= 0 ? 4u : 0u;
                if (rescued) {
                    const uint32_t j = rfirst[r];
                    o_score[r] = rscore[j];
                    o_flags[r] = 1u | (rstrand[r] << 1) | pair_bits | 8u;
                    o_votes[r] = 0;
                    uint32_t base = 0;
                    if (REFS) {
                        const uint64_t ax = 2 * i + 1 - x; // the anchor: the other mate's chosen candidate
                        const uint32_t id = rv.crid[ax * g.C + (uint32_t)choice[ax]];
                        base = rv.start[id];
                        rv.o_rid[r] = id;
                    }
                    o_re[r] = rlo[r] + rendB[j] - base;
                    o_qe[r] = rendA[j];
                    src[r] = SRC_RESCUE | j;
                } else if (mapped) {
                    const uint32_t bp = p0 + (uint32_t)ch;
                    const uint64_t c = r * g.C + (uint32_t)ch;
                    o_score[r] = pscore[bp];
                    o_flags[r] = 1u | (cstrand[c] << 1) | pair_bits;
                    o_votes[r] = cvotes[c];
                    uint32_t base = 0;
                    if (REFS) {
                        const uint32_t id = rv.crid[c];
                        base = rv.start[id];
                        rv.o_rid[r] = id;
                    }
                    o_re[r] = clo[c] + pendB[bp] - base;
                    o_qe[r] = pendA[bp];
                    src[r] = bp;
                } else {
                    if (REFS)
                        rv.o_rid[r] = 0;
                    o_score[r] = 0;
                    o_flags[r] = 0;
                    o_votes[r] = 0;
                    o_re[r] = 0;
                    o_qe[r] = 0;
                    src[r] = 0;
                }
                o_second[r] = mapped ? second : 0;
                o_rs[r] = 0;
                o_qs[r] = 0;
                slen[r] = 0;
                wmap[r] = mapped;
                nmapped += mapped;
            }
        }
        if (lane == 0) {
            o_tlen[i] = paired || resc >= 0 ? tlen : 0;
            nproper += paired || resc >= 0;
            nrescued += resc >= 0;
        }
    }
    count_add(cnt + CNT_MAPPED, nmapped);
    count_add(cnt + CNT_PROPER, nproper);
    count_add(cnt + CNT_RESCUED, nrescued);
}

// map_winners_kernel / map_wgather_kernel for winners that lie in either batch
__global__ __launch_bounds__(BT) void pair_winners_kernel(const uint32_t *__restrict__ wfirst, const uint32_t *__restrict__ src, uint64_t nreads,
                                                          const uint64_t *__restrict__ offA, const uint64_t *__restrict__ offB,
                                                          const int64_t *__restrict__ pscore, const uint32_t *__restrict__ pendA,
                                                          const uint32_t *__restrict__ pendB, const uint64_t *__restrict__ roffA,
                                                          const uint64_t *__restrict__ roffB, const int64_t *__restrict__ rscore,
                                                          const uint32_t *__restrict__ rendA, const uint32_t *__restrict__ rendB,
                                                          uint32_t *__restrict__ wsrc, uint64_t *__restrict__ wlenA, uint64_t *__restrict__ wlenB,
                                                          int64_t *__restrict__ wscore, uint32_t *__restrict__ wendA,
                                                          uint32_t *__restrict__ wendB, uint32_t *__restrict__ werr)
{
    for (uint64_t r = blockIdx.x * (uint64_t)BT + threadIdx.x; r < nreads; r += (uint64_t)gridDim.x * BT) {
        const uint32_t w = wfirst[r];
        if (wfirst[r + 1] == w)
            continue;
        const uint32_t s = src[r], p = s & ~SRC_RESCUE;
        const bool resc = (s & SRC_RESCUE) != 0;
        wsrc[w] = s;
        wlenA[w] = resc ? roffA[p + 1] - roffA[p] : offA[p + 1] - offA[p];
        wlenB[w] = resc ? roffB[p + 1] - roffB[p] : offB[p + 1] - offB[p];
        wscore[w] = resc ? rscore[p] : pscore[p];
        wendA[w] = resc ? rendA[p] : pendA[p];
        wendB[w] = resc ? rendB[p] : pendB[p];
        werr[w] = 0u;
    }
}

__global__ __launch_bounds__(BT) void pair_wgather_kernel(const uint32_t *__restrict__ wsrc, uint64_t nwin, const uint64_t *__restrict__ offA,
                                                          const uint64_t *__restrict__ offB, const uint8_t *__restrict__ A,
                                                          const uint8_t *__restrict__ B, const uint64_t *__restrict__ roffA,
                                                          const uint64_t *__restrict__ roffB, const uint8_t *__restrict__ rA,
                                                          const uint8_t *__restrict__ rB, const uint64_t *__restrict__ woffA,
                                                          const uint64_t *__restrict__ woffB, uint8_t *__restrict__ wA, uint8_t *__restrict__ wB)
{
    const int lane = threadIdx.x & 63;
    for (uint64_t w = (blockIdx.x * (uint64_t)BT + threadIdx.x) / 64; w < nwin; w += (uint64_t)gridDim.x * (BT / 64)) {
        const uint32_t s = wsrc[w], p = s & ~SRC_RESCUE;
        const bool resc = (s & SRC_RESCUE) != 0;
        const uint64_t la = woffA[w + 1] - woffA[w], lb = woffB[w + 1] - woffB[w];
        const uint8_t *sa_ = resc ? rA + roffA[p] : A + offA[p], *sb_ = resc ? rB + roffB[p] : B + offB[p];
        uint8_t *da = wA + woffA[w], *db = wB + woffB[w];
        for (uint64_t i = lane; i < la; i += 64)
            da[i] = sa_[i];
        for (uint64_t i = lane; i < lb; i += 64)
            db[i] = sb_[i];
    }
}

// ---- the workspace of a chunk of nr reads ---------------------------------------------------------------------------------
struct MapWork {
    unsigned long long *cnt; // CNT_N counters, then the strings' running total
    uint32_t *start, *first;
    uint64_t *ka, *kb;
    uint32_t *va, *vb, *hist;
    uint8_t *scratch;
    uint32_t *pfirst, *cvotes, *cstrand, *clo, *chi, *pread;
    uint64_t *offA, *offB;
    uint8_t *A, *B;
    int64_t *score;
    uint32_t *endA, *endB, *err, *alnLen;
    uint8_t *slotA, *slotB;
    void *sw_work, *tb_work;
    size_t sw_bytes, tb_bytes;
    uint64_t *soff;
    uint32_t *best;
    uint64_t hcap, pcap;
    uint32_t lenB, stride;
    // the affine path's (instead of sw_work / tb_work; slotA / slotB hold the winners' strings only)
    void *band;
    unsigned blocks; // workgroups the band scratch is sized for
    uint32_t *wfirst, *wsrc, *wendA, *wendB, *werr, *wlen, *dir;
    uint64_t *woffA, *woffB, *dirOff;
    uint8_t *wA, *wB;
    int64_t *wscore;
    uint64_t sub, dwords; // pairs per traceback sub-chunk; direction words of each
    uint32_t lenW;        // the widest window a winner can have: lenB, or a rescue window
    // polyhip_map_pairs': per mate the candidate pairing chose (-1 none), per pair proper / insert, the rescue requests by
    // rescued mate, and the rescue batch with its scores
    int32_t *choice;
    uint32_t *proper, *rfirst, *rstrand, *rlo, *rhi, *rread, *rendA, *rendB, *rerr;
    int64_t *ptlen, *rscore;
    uint64_t *roffA, *roffB;
    uint8_t *rA, *rB;
    // the refs calls': every seed's rows (first[] holds the kept hits), every kept candidate's contig
    uint32_t *width, *crid;
};

// polyhip_map_reads_affine's gaps and what k3a::choose() fixed for the call
struct MapAffine {
    int go, ge;
    k3a::Choice c;
    // polyhip_map_pairs: the reads are mates (2i, 2i + 1), and the winners' windows are up to `wide` columns (a rescue
    // window; 0: none is wider than a candidate's)
    bool pairs = false;
    uint32_t wide = 0;
};

// carves the chunk's arrays out of `base` (nullptr: sizes only) and returns the bytes; 0 = the chunk cannot be held at all
// (2^31 hits or more)
size_t map_carve(const polyhip_scoring *sc, const MapShape &g, const MapAffine *af, uint64_t nr, uint8_t *base, MapWork *out)
{
    MapWork w{};
    const uint64_t slots = nr * g.strands * g.ns;
    w.hcap = slots * g.max_occ;
    w.pcap = nr * g.C;
    if (w.hcap >= (1ull << 31) || w.pcap >= (1ull << 31) || (g.rcap && nr > g.rcap))
        return 0;
    w.lenB = g.max_len + 3 * g.W;
    w.lenW = af ? std::max(w.lenB, af->wide) : w.lenB;
    w.stride = af ? k3a::slot_stride(g.max_len, w.lenW) : polyhip_sw_traceback_stride(sc, g.max_len, w.lenB);
    const uint64_t nb = radix_blocks(std::max<uint64_t>(w.hcap, 1));
    Carve c{base};
    w.cnt = c.take<unsigned long long>(CNT_N + 1);
    w.start = c.take<uint32_t>(slots);
    w.first = c.take<uint32_t>(slots + 1);
    w.ka = c.take<uint64_t>(w.hcap);
    w.kb = c.take<uint64_t>(w.hcap);
    w.va = c.take<uint32_t>(w.hcap);
    w.vb = c.take<uint32_t>(w.hcap);
    w.hist = c.take<uint32_t>(256 * nb + 1);
    const size_t sb = std::max(std::max(scan_scratch_bytes<uint32_t>(256 * nb), scan_scratch_bytes<uint32_t>(slots)),
                               std::max(scan_scratch_bytes<uint64_t>(w.pcap), scan_scratch_bytes<uint64_t>(nr)));
    w.scratch = c.take<uint8_t>(sb);
    w.pfirst = c.take<uint32_t>(nr + 1);
    w.cvotes = c.take<uint32_t>(w.pcap);
    w.cstrand = c.take<uint32_t>(w.pcap);
    w.clo = c.take<uint32_t>(w.pcap);
    w.chi = c.take<uint32_t>(w.pcap);
    w.pread = c.take<uint32_t>(w.pcap);
    w.offA = c.take<uint64_t>(w.pcap + 1);
    w.offB = c.take<uint64_t>(w.pcap + 1);
    w.A = c.take<uint8_t>(w.pcap * g.max_len + 64); // (the aligner's vector loads run a few bytes past a sequence)
    w.B = c.take<uint8_t>(w.pcap * w.lenB + 64);
    w.score = c.take<int64_t>(w.pcap);
    w.endA = c.take<uint32_t>(w.pcap);
    w.endB = c.take<uint32_t>(w.pcap);
    w.err = c.take<uint32_t>(w.pcap);
    w.alnLen = c.take<uint32_t>(w.pcap);
    if (af) {
        // the score pass's band scratch serves the traceback too (fewer pairs, the same columns); the direction words of
        // a sub-chunk are the worst case per pair, held under the affine call's cap
        w.blocks = k3a::grid_blocks(af->c, std::max<uint64_t>(w.pcap, 1), w.lenB);
        size_t band = k3a::band_bytes(w.blocks, w.lenB);
        if (w.lenW > w.lenB) // at most nr pairs (rescue requests, winners) run at the wider window
            band = std::max(band, k3a::band_bytes(k3a::grid_blocks(af->c, std::max<uint64_t>(nr, 1), w.lenW), w.lenW));
        w.band = c.take<uint8_t>(band);
        w.dwords = k3a::dir_words(g.max_len, w.lenW);
        w.sub = std::min(std::min(af->c.chunk_pairs, af->c.dir_cap / std::max<uint64_t>(w.dwords * 4, 1)), nr);
        w.sub = std::max<uint64_t>(w.sub, 1);
        w.wfirst = c.take<uint32_t>(nr + 1);
        w.wsrc = c.take<uint32_t>(nr);
        w.woffA = c.take<uint64_t>(nr + 1);
        w.woffB = c.take<uint64_t>(nr + 1);
        w.wA = c.take<uint8_t>(nr * g.max_len + 64);
        w.wB = c.take<uint8_t>(nr * w.lenW + 64);
        w.wscore = c.take<int64_t>(nr);
        w.wendA = c.take<uint32_t>(nr);
        w.wendB = c.take<uint32_t>(nr);
        w.werr = c.take<uint32_t>(nr);
        w.wlen = c.take<uint32_t>(nr);
        w.dirOff = c.take<uint64_t>(w.sub);
        w.dir = c.take<uint32_t>(w.sub * w.dwords + 4);
        w.slotA = c.take<uint8_t>(nr * w.stride);
        w.slotB = c.take<uint8_t>(nr * w.stride);
        if (af->pairs) {
            w.choice = c.take<int32_t>(nr);
            w.proper = c.take<uint32_t>(nr / 2 + 1);
            w.ptlen = c.take<int64_t>(nr / 2 + 1);
            w.rfirst = c.take<uint32_t>(nr + 1);
            w.rstrand = c.take<uint32_t>(nr);
            w.rlo = c.take<uint32_t>(nr);
            w.rhi = c.take<uint32_t>(nr);
            w.rread = c.take<uint32_t>(nr);
            w.roffA = c.take<uint64_t>(nr + 1);
            w.roffB = c.take<uint64_t>(nr + 1);
            w.rA = c.take<uint8_t>(nr * g.max_len + 64);
            w.rB = c.take<uint8_t>(nr * w.lenW + 64);
            w.rscore = c.take<int64_t>(nr);
            w.rendA = c.take<uint32_t>(nr);
            w.rendB = c.take<uint32_t>(nr);
            w.rerr = c.take<uint32_t>(nr);
        }
    } else {
        w.slotA = c.take<uint8_t>(w.pcap * w.stride);
        w.slotB = c.take<uint8_t>(w.pcap * w.stride);
        w.sw_bytes = std::max<size_t>(polyhip_sw_workspace_bytes(sc, w.pcap, g.max_len, w.lenB, 0), 256);
        w.sw_work = c.take<uint8_t>(w.sw_bytes);
        w.tb_bytes = polyhip_sw_traceback_workspace_bytes(sc, std::min(w.pcap, MAP_TB_PAIRS), g.max_len, w.lenB);
        w.tb_work = c.take<uint8_t>(w.tb_bytes);
    }
    w.soff = c.take<uint64_t>(nr + 1);
    w.best = c.take<uint32_t>(nr);
    if (g.k) {
        w.width = c.take<uint32_t>(slots);
        w.crid = c.take<uint32_t>(w.pcap);
    }
    if (out)
        *out = w;
    return c.used;
}

// reads per chunk that `bytes` hold: every read when they all fit, else a multiple of MAP_CHUNK (0: not even one)
uint64_t map_chunk_reads(const polyhip_scoring *sc, const MapShape &g, const MapAffine *af, uint64_t nreads, size_t bytes)
{
    auto fits = [&](uint64_t nr) {
        const size_t need = map_carve(sc, g, af, nr, nullptr, nullptr);
        return need != 0 && need <= bytes;
    };
    if (fits(nreads))
        return nreads;
    uint64_t lo = 0, hi = (nreads + MAP_CHUNK - 1) / MAP_CHUNK; // chunks of lo * MAP_CHUNK fit, of hi * MAP_CHUNK do not
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        (fits(mid * MAP_CHUNK) ? lo : hi) = mid;
    }
    return lo * MAP_CHUNK;
}

const char *check_params(const polyhip_map_params *p)
{
    if (!p)
        return "null parameters";
    if (p->seed_len < 1)
        return "seed_len must be at least 1";
    if (p->seed_stride < 1)
        return "seed_stride must be at least 1";
    if (p->max_occ < 1)
        return "max_occ must be at least 1";
    if (p->max_cand < 1 || p->max_cand > MAP_MAX_CAND)
        return "max_cand must be 1..64";
    if (p->min_score < 1)
        return "min_score must be at least 1";
    return nullptr;
}

MapShape make_shape(const polyhip_map_params *p, uint64_t n, uint32_t max_len)
{
    MapShape g{};
    g.L = p->seed_len;
    g.S = p->seed_stride;
    g.max_occ = (uint32_t)std::min<uint64_t>(p->max_occ, n); // a seed has at most n occurrences: above n means no limit
    g.W = p->band;
    g.C = p->max_cand;
    g.strands = p->both_strands ? 2 : 1;
    g.ns = max_len >= g.L ? (max_len - g.L) / g.S + 1 : 0;
    g.max_len = max_len;
    g.dbits = (uint32_t)bits_for(n + max_len);
    g.kbits = g.dbits;
    g.n = n;
    return g;
}

// the shape of a call on a reference set: a biased local diagonal is at most nmax + max_len, and the field also holds
// + band, so that the cluster kernel's k0 + W stays inside it
MapShape make_shape(const polyhip_map_params *p, const RefsHandle *rf, uint32_t max_len)
{
    MapShape g = make_shape(p, as_h(rf->index)->n, max_len);
    g.k = rf->k;
    g.cbits = (uint32_t)bits_for(rf->k - 1);
    g.dbits = (uint32_t)bits_for((uint64_t)rf->nmax + max_len + p->band);
    g.kbits = g.cbits + g.dbits;
    const uint32_t left = 64 - g.kbits; // bits for read * 2 + strand
    g.rcap = left >= 33 ? 0 : left >= 1 ? 1ull << (left - 1) : 1;
    return g;
}

// a chunk of MAP_CHUNK reads can be sorted: its keys fit 64 bits
bool keys_fit(const polyhip_map_params *p, const RefsHandle *rf, uint32_t max_len)
{
    const uint64_t rcap = make_shape(p, rf, max_len).rcap;
    return rcap == 0 || rcap >= MAP_CHUNK;
}

thread_local polyhip_map_info t_info{};
thread_local polyhip_map_affine_info t_ainfo{};
thread_local polyhip_map_refs_info t_rinfo{};

int validate(const char *who, const polyhip_bwt *hp, const polyhip_scoring *sc, const polyhip_map_params *p, uint32_t max_len)
{
    if (const char *bad = check_params(p))
        return set_error(POLYHIP_ERR_INVALID, "%s: %s", who, bad);
    if (max_len > MAP_MAX_LEN)
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: max_len %u exceeds %u (the per-pair alignment kernels' limit)", who, max_len,
                         MAP_MAX_LEN);
    if (p->band > MAP_MAX_BAND)
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: band %u exceeds %u", who, p->band, MAP_MAX_BAND);
    PH_REQUIRE(hp, "%s: null index handle", who);
    PH_REQUIRE(sc, "%s: null scoring handle", who);
    PH_REQUIRE(sc->device == as_h(hp)->dev, "%s: the scoring handle lives on device %d, the index on device %d", who, sc->device,
               as_h(hp)->dev);
    return POLYHIP_OK;
}

struct MapOut {
    int64_t *score, *second;
    uint32_t *flags, *votes, *ref_start, *ref_end, *read_start, *read_end, *err;
    uint8_t *alnA, *alnB;
    uint64_t *alnOff;
    uint64_t capacity;
    uint32_t *rid = nullptr; // the refs calls'
};

// a refs call's view for its kernels (all null for one text); o_rid = the chunk's part of the per-entry contigs
RefView ref_view(const RefsHandle *rf, const MapWork &w, uint32_t *o_rid)
{
    return rf ? RefView{rf->d_start, w.crid, o_rid} : RefView{nullptr, nullptr, nullptr};
}

// what a call leaves for polyhip_map_last_info, or (af) for polyhip_map_affine_last_info
void keep_info(const polyhip_map_info &i, const MapAffine *af, uint64_t traced, uint64_t tb_cells, uint32_t tb_chunks)
{
    if (!af) {
        t_info = i;
        return;
    }
    t_ainfo = polyhip_map_affine_info{i.seeds, i.seeds_over_max_occ, i.hits, i.clusters, i.pairs_aligned, i.reads_mapped, traced, tb_cells,
                                      i.chunks, tb_chunks};
}

// Steps 1-5 for a chunk of nr reads: seeds -> hits -> clusters -> the kept candidates as a pair batch -> its scores (the
// affine score pass, or the linear aligner with every pair's strings).  *pairs_out = the candidates.
int map_candidates(const BwtHandle *h, const RefsHandle *rf, const polyhip_scoring *sc, const MapShape &g, const MapAffine *af,
                   const MapWork &w, const uint8_t *d_reads, const uint64_t *off, uint64_t nr, hipStream_t st, polyhip_map_info &info,
                   uint32_t *pairs_out)
{
    const RefView rv = ref_view(rf, w, nullptr);
    const uint64_t slots = nr * g.strands * g.ns;
    // seeds -> hits
    uint32_t nhits = 0;
    if (slots) {
        if (h->x.layout == 0)
            hipLaunchKernelGGL(map_seed_kernel<0>, dim3(grid_for(slots)), dim3(BT), 0, st, h->x, d_reads, off, slots, g, w.start, w.first,
                               w.cnt);
        else
            hipLaunchKernelGGL(map_seed_kernel<1>, dim3(grid_for(slots)), dim3(BT), 0, st, h->x, d_reads, off, slots, g, w.start, w.first,
                               w.cnt);
        PH_HIP(hipGetLastError());
        if (rf) { // the seeds' rows -> the hits kept
            hipLaunchKernelGGL(map_count_refs_kernel, dim3(grid_for(slots)), dim3(BT), 0, st, h->d_sa, w.start, slots, g, rf->d_start,
                               w.first, w.width, w.cnt);
            PH_HIP(hipGetLastError());
        }
        PH_HIP(scan_excl<uint32_t>(w.first, w.first, slots, w.scratch, st));
        PH_HIP(hipMemcpyAsync(&nhits, w.first + slots, sizeof nhits, hipMemcpyDeviceToHost, st));
        PH_HIP(hipStreamSynchronize(st));
    }
    info.hits += nhits;
    uint32_t npairs = 0;
    uint64_t *ka = w.ka, *kb = w.kb;
    uint32_t *va = w.va, *vb = w.vb;
    if (nhits) {
        if (rf)
            hipLaunchKernelGGL(map_expand_refs_kernel, dim3(grid_for(slots)), dim3(BT), 0, st, h->d_sa, w.start, w.width, w.first, slots, g,
                               rf->d_start, ka, va);
        else
            hipLaunchKernelGGL(map_expand_kernel, dim3(grid_for(slots)), dim3(BT), 0, st, h->d_sa, w.start, w.first, slots, g, ka, va);
        PH_HIP(hipGetLastError());
        if (int rc = radix_sort(ka, va, kb, vb, nhits, (int)g.kbits + bits_for(2 * nr - 1), w.hist, w.scratch, st))
            return rc;
        if (rf)
            hipLaunchKernelGGL(map_cluster_kernel<true>, dim3(grid_for(nr * 64)), dim3(BT), 0, st, ka, w.first, off, nr, g, w.pfirst,
                               w.cvotes, w.cstrand, w.clo, w.chi, rv, w.cnt);
        else
            hipLaunchKernelGGL(map_cluster_kernel<false>, dim3(grid_for(nr * 64)), dim3(BT), 0, st, ka, w.first, off, nr, g, w.pfirst,
                               w.cvotes, w.cstrand, w.clo, w.chi, rv, w.cnt);
        PH_HIP(hipGetLastError());
        PH_HIP(scan_excl<uint32_t>(w.pfirst, w.pfirst, nr, w.scratch, st));
        PH_HIP(hipMemcpyAsync(&npairs, w.pfirst + nr, sizeof npairs, hipMemcpyDeviceToHost, st));
        PH_HIP(hipStreamSynchronize(st));
    } else {
        PH_HIP(hipMemsetAsync(w.pfirst, 0, (nr + 1) * sizeof(uint32_t), st)); // no read has a candidate
    }
    info.pairs_aligned += npairs;
    if (npairs) {
        hipLaunchKernelGGL(map_pairs_kernel, dim3(grid_for(nr * g.C)), dim3(BT), 0, st, w.pfirst, off, w.clo, w.chi, nr, g.C, w.pread,
                           w.offA, w.offB);
        PH_HIP(hipGetLastError());
        PH_HIP(scan_excl<uint64_t>(w.offA, w.offA, npairs, w.scratch, st));
        PH_HIP(scan_excl<uint64_t>(w.offB, w.offB, npairs, w.scratch, st));
        hipLaunchKernelGGL(map_gather_kernel, dim3(grid_for((uint64_t)npairs * 64)), dim3(BT), 0, st, d_reads, off, h->d_text, w.pread,
                           w.pfirst, w.cstrand, w.clo, g.C, (uint64_t)npairs, w.offA, w.offB, w.A, w.B);
        PH_HIP(hipGetLastError());
        if (af) {
            if (int rc = k3a::score_pass(sc, af->c, af->go, af->ge, w.A, w.offA, npairs, w.B, w.offB, w.lenB, w.score, w.endA, w.endB,
                                         w.err, w.band, k3a::grid_blocks(af->c, npairs, w.lenB), st))
                return rc;
        } else if (int rc = polyhip_sw_align_batch_dev(sc, w.A, w.offA, npairs, g.max_len, w.B, w.offB, w.lenB, w.score, w.endA, w.endB,
                                                       w.err, w.slotA, w.slotB, w.alnLen, w.stride, w.sw_work, w.sw_bytes, w.tb_work,
                                                       w.tb_bytes, st)) {
            return rc;
        }
    }
    *pairs_out = npairs;
    return POLYHIP_OK;
}

// The call on device pointers, on the index's device (the caller has entered it).  *needed = the strings' bytes.
// af: the extension has affine gaps and only the winners are traced (polyhip_map_reads_affine).
int map_run(const BwtHandle *h, const RefsHandle *rf, const polyhip_scoring *sc, const polyhip_map_params *p, const MapAffine *af,
            const uint8_t *d_reads, const uint64_t *d_off, uint64_t nreads, uint32_t max_len, const MapOut &o, void *d_work,
            size_t work_bytes, hipStream_t st, uint64_t *needed)
{
    const char *who = rf ? "polyhip_map_reads_refs" : af ? "polyhip_map_reads_affine" : "polyhip_map_reads";
    if (rf)
        t_rinfo = polyhip_map_refs_info{rf->k, 0};
    polyhip_map_info info{};
    uint64_t traced = 0;
    uint32_t tb_chunks = 0;
    *needed = 0;
    const bool strings = o.alnA != nullptr;
    if (nreads == 0) {
        if (o.alnOff)
            PH_HIP(hipMemsetAsync(o.alnOff, 0, sizeof(uint64_t), st));
        keep_info(info, af, 0, 0, 0);
        return POLYHIP_OK;
    }
    PH_REQUIRE(d_off && o.score && o.second && o.flags && o.votes && o.ref_start && o.ref_end && o.read_start && o.read_end && o.err,
               "%s: null argument", who);
    PH_REQUIRE(!strings || (o.alnB && o.alnOff), "%s: alnA without alnB / alnOff", who);
    const MapShape g = rf ? make_shape(p, rf, max_len) : make_shape(p, h->n, max_len);
    const uint64_t per = map_chunk_reads(sc, g, af, nreads, d_work ? work_bytes : 0);
    PH_REQUIRE(per > 0, "%s: a workspace of %zu bytes does not hold a chunk of %llu reads (%zu bytes)", who, work_bytes,
               (unsigned long long)std::min<uint64_t>(nreads, MAP_CHUNK),
               map_carve(sc, g, af, std::min<uint64_t>(nreads, MAP_CHUNK), nullptr, nullptr));
    MapWork w;
    (void)map_carve(sc, g, af, per, static_cast<uint8_t *>(d_work), &w);
    uint64_t *sbase = reinterpret_cast<uint64_t *>(w.cnt + CNT_N);
    PH_HIP(hipMemsetAsync(w.cnt, 0, (CNT_N + 1) * sizeof(unsigned long long), st));
    if (af) {
        hipLaunchKernelGGL(map_diroff_kernel, dim3(grid_for(w.sub)), dim3(BT), 0, st, w.dirOff, w.sub, w.dwords);
        PH_HIP(hipGetLastError());
    }
    SyncOnExit sync(st); // counts are read back into locals
    for (uint64_t r0 = 0; r0 < nreads; r0 += per, ++info.chunks) {
        const uint64_t nr = std::min(per, nreads - r0);
        const uint64_t *off = d_off + r0;
        uint32_t npairs = 0;
        if (int rc = map_candidates(h, rf, sc, g, af, w, d_reads, off, nr, st, info, &npairs))
            return rc;
        if (af) {
            // the winner of every read from scores, errs and ranks; then the strings of the winners alone
            const auto reduce = rf ? map_reduce_kernel<true, true> : map_reduce_kernel<true, false>;
            hipLaunchKernelGGL(reduce, dim3(grid_for(nr * 64)), dim3(BT), 0, st, w.pfirst, off, nr, g, p->min_score, w.score, w.endA, w.endB,
                               w.err, w.alnLen, w.slotA, w.slotB, w.stride, w.cvotes, w.cstrand, w.clo, o.score + r0, o.second + r0,
                               o.flags + r0, o.votes + r0, o.ref_start + r0, o.ref_end + r0, o.read_start + r0, o.read_end + r0,
                               o.err + r0, w.soff, w.best, w.wfirst, ref_view(rf, w, rf ? o.rid + r0 : nullptr), w.cnt);
            PH_HIP(hipGetLastError());
            uint32_t nwin = 0;
            PH_HIP(scan_excl<uint32_t>(w.wfirst, w.wfirst, nr, w.scratch, st));
            PH_HIP(hipMemcpyAsync(&nwin, w.wfirst + nr, sizeof nwin, hipMemcpyDeviceToHost, st));
            PH_HIP(hipStreamSynchronize(st));
            traced += nwin;
            if (nwin) { // a chunk without a winner launches no traceback
                hipLaunchKernelGGL(map_winners_kernel, dim3(grid_for(nr)), dim3(BT), 0, st, w.wfirst, w.best, nr, w.offA, w.offB, w.score,
                                   w.endA, w.endB, w.wsrc, w.woffA, w.woffB, w.wscore, w.wendA, w.wendB, w.werr);
                PH_HIP(hipGetLastError());
                PH_HIP(scan_excl<uint64_t>(w.woffA, w.woffA, nwin, w.scratch, st));
                PH_HIP(scan_excl<uint64_t>(w.woffB, w.woffB, nwin, w.scratch, st));
                hipLaunchKernelGGL(map_wgather_kernel, dim3(grid_for((uint64_t)nwin * 64)), dim3(BT), 0, st, w.wsrc, (uint64_t)nwin, w.offA,
                                   w.offB, w.A, w.B, w.woffA, w.woffB, w.wA, w.wB);
                PH_HIP(hipGetLastError());
                for (uint64_t i0 = 0; i0 < nwin; i0 += w.sub, ++tb_chunks) {
                    const uint64_t m = std::min<uint64_t>(w.sub, nwin - i0);
                    if (int rc = k3a::traceback_pass(sc, af->c, af->go, af->ge, w.wA, w.woffA + i0, m, w.wB, w.woffB + i0, w.lenB,
                                                     w.wscore + i0, w.wendA + i0, w.wendB + i0, w.werr + i0, w.dirOff, w.dir, w.band,
                                                     w.lenB, k3a::grid_blocks(af->c, m, w.lenB), w.slotA + i0 * w.stride,
                                                     w.slotB + i0 * w.stride, w.wlen + i0, w.stride, st))
                        return rc;
                }
                hipLaunchKernelGGL(map_finish_kernel, dim3(grid_for(nr * 64)), dim3(BT), 0, st, w.wfirst, nr, w.wlen, w.slotA, w.slotB,
                                   w.stride, w.wscore, w.wendA, w.wendB, (int)sc->smax, af->ge, o.ref_end + r0, o.read_end + r0,
                                   o.ref_start + r0, o.read_start + r0, w.soff, w.best, w.cnt);
                PH_HIP(hipGetLastError());
            }
        } else {
            hipLaunchKernelGGL(map_reduce_kernel<false>, dim3(grid_for(nr * 64)), dim3(BT), 0, st, w.pfirst, off, nr, g, p->min_score, w.score,
                               w.endA, w.endB, w.err, w.alnLen, w.slotA, w.slotB, w.stride, w.cvotes, w.cstrand, w.clo, o.score + r0,
                               o.second + r0, o.flags + r0, o.votes + r0, o.ref_start + r0, o.ref_end + r0, o.read_start + r0,
                               o.read_end + r0, o.err + r0, w.soff, w.best, (uint32_t *)nullptr, RefView{}, w.cnt);
            PH_HIP(hipGetLastError());
        }
        if (strings) {
            PH_HIP(scan_excl<uint64_t>(w.soff, w.soff, nr, w.scratch, st));
            hipLaunchKernelGGL(map_strings_kernel, dim3(grid_for(nr * 64)), dim3(BT), 0, st, w.soff, w.best, nr, w.slotA, w.slotB, w.stride,
                               sbase, o.alnOff + r0, o.alnA, o.alnB, o.capacity);
            PH_HIP(hipGetLastError());
            hipLaunchKernelGGL(map_advance_kernel, dim3(1), dim3(64), 0, st, sbase, w.soff + nr, o.alnOff + nreads);
            PH_HIP(hipGetLastError());
        }
    }
    unsigned long long cnt[CNT_N + 1];
    PH_HIP(hipMemcpyAsync(cnt, w.cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    info.seeds = cnt[CNT_SEEDS];
    info.seeds_over_max_occ = cnt[CNT_OVER];
    info.clusters = cnt[CNT_CLUSTERS];
    info.reads_mapped = cnt[CNT_MAPPED];
    keep_info(info, af, traced, cnt[CNT_TBCELLS], tb_chunks);
    if (rf)
        t_rinfo.straddling = cnt[CNT_STRADDLE];
    *needed = cnt[CNT_N];
    if (strings && *needed > o.capacity)
        return set_error(POLYHIP_ERR_INVALID, "%s: the aligned strings need %llu bytes, the buffers hold %llu", who,
                         (unsigned long long)*needed, (unsigned long long)o.capacity);
    return POLYHIP_OK;
}

// the whole-batch workspace, capped: what map_run cuts its chunks from
size_t map_workspace(const polyhip_scoring *sc, const MapShape &g, const MapAffine *af, uint64_t nreads)
{
    if (nreads == 0)
        return 0;
    const uint64_t padded = nreads <= MAP_CHUNK ? nreads : (nreads + MAP_CHUNK - 1) / MAP_CHUNK * MAP_CHUNK;
    const size_t all = map_carve(sc, g, af, padded, nullptr, nullptr);
    if (all != 0 && all <= MAP_WORK_CAP)
        return all;
    const uint64_t per = std::max<uint64_t>(map_chunk_reads(sc, g, af, padded, MAP_WORK_CAP), MAP_CHUNK);
    return map_carve(sc, g, af, per, nullptr, nullptr);
}

// The host-pointer calls: polyhip_map_reads (gaps == nullptr) and polyhip_map_reads_affine (gaps = {open, extend}).
// work_limit: the most workspace the call may use (0: the whole batch, capped).
// rf: the call is polyhip_map_reads_refs (hp is then the set's index, NULL for a NULL set) and rid is its extra output.
int map_host(const char *who, const polyhip_bwt *hp, const RefsHandle *rf, const polyhip_scoring *sc, const polyhip_map_params *p,
             const int64_t *gaps, uint64_t work_limit, const uint8_t *reads, const uint64_t *off, uint64_t nreads, uint32_t max_len,
             int64_t *score, int64_t *second, uint32_t *flags, uint32_t *votes, uint32_t *rid, uint32_t *ref_start, uint32_t *ref_end,
             uint32_t *read_start, uint32_t *read_end, uint32_t *err, uint8_t *alnA, uint8_t *alnB, uint64_t *alnOff,
             uint64_t aln_capacity)
{
    if (int rc = validate(who, hp, sc, p, max_len))
        return rc;
    const bool strings = alnA != nullptr;
    uint64_t nbytes = 0;
    if (nreads) {
        PH_REQUIRE(off && score && second && flags && votes && ref_start && ref_end && read_start && read_end && err && (rid || !rf),
                   "%s: null argument", who);
        PH_REQUIRE(!strings || (alnB && alnOff), "%s: alnA without alnB / alnOff", who);
        for (uint64_t i = 0; i < nreads; ++i)
            PH_REQUIRE(off[i] <= off[i + 1], "%s: offsets are not ascending at %llu", who, (unsigned long long)i);
        nbytes = off[nreads] - off[0];
        PH_REQUIRE(reads || nbytes == 0, "%s: null read buffer", who);
    }
    MapAffine aff{};
    const MapAffine *af = nullptr;
    if (gaps) {
        const int64_t go = gaps[0], ge = gaps[1];
        if (!(go <= ge && ge <= -1))
            return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: gap_open %lld, gap_extend %lld: need gap_open <= gap_extend <= -1", who,
                             (long long)go, (long long)ge);
        // the affine kernel's int32 cells at the mapper's largest window
        const int64_t absmax = std::max<int64_t>(std::max<int64_t>(std::llabs((long long)sc->smin), std::llabs((long long)sc->smax)), -go);
        const int64_t span = (int64_t)max_len + ((int64_t)max_len + 3 * (int64_t)p->band), range = 1ll << 30;
        if (absmax >= range || absmax * span >= range)
            return set_error(POLYHIP_ERR_UNSUPPORTED,
                             "%s: scores could leave the int32 cells (|s|max %lld, max_len %u, band %u: |s|max * (2 * max_len + 3 * band) "
                             "must stay below 2^30)",
                             who, (long long)absmax, max_len, p->band);
        aff.go = (int)go;
        aff.ge = (int)ge;
        af = &aff;
    }
    if (rf && !keys_fit(p, rf, max_len))
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %u contigs, the longest of %u bytes: the sort keys of 256 reads do not fit 64 bits",
                         who, rf->k, rf->nmax);
    if (nreads == 0) {
        if (alnOff)
            alnOff[0] = 0;
        keep_info(polyhip_map_info{}, af, 0, 0, 0);
        if (rf)
            t_rinfo = polyhip_map_refs_info{rf->k, 0};
        return POLYHIP_OK;
    }
    const BwtHandle *h = as_h(hp);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    hipStream_t st = h->stream;
    if (af) {
        int cus = 0;
        PH_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->dev));
        aff.c = k3a::choose(sc, cus);
    }
    size_t wb = map_workspace(sc, rf ? make_shape(p, rf, max_len) : make_shape(p, h->n, max_len), af, nreads);
    if (work_limit && work_limit < wb)
        wb = work_limit;
    // outputs in one block: two int64 and seven uint32 per read (eight with rid), then the string offsets
    DevBuf dreads, doff, dout, dA, dB, dwork;
    PH_HIP(dreads.alloc(nbytes + 64));
    PH_HIP(doff.alloc((nreads + 1) * sizeof(uint64_t)));
    PH_HIP(dout.alloc(nreads * (2 * 8 + (rf ? 8 : 7) * 4) + (nreads + 1) * 8));
    if (strings) {
        PH_HIP(dA.alloc(aln_capacity));
        PH_HIP(dB.alloc(aln_capacity));
    }
    PH_HIP(dwork.alloc(wb));
    std::vector<uint64_t> rebased(nreads + 1);
    for (uint64_t i = 0; i <= nreads; ++i)
        rebased[i] = off[i] - off[0];
    SyncOnExit sync(st);
    if (nbytes)
        PH_HIP(hipMemcpyAsync(dreads.p, reads + off[0], nbytes, hipMemcpyHostToDevice, st));
    PH_HIP(hipMemcpyAsync(doff.p, rebased.data(), (nreads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    int64_t *d64 = dout.as<int64_t>();
    uint64_t *dao = reinterpret_cast<uint64_t *>(d64 + 2 * nreads);
    uint32_t *d32 = reinterpret_cast<uint32_t *>(dao + nreads + 1);
    const MapOut o{d64, d64 + nreads, d32, d32 + nreads, d32 + 2 * nreads, d32 + 3 * nreads, d32 + 4 * nreads, d32 + 5 * nreads,
                   d32 + 6 * nreads, strings ? dA.as<uint8_t>() : nullptr, strings ? dB.as<uint8_t>() : nullptr, strings ? dao : nullptr,
                   aln_capacity, rf ? d32 + 7 * nreads : nullptr};
    uint64_t needed = 0;
    const int rc = map_run(h, rf, sc, p, af, dreads.as<uint8_t>(), doff.as<uint64_t>(), nreads, max_len, o, dwork.p, wb, st, &needed);
    if (rc != POLYHIP_OK && !(strings && needed > aln_capacity))
        return rc;
    if (rf)
        PH_HIP(hipMemcpyAsync(rid, o.rid, nreads * 4, hipMemcpyDeviceToHost, st));
    // (a call whose only failure is the strings' capacity still delivers everything else)
    uint32_t *const h32[7] = {flags, votes, ref_start, ref_end, read_start, read_end, err};
    PH_HIP(hipMemcpyAsync(score, o.score, nreads * 8, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(second, o.second, nreads * 8, hipMemcpyDeviceToHost, st));
    for (int q = 0; q < 7; ++q)
        PH_HIP(hipMemcpyAsync(h32[q], d32 + q * nreads, nreads * 4, hipMemcpyDeviceToHost, st));
    if (strings) {
        PH_HIP(hipMemcpyAsync(alnOff, dao, (nreads + 1) * 8, hipMemcpyDeviceToHost, st));
        const uint64_t fit = std::min(needed, aln_capacity);
        if (fit) {
            PH_HIP(hipMemcpyAsync(alnA, dA.p, fit, hipMemcpyDeviceToHost, st));
            PH_HIP(hipMemcpyAsync(alnB, dB.p, fit, hipMemcpyDeviceToHost, st));
        }
    }
    PH_HIP(hipStreamSynchronize(st));
    return rc;
}

// ---- polyhip_map_pairs -----------------------------------------------------------------------------------------------------
constexpr uint32_t MAP_MAX_RESCUE = POLYHIP_MAP_MAX_RESCUE_COLS; // = MAP_MAX_LEN + 3 * MAP_MAX_BAND, the widest candidate window

thread_local polyhip_map_pairs_info t_pinfo{};

// columns of the widest rescue window of a call: max_insert - min_insert + max_len + 2 * band (0 without rescue)
uint64_t rescue_cols(const polyhip_map_params *p, const polyhip_map_pair_params *pp, uint32_t max_len)
{
    if (!pp || !pp->rescue || pp->min_insert > pp->max_insert)
        return 0;
    return (uint64_t)(pp->max_insert - pp->min_insert) + max_len + 2ull * p->band;
}

// The paired call on device pointers: d_reads / d_off hold the mates interleaved (2 * npairs reads).  A sibling of map_run's
// affine branch: the same candidate pass and the same winners' traceback, with the pair rule and the rescue pass between.
int pairs_run(const char *who, const BwtHandle *h, const RefsHandle *rf, const polyhip_scoring *sc, const polyhip_map_params *p,
              const PairShape &q, const MapAffine *af, const uint8_t *d_reads, const uint64_t *d_off, uint64_t npairs, uint32_t max_len,
              const MapOut &o, int64_t *o_tlen, void *d_work, size_t work_bytes, hipStream_t st, uint64_t *needed)
{
    if (rf)
        t_rinfo = polyhip_map_refs_info{rf->k, 0};
    polyhip_map_info info{};
    uint64_t traced = 0, attempts = 0;
    *needed = 0;
    const bool strings = o.alnA != nullptr;
    const uint64_t nreads = 2 * npairs;
    const MapShape g = rf ? make_shape(p, rf, max_len) : make_shape(p, h->n, max_len);
    const uint64_t per = map_chunk_reads(sc, g, af, nreads, d_work ? work_bytes : 0); // MAP_CHUNK reads are 128 pairs
    PH_REQUIRE(per > 0, "%s: a workspace of %zu bytes does not hold a chunk of %llu pairs (%zu bytes)", who, work_bytes,
               (unsigned long long)(std::min<uint64_t>(nreads, MAP_CHUNK) / 2),
               map_carve(sc, g, af, std::min<uint64_t>(nreads, MAP_CHUNK), nullptr, nullptr));
    MapWork w;
    (void)map_carve(sc, g, af, per, static_cast<uint8_t *>(d_work), &w);
    uint64_t *sbase = reinterpret_cast<uint64_t *>(w.cnt + CNT_N);
    PH_HIP(hipMemsetAsync(w.cnt, 0, (CNT_N + 1) * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(map_diroff_kernel, dim3(grid_for(w.sub)), dim3(BT), 0, st, w.dirOff, w.sub, w.dwords);
    PH_HIP(hipGetLastError());
    SyncOnExit sync(st); // counts are read back into locals
    for (uint64_t r0 = 0; r0 < nreads; r0 += per, ++info.chunks) {
        const uint64_t nr = std::min(per, nreads - r0), np = nr / 2;
        const uint64_t *off = d_off + r0;
        uint32_t ncand = 0;
        if (int rc = map_candidates(h, rf, sc, g, af, w, d_reads, off, nr, st, info, &ncand))
            return rc;
        const RefView rv = ref_view(rf, w, rf ? o.rid + r0 : nullptr);
        const auto reduce = rf ? pair_reduce_kernel<true> : pair_reduce_kernel<false>;
        const auto resolve = rf ? pair_resolve_kernel<true> : pair_resolve_kernel<false>;
        // the pair rule on scores, errs, ranks and projections; then the rescue windows it asks for, scored
        hipLaunchKernelGGL(reduce, dim3(grid_for(np * 64)), dim3(BT), 0, st, w.pfirst, off, np, g, q, p->min_score, w.score, w.endA,
                           w.endB, w.err, w.cstrand, w.clo, o.err + r0, w.choice, w.proper, w.ptlen, w.rfirst, w.rstrand, w.rlo, w.rhi, rv);
        PH_HIP(hipGetLastError());
        uint32_t nreq = 0;
        PH_HIP(scan_excl<uint32_t>(w.rfirst, w.rfirst, nr, w.scratch, st));
        if (q.rescue) {
            PH_HIP(hipMemcpyAsync(&nreq, w.rfirst + nr, sizeof nreq, hipMemcpyDeviceToHost, st));
            PH_HIP(hipStreamSynchronize(st));
        }
        attempts += nreq;
        if (nreq) { // a chunk without a request launches no rescue pass
            hipLaunchKernelGGL(rescue_plan_kernel, dim3(grid_for(nr)), dim3(BT), 0, st, w.rfirst, off, nr, w.rlo, w.rhi, w.rread, w.roffA,
                               w.roffB);
            PH_HIP(hipGetLastError());
            PH_HIP(scan_excl<uint64_t>(w.roffA, w.roffA, nreq, w.scratch, st));
            PH_HIP(scan_excl<uint64_t>(w.roffB, w.roffB, nreq, w.scratch, st));
            hipLaunchKernelGGL(rescue_gather_kernel, dim3(grid_for((uint64_t)nreq * 64)), dim3(BT), 0, st, d_reads, off, h->d_text, w.rread,
                               w.rstrand, w.rlo, (uint64_t)nreq, w.roffA, w.roffB, w.rA, w.rB);
            PH_HIP(hipGetLastError());
            if (int rc = k3a::score_pass(sc, af->c, af->go, af->ge, w.rA, w.roffA, nreq, w.rB, w.roffB, w.lenW, w.rscore, w.rendA, w.rendB,
                                         w.rerr, w.band, k3a::grid_blocks(af->c, nreq, w.lenW), st))
                return rc;
        }
        hipLaunchKernelGGL(resolve, dim3(grid_for(np * 64)), dim3(BT), 0, st, w.pfirst, off, np, g, q, p->min_score, w.score, w.endA,
                           w.endB, w.cvotes, w.cstrand, w.clo, w.choice, w.proper, w.ptlen, w.rfirst, w.rstrand, w.rlo, w.rscore, w.rendA,
                           w.rendB, w.rerr, o.score + r0, o.second + r0, o.flags + r0, o.votes + r0, o.ref_start + r0, o.ref_end + r0,
                           o.read_start + r0, o.read_end + r0, o_tlen + r0 / 2, w.soff, w.best, w.wfirst, rv, w.cnt);
        PH_HIP(hipGetLastError());
        uint32_t nwin = 0;
        PH_HIP(scan_excl<uint32_t>(w.wfirst, w.wfirst, nr, w.scratch, st));
        PH_HIP(hipMemcpyAsync(&nwin, w.wfirst + nr, sizeof nwin, hipMemcpyDeviceToHost, st));
        PH_HIP(hipStreamSynchronize(st));
        traced += nwin;
        if (nwin) { // a chunk without a mapped mate launches no traceback
            hipLaunchKernelGGL(pair_winners_kernel, dim3(grid_for(nr)), dim3(BT), 0, st, w.wfirst, w.best, nr, w.offA, w.offB, w.score,
                               w.endA, w.endB, w.roffA, w.roffB, w.rscore, w.rendA, w.rendB, w.wsrc, w.woffA, w.woffB, w.wscore, w.wendA,
                               w.wendB, w.werr);
            PH_HIP(hipGetLastError());
            PH_HIP(scan_excl<uint64_t>(w.woffA, w.woffA, nwin, w.scratch, st));
            PH_HIP(scan_excl<uint64_t>(w.woffB, w.woffB, nwin, w.scratch, st));
            hipLaunchKernelGGL(pair_wgather_kernel, dim3(grid_for((uint64_t)nwin * 64)), dim3(BT), 0, st, w.wsrc, (uint64_t)nwin, w.offA,
                               w.offB, w.A, w.B, w.roffA, w.roffB, w.rA, w.rB, w.woffA, w.woffB, w.wA, w.wB);
            PH_HIP(hipGetLastError());
            for (uint64_t i0 = 0; i0 < nwin; i0 += w.sub) {
                const uint64_t m = std::min<uint64_t>(w.sub, nwin - i0);
                if (int rc = k3a::traceback_pass(sc, af->c, af->go, af->ge, w.wA, w.woffA + i0, m, w.wB, w.woffB + i0, w.lenW,
                                                 w.wscore + i0, w.wendA + i0, w.wendB + i0, w.werr + i0, w.dirOff, w.dir, w.band,
                                                 w.lenW, k3a::grid_blocks(af->c, m, w.lenW), w.slotA + i0 * w.stride,
                                                 w.slotB + i0 * w.stride, w.wlen + i0, w.stride, st))
                    return rc;
            }
            hipLaunchKernelGGL(map_finish_kernel, dim3(grid_for(nr * 64)), dim3(BT), 0, st, w.wfirst, nr, w.wlen, w.slotA, w.slotB, w.stride,
                               w.wscore, w.wendA, w.wendB, (int)sc->smax, af->ge, o.ref_end + r0, o.read_end + r0, o.ref_start + r0,
                               o.read_start + r0, w.soff, w.best, w.cnt);
            PH_HIP(hipGetLastError());
        }
        if (strings) {
            PH_HIP(scan_excl<uint64_t>(w.soff, w.soff, nr, w.scratch, st));
            hipLaunchKernelGGL(map_strings_kernel, dim3(grid_for(nr * 64)), dim3(BT), 0, st, w.soff, w.best, nr, w.slotA, w.slotB, w.stride,
                               sbase, o.alnOff + r0, o.alnA, o.alnB, o.capacity);
            PH_HIP(hipGetLastError());
            hipLaunchKernelGGL(map_advance_kernel, dim3(1), dim3(64), 0, st, sbase, w.soff + nr, o.alnOff + nreads);
            PH_HIP(hipGetLastError());
        }
    }
    unsigned long long cnt[CNT_N + 1];
    PH_HIP(hipMemcpyAsync(cnt, w.cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    t_pinfo = polyhip_map_pairs_info{cnt[CNT_SEEDS], cnt[CNT_OVER], info.hits, cnt[CNT_CLUSTERS], info.pairs_aligned, cnt[CNT_MAPPED],
                                     cnt[CNT_PROPER], attempts, cnt[CNT_RESCUED], traced, info.chunks};
    if (rf)
        t_rinfo.straddling = cnt[CNT_STRADDLE];
    *needed = cnt[CNT_N];
    if (strings && *needed > o.capacity)
        return set_error(POLYHIP_ERR_INVALID, "%s: the aligned strings need %llu bytes, the buffers hold %llu", who,
                         (unsigned long long)*needed, (unsigned long long)o.capacity);
    return POLYHIP_OK;
}

// rf: the call is polyhip_map_pairs_refs (hp is then the set's index, NULL for a NULL set) and rid is its extra output.
int pairs_host(const char *who, const polyhip_bwt *hp, const RefsHandle *rf, const polyhip_scoring *sc, const polyhip_map_params *p,
               const polyhip_map_pair_params *pp, int64_t go, int64_t ge, const uint8_t *reads1, const uint64_t *off1,
               const uint8_t *reads2, const uint64_t *off2, uint64_t npairs, uint32_t max_len, uint64_t work_limit, int64_t *score,
               int64_t *second, uint32_t *flags, uint32_t *votes, uint32_t *rid, uint32_t *ref_start, uint32_t *ref_end,
               uint32_t *read_start, uint32_t *read_end, uint32_t *err, int64_t *tlen, uint8_t *alnA, uint8_t *alnB, uint64_t *alnOff,
               uint64_t aln_capacity)
{
    if (int rc = validate(who, hp, sc, p, max_len))
        return rc;
    const bool strings = alnA != nullptr;
    uint64_t nb1 = 0, nb2 = 0;
    if (npairs) {
        PH_REQUIRE(off1 && off2 && score && second && flags && votes && ref_start && ref_end && read_start && read_end && err && tlen &&
                       (rid || !rf),
                   "%s: null argument", who);
        PH_REQUIRE(!strings || (alnB && alnOff), "%s: alnA without alnB / alnOff", who);
        for (uint64_t i = 0; i < npairs; ++i)
            PH_REQUIRE(off1[i] <= off1[i + 1] && off2[i] <= off2[i + 1], "%s: offsets are not ascending at %llu", who,
                       (unsigned long long)i);
        nb1 = off1[npairs] - off1[0];
        nb2 = off2[npairs] - off2[0];
        PH_REQUIRE((reads1 || nb1 == 0) && (reads2 || nb2 == 0), "%s: null read buffer", who);
    }
    if (!(go <= ge && ge <= -1))
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: gap_open %lld, gap_extend %lld: need gap_open <= gap_extend <= -1", who,
                         (long long)go, (long long)ge);
    // the affine kernel's int32 cells at the wider of the mapping window and the rescue window
    const uint64_t wide = rescue_cols(p, pp, max_len);
    const int64_t absmax = std::max<int64_t>(std::max<int64_t>(std::llabs((long long)sc->smin), std::llabs((long long)sc->smax)), -go);
    const int64_t cols = std::max<int64_t>((int64_t)max_len + 3 * (int64_t)p->band, (int64_t)wide);
    const int64_t span = (int64_t)max_len + cols, range = 1ll << 30;
    if (absmax >= range || absmax * span >= range)
        return set_error(POLYHIP_ERR_UNSUPPORTED,
                         "%s: scores could leave the int32 cells (|s|max %lld, max_len %u, widest window %lld columns: |s|max * (max_len "
                         "+ columns) must stay below 2^30)",
                         who, (long long)absmax, max_len, (long long)cols);
    PH_REQUIRE(pp, "%s: null pair parameters", who);
    PH_REQUIRE(p->both_strands, "%s: both_strands must be set (a proper pair has one mate on each strand)", who);
    PH_REQUIRE(pp->min_insert <= pp->max_insert, "%s: min_insert %u exceeds max_insert %u", who, pp->min_insert, pp->max_insert);
    PH_REQUIRE(pp->rescue <= 1, "%s: rescue must be 0 or 1", who);
    if (wide > MAP_MAX_RESCUE)
        return set_error(POLYHIP_ERR_UNSUPPORTED,
                         "%s: a rescue window of max_insert - min_insert + max_len + 2 * band = %llu columns exceeds %u", who,
                         (unsigned long long)wide, MAP_MAX_RESCUE);
    if (rf && !keys_fit(p, rf, max_len))
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %u contigs, the longest of %u bytes: the sort keys of 256 reads do not fit 64 bits",
                         who, rf->k, rf->nmax);
    if (npairs == 0) {
        if (alnOff)
            alnOff[0] = 0;
        t_pinfo = polyhip_map_pairs_info{};
        if (rf)
            t_rinfo = polyhip_map_refs_info{rf->k, 0};
        return POLYHIP_OK;
    }
    PH_REQUIRE(npairs < (1ull << 31), "%s: %llu pairs exceed 2^31 - 1", who, (unsigned long long)npairs);
    const BwtHandle *h = as_h(hp);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    hipStream_t st = h->stream;
    MapAffine aff{};
    aff.go = (int)go;
    aff.ge = (int)ge;
    aff.pairs = true;
    aff.wide = (uint32_t)wide;
    int cus = 0;
    PH_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->dev));
    aff.c = k3a::choose(sc, cus);
    const PairShape q{(int64_t)pp->min_insert, (int64_t)pp->max_insert, pp->rescue};
    const uint64_t nreads = 2 * npairs, nbytes = nb1 + nb2;
    size_t wb = map_workspace(sc, rf ? make_shape(p, rf, max_len) : make_shape(p, h->n, max_len), &aff, nreads);
    if (work_limit && work_limit < wb)
        wb = work_limit;
    // the mates as they came, the interleaved batch, and the outputs in one block: two int64 and seven uint32 per mate, the
    // string offsets, an int64 per pair
    DevBuf din, dinoff, dreads, doff, dscan, dout, dA, dB, dwork;
    PH_HIP(din.alloc(nbytes + 64));
    PH_HIP(dinoff.alloc(2 * (npairs + 1) * sizeof(uint64_t)));
    PH_HIP(dreads.alloc(nbytes + 64));
    PH_HIP(doff.alloc((nreads + 1) * sizeof(uint64_t)));
    PH_HIP(dscan.alloc(scan_scratch_bytes<uint64_t>(nreads)));
    PH_HIP(dout.alloc(nreads * (2 * 8 + (rf ? 8 : 7) * 4) + (nreads + 1) * 8 + npairs * 8));
    if (strings) {
        PH_HIP(dA.alloc(aln_capacity));
        PH_HIP(dB.alloc(aln_capacity));
    }
    PH_HIP(dwork.alloc(wb));
    std::vector<uint64_t> rebased(2 * (npairs + 1));
    for (uint64_t i = 0; i <= npairs; ++i) {
        rebased[i] = off1[i] - off1[0];
        rebased[npairs + 1 + i] = off2[i] - off2[0];
    }
    SyncOnExit sync(st);
    uint8_t *d1 = din.as<uint8_t>(), *d2 = d1 + nb1;
    if (nb1)
        PH_HIP(hipMemcpyAsync(d1, reads1 + off1[0], nb1, hipMemcpyHostToDevice, st));
    if (nb2)
        PH_HIP(hipMemcpyAsync(d2, reads2 + off2[0], nb2, hipMemcpyHostToDevice, st));
    uint64_t *do1 = dinoff.as<uint64_t>(), *do2 = do1 + npairs + 1;
    PH_HIP(hipMemcpyAsync(do1, rebased.data(), rebased.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pair_lens_kernel, dim3(grid_for(npairs)), dim3(BT), 0, st, do1, do2, npairs, doff.as<uint64_t>());
    PH_HIP(hipGetLastError());
    PH_HIP(scan_excl<uint64_t>(doff.as<uint64_t>(), doff.as<uint64_t>(), nreads, dscan.as<uint8_t>(), st));
    hipLaunchKernelGGL(pair_interleave_kernel, dim3(grid_for(nreads * 64)), dim3(BT), 0, st, d1, do1, d2, do2, nreads, doff.as<uint64_t>(),
                       dreads.as<uint8_t>());
    PH_HIP(hipGetLastError());
    int64_t *d64 = dout.as<int64_t>();
    int64_t *dtl = d64 + 2 * nreads;
    uint64_t *dao = reinterpret_cast<uint64_t *>(dtl + npairs);
    uint32_t *d32 = reinterpret_cast<uint32_t *>(dao + nreads + 1);
    const MapOut o{d64, d64 + nreads, d32, d32 + nreads, d32 + 2 * nreads, d32 + 3 * nreads, d32 + 4 * nreads, d32 + 5 * nreads,
                   d32 + 6 * nreads, strings ? dA.as<uint8_t>() : nullptr, strings ? dB.as<uint8_t>() : nullptr, strings ? dao : nullptr,
                   aln_capacity, rf ? d32 + 7 * nreads : nullptr};
    uint64_t needed = 0;
    const int rc = pairs_run(who, h, rf, sc, p, q, &aff, dreads.as<uint8_t>(), doff.as<uint64_t>(), npairs, max_len, o, dtl, dwork.p, wb, st,
                             &needed);
    if (rc != POLYHIP_OK && !(strings && needed > aln_capacity))
        return rc;
    if (rf)
        PH_HIP(hipMemcpyAsync(rid, o.rid, nreads * 4, hipMemcpyDeviceToHost, st));
    // (a call whose only failure is the strings' capacity still delivers everything else)
    uint32_t *const h32[7] = {flags, votes, ref_start, ref_end, read_start, read_end, err};
    PH_HIP(hipMemcpyAsync(score, o.score, nreads * 8, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(second, o.second, nreads * 8, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(tlen, dtl, npairs * 8, hipMemcpyDeviceToHost, st));
    for (int k = 0; k < 7; ++k)
        PH_HIP(hipMemcpyAsync(h32[k], d32 + k * nreads, nreads * 4, hipMemcpyDeviceToHost, st));
    if (strings) {
        PH_HIP(hipMemcpyAsync(alnOff, dao, (nreads + 1) * 8, hipMemcpyDeviceToHost, st));
        const uint64_t fit = std::min(needed, aln_capacity);
        if (fit) {
            PH_HIP(hipMemcpyAsync(alnA, dA.p, fit, hipMemcpyDeviceToHost, st));
            PH_HIP(hipMemcpyAsync(alnB, dB.p, fit, hipMemcpyDeviceToHost, st));
        }
    }
    PH_HIP(hipStreamSynchronize(st));
    return rc;
}

} // namespace
} // namespace polyhip

using namespace polyhip;

extern "C" {

size_t polyhip_map_workspace_bytes(const polyhip_bwt *hp, const polyhip_scoring *sc, const polyhip_map_params *p, uint64_t nreads,
                                   uint32_t max_len)
{
    if (!hp || !sc || check_params(p) || max_len > MAP_MAX_LEN || p->band > MAP_MAX_BAND)
        return 0;
    return map_workspace(sc, make_shape(p, as_h(hp)->n, max_len), nullptr, nreads);
}

int polyhip_map_reads_dev(const polyhip_bwt *hp, const polyhip_scoring *sc, const polyhip_map_params *p, const uint8_t *d_reads,
                          const uint64_t *d_off, uint64_t nreads, uint32_t max_len, int64_t *d_score, int64_t *d_second, uint32_t *d_flags,
                          uint32_t *d_votes, uint32_t *d_ref_start, uint32_t *d_ref_end, uint32_t *d_read_start, uint32_t *d_read_end,
                          uint32_t *d_err, uint8_t *d_alnA, uint8_t *d_alnB, uint64_t *d_alnOff, uint64_t aln_capacity, void *d_work,
                          size_t work_bytes, polyhip_stream_t stream)
{
    if (int rc = validate("polyhip_map_reads_dev", hp, sc, p, max_len))
        return rc;
    const BwtHandle *h = as_h(hp);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    const MapOut o{d_score, d_second, d_flags, d_votes, d_ref_start, d_ref_end, d_read_start, d_read_end, d_err, d_alnA, d_alnB, d_alnOff,
                   aln_capacity};
    uint64_t needed = 0;
    return map_run(h, nullptr, sc, p, nullptr, d_reads, d_off, nreads, max_len, o, d_work, work_bytes, as_stream(stream), &needed);
}

int polyhip_map_reads(const polyhip_bwt *hp, const polyhip_scoring *sc, const polyhip_map_params *p, const uint8_t *reads,
                      const uint64_t *off, uint64_t nreads, uint32_t max_len, int64_t *score, int64_t *second, uint32_t *flags,
                      uint32_t *votes, uint32_t *ref_start, uint32_t *ref_end, uint32_t *read_start, uint32_t *read_end, uint32_t *err,
                      uint8_t *alnA, uint8_t *alnB, uint64_t *alnOff, uint64_t aln_capacity)
{
    return map_host("polyhip_map_reads", hp, nullptr, sc, p, nullptr, 0, reads, off, nreads, max_len, score, second, flags, votes, nullptr,
                    ref_start, ref_end, read_start, read_end, err, alnA, alnB, alnOff, aln_capacity);
}

int polyhip_map_reads_affine(const polyhip_bwt *hp, const polyhip_scoring *sc, const polyhip_map_params *p, int64_t gap_open,
                             int64_t gap_extend, const uint8_t *reads, const uint64_t *off, uint64_t nreads, uint32_t max_len,
                             uint64_t work_limit, int64_t *score, int64_t *second, uint32_t *flags, uint32_t *votes, uint32_t *ref_start,
                             uint32_t *ref_end, uint32_t *read_start, uint32_t *read_end, uint32_t *err, uint8_t *alnA, uint8_t *alnB,
                             uint64_t *alnOff, uint64_t aln_capacity)
{
    const int64_t gaps[2] = {gap_open, gap_extend};
    return map_host("polyhip_map_reads_affine", hp, nullptr, sc, p, gaps, work_limit, reads, off, nreads, max_len, score, second, flags,
                    votes, nullptr, ref_start, ref_end, read_start, read_end, err, alnA, alnB, alnOff, aln_capacity);
}

int polyhip_map_reads_refs(const polyhip_refs *rp, const polyhip_scoring *sc, const polyhip_map_params *p, int64_t gap_open,
                           int64_t gap_extend, const uint8_t *reads, const uint64_t *off, uint64_t nreads, uint32_t max_len,
                           uint64_t work_limit, int64_t *score, int64_t *second, uint32_t *flags, uint32_t *votes, uint32_t *rid,
                           uint32_t *ref_start, uint32_t *ref_end, uint32_t *read_start, uint32_t *read_end, uint32_t *err, uint8_t *alnA,
                           uint8_t *alnB, uint64_t *alnOff, uint64_t aln_capacity)
{
    const int64_t gaps[2] = {gap_open, gap_extend};
    const RefsHandle *rf = as_refs(rp);
    return map_host("polyhip_map_reads_refs", rf ? rf->index : nullptr, rf, sc, p, gaps, work_limit, reads, off, nreads, max_len, score,
                    second, flags, votes, rid, ref_start, ref_end, read_start, read_end, err, alnA, alnB, alnOff, aln_capacity);
}

int polyhip_map_pairs_refs(const polyhip_refs *rp, const polyhip_scoring *sc, const polyhip_map_params *p,
                           const polyhip_map_pair_params *pp, int64_t gap_open, int64_t gap_extend, const uint8_t *reads1,
                           const uint64_t *off1, const uint8_t *reads2, const uint64_t *off2, uint64_t npairs, uint32_t max_len,
                           uint64_t work_limit, int64_t *score, int64_t *second, uint32_t *flags, uint32_t *votes, uint32_t *rid,
                           uint32_t *ref_start, uint32_t *ref_end, uint32_t *read_start, uint32_t *read_end, uint32_t *err, int64_t *tlen,
                           uint8_t *alnA, uint8_t *alnB, uint64_t *alnOff, uint64_t aln_capacity)
{
    const RefsHandle *rf = as_refs(rp);
    return pairs_host("polyhip_map_pairs_refs", rf ? rf->index : nullptr, rf, sc, p, pp, gap_open, gap_extend, reads1, off1, reads2, off2,
                      npairs, max_len, work_limit, score, second, flags, votes, rid, ref_start, ref_end, read_start, read_end, err, tlen,
                      alnA, alnB, alnOff, aln_capacity);
}

int polyhip_map_refs_last_info(polyhip_map_refs_info *info)
{
    PH_REQUIRE(info, "polyhip_map_refs_last_info: null argument");
    *info = t_rinfo;
    return POLYHIP_OK;
}

int polyhip_map_pairs(const polyhip_bwt *hp, const polyhip_scoring *sc, const polyhip_map_params *p, const polyhip_map_pair_params *pp,
                      int64_t gap_open, int64_t gap_extend, const uint8_t *reads1, const uint64_t *off1, const uint8_t *reads2,
                      const uint64_t *off2, uint64_t npairs, uint32_t max_len, uint64_t work_limit, int64_t *score, int64_t *second,
                      uint32_t *flags, uint32_t *votes, uint32_t *ref_start, uint32_t *ref_end, uint32_t *read_start, uint32_t *read_end,
                      uint32_t *err, int64_t *tlen, uint8_t *alnA, uint8_t *alnB, uint64_t *alnOff, uint64_t aln_capacity)
{
    return pairs_host("polyhip_map_pairs", hp, nullptr, sc, p, pp, gap_open, gap_extend, reads1, off1, reads2, off2, npairs, max_len,
                      work_limit, score, second, flags, votes, nullptr, ref_start, ref_end, read_start, read_end, err, tlen, alnA, alnB,
                      alnOff, aln_capacity);
}

int polyhip_map_pairs_last_info(polyhip_map_pairs_info *info)
{
    PH_REQUIRE(info, "polyhip_map_pairs_last_info: null argument");
    *info = t_pinfo;
    return POLYHIP_OK;
}

int polyhip_map_affine_last_info(polyhip_map_affine_info *info)
{
    PH_REQUIRE(info, "polyhip_map_affine_last_info: null argument");
    *info = t_ainfo;
    return POLYHIP_OK;
}

int polyhip_map_last_info(polyhip_map_info *info)
{
    PH_REQUIRE(info, "polyhip_map_last_info: null argument");
    *info = t_info;
    return POLYHIP_OK;
}

} // extern "C"
