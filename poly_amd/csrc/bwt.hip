// bwt.hip -- search/bwt (search/bwt/bwt.go) on gfx950: a suffix-array FM-index built on the device, and batched
// Count / Locate / Extract / GetTransform over it.
//
// Text T = sequence + '$' (N = n + 1 bytes).  Suffixes sort with '$' lowest and every other byte by its unsigned
// value (bwt.go sortPrefixArray); '$' occurs once, at the end, so suffix order is rotation order.
//
// Build (polyhip_bwt_create[_dev]):
//   1. byte histogram -> the reference's New errors ('$' in the sequence), the alphabet (dense codes 1..sigma in
//      byte order, '$' = 0) and the layout (choose_layout: the one place that decides).
//   2. suffix array by prefix doubling: round 0 sorts every suffix by its first k symbols packed into one 64-bit
//      key (k = 64 / bits(sigma): 21 for DNA), round r by (rank[i], rank[i + h]) with h = k * 2^(r-1); each round
//      is an LSD radix sort over the key's significant bits only (device_prims.h: histogram / exclusive scan /
//      stable scatter, the style of mash_distance.hip) and a re-rank by adjacent compare + scan.  The loop stops as
//      soon as the group count reaches N, so a text whose longest repeat is R takes ceil(log2(R / k)) + 1 rounds.
//   3. L[j] = T[SA[j] - 1] ('$' for SA[j] == 0, the primary row), the C array and an occurrence structure:
//        nucleotide layout (sigma <= 4): 128-byte lines, 4 x uint32 checkpoint counts + 448 2-bit symbols, so an
//          LF step reads one line per range end; the primary row holds code 0 and is subtracted where it counts;
//        general layout (any alphabet): L as bytes (the primary row holds '$', which no query byte equals) and
//          sigma uint32 checkpoint counts per 64 rows.
// Queries run one pattern per lane (Count: backward search, a lane stops when its range is empty) or one wave
// per pattern / request (Locate, Extract: coalesced copies).
#include <cstring>

#include "bwt_index.h"
#include "device_prims.h"

namespace polyhip {
namespace {

// ---- prefix doubling ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT) void byte_hist_kernel(const uint8_t *__restrict__ t, uint64_t n, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t i = blockIdx.x * (uint64_t)BT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BT)
        atomicAdd(&cnt[t[i]], 1u);
    __syncthreads();
    if (cnt[threadIdx.x])
        atomicAdd(&hist[threadIdx.x], cnt[threadIdx.x]);
}

// round 0: key[i] = codes of T[i .. i + k) packed most significant first (past the end: 0), value i
__global__ __launch_bounds__(BT) void seed_keys_kernel(const uint8_t *__restrict__ t, uint64_t N, const uint8_t *__restrict__ code_of,
                                                       int bits, int k, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    __shared__ uint8_t code[256];
    code[threadIdx.x] = code_of[threadIdx.x];
    __syncthreads();
    for (uint64_t i = blockIdx.x * (uint64_t)BT + threadIdx.x; i < N; i += (uint64_t)gridDim.x * BT) {
        uint64_t key = 0;
        for (int j = 0; j < k; ++j) {
            const uint64_t p = i + j;
            const uint32_t c = p < N ? code[t[p]] : 0u;
            key = (key << bits) | c;
        }
        keys[i] = key;
        vals[i] = (uint32_t)i;
    }
}

// round r > 0: key[i] = rank[i] << B | rank[i + h] (past the end: 0 -- never decides an order, '$' is unique)
__global__ __launch_bounds__(BT) void pair_keys_kernel(const uint32_t *__restrict__ rank, uint64_t N, uint64_t h, int B,
                                                       uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    for (uint64_t i = blockIdx.x * (uint64_t)BT + threadIdx.x; i < N; i += (uint64_t)gridDim.x * BT) {
        const uint64_t hi = rank[i], lo = i + h < N ? rank[i + h] : 0u;
        keys[i] = (hi << B) | lo;
        vals[i] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(BT) void head_flags_kernel(const uint64_t *__restrict__ keys, uint64_t N, uint32_t *__restrict__ flag)
{
    for (uint64_t j = blockIdx.x * (uint64_t)BT + threadIdx.x; j < N; j += (uint64_t)gridDim.x * BT)
        flag[j] = (j == 0 || keys[j] != keys[j - 1]) ? 1u : 0u;
}

// rank[SA[j]] = the group index of row j (0-based): the exclusive scan of the head flags + the row's own flag - 1
__global__ __launch_bounds__(BT) void rerank_kernel(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ excl, uint64_t N,
                                                    uint32_t *__restrict__ rank)
{
    for (uint64_t j = blockIdx.x * (uint64_t)BT + threadIdx.x; j < N; j += (uint64_t)gridDim.x * BT) {
        const uint32_t head = excl[j + 1] - excl[j]; // 1 iff row j starts a group
        rank[sa[j]] = excl[j] + head - 1u;
    }
}

// ---- index from SA -----------------------------------------------------------------------------------------------------
// L[j] = T[SA[j] - 1], '$' on the primary row (SA[j] == 0); rows [N, Lpad) are '$' padding
__global__ __launch_bounds__(BT) void last_column_kernel(const uint8_t *__restrict__ t, const uint32_t *__restrict__ sa, uint64_t N,
                                                         uint64_t Lpad, uint8_t *__restrict__ L, uint32_t *__restrict__ primary)
{
    for (uint64_t j = blockIdx.x * (uint64_t)BT + threadIdx.x; j < Lpad; j += (uint64_t)gridDim.x * BT) {
        if (j >= N) {
            L[j] = NULL_CHAR;
            continue;
        }
        const uint32_t s = sa[j];
        L[j] = s ? t[s - 1] : NULL_CHAR;
        if (s == 0)
            *primary = (uint32_t)j;
    }
}

// general layout: cnt[c * nblk + blk] = rows of block blk whose L byte has code c (one wave per 64-row block;
// cnt is zeroed first, only codes that occur are written)
__global__ __launch_bounds__(BT) void gen_block_counts_kernel(const uint8_t *__restrict__ L, const uint8_t *__restrict__ dense,
                                                              uint64_t nblk, uint32_t *__restrict__ cnt)
{
    __shared__ uint8_t code[256];
    code[threadIdx.x] = dense[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (uint64_t blk = (blockIdx.x * (uint64_t)BT + threadIdx.x) / 64; blk < nblk; blk += (uint64_t)gridDim.x * (BT / 64)) {
        const uint8_t b = L[blk * GEN_ROWS + lane];
        const uint32_t c = code[b];
        const bool valid = c != 0xFFu;
        const uint64_t m = same_digit_lanes(c, valid);
        if (valid && (m & ((1ull << lane) - 1)) == 0)
            cnt[(uint64_t)c * nblk + blk] = (uint32_t)__popcll(m);
    }
}

// cp[blk * sigma + c] = occurrences of code c in rows [0, 64 * blk): a column of the symbol-major scan, rebased
// (uint32 arithmetic modulo 2^32: every true count is < N < 2^32)
__global__ __launch_bounds__(BT) void gen_checkpoints_kernel(const uint32_t *__restrict__ excl, uint64_t nblk, uint32_t sigma,
                                                             uint32_t *__restrict__ cp)
{
    const uint64_t total = nblk * sigma;
    for (uint64_t x = blockIdx.x * (uint64_t)BT + threadIdx.x; x < total; x += (uint64_t)gridDim.x * BT) {
        const uint64_t blk = x / sigma, c = x - blk * sigma;
        cp[x] = excl[c * nblk + blk] - excl[c * nblk];
    }
}

// nucleotide layout, pass 1: one thread per 128-byte line packs its 448 symbols (the primary row as code 0) and
// writes cnt[c * nlines + line] (the primary row not counted)
__global__ __launch_bounds__(BT) void nuc_pack_kernel(const uint8_t *__restrict__ L, const uint8_t *__restrict__ dense, uint64_t nlines,
                                                      uint4 *__restrict__ lines, uint32_t *__restrict__ cnt)
{
    __shared__ uint8_t code[256];
    code[threadIdx.x] = dense[threadIdx.x];
    __syncthreads();
    for (uint64_t line = blockIdx.x * (uint64_t)BT + threadIdx.x; line < nlines; line += (uint64_t)gridDim.x * BT) {
        const uint4 *src = reinterpret_cast<const uint4 *>(L + line * NUC_SYMS); // 448 = 28 x 16 bytes
        uint32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;
        uint4 *dst = lines + line * 8;
        dst[0] = make_uint4(0, 0, 0, 0); // the counts: nuc_counts_kernel, after the scan
#pragma unroll
        for (int q = 0; q < 7; ++q) { // 16 bytes of symbols = 64 symbols = 4 uint4 of L
            uint32_t part[4] = {0, 0, 0, 0};
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const uint4 v = src[4 * q + h];
                const uint32_t by[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int z = 0; z < 16; ++z) {
                    const uint32_t c = code[(by[z >> 2] >> (8 * (z & 3))) & 255u];
                    const bool real = c != 0xFFu;
                    const uint32_t c2 = real ? c : 0u;
                    n0 += real && c2 == 0;
                    n1 += c2 == 1;
                    n2 += c2 == 2;
                    n3 += c2 == 3;
                    part[h] |= c2 << (2 * z); // symbol 16h + z of this 64-symbol group: bits 2z of dword h
                }
            }
            dst[1 + q] = make_uint4(part[0], part[1], part[2], part[3]);
        }
        const uint32_t n4[4] = {n0, n1, n2, n3};
#pragma unroll
        for (int c = 0; c < 4; ++c)
            cnt[(uint64_t)c * nlines + line] = n4[c];
    }
}

__global__ __launch_bounds__(BT) void nuc_counts_kernel(const uint32_t *__restrict__ excl, uint64_t nlines, uint4 *__restrict__ lines)
{
    for (uint64_t line = blockIdx.x * (uint64_t)BT + threadIdx.x; line < nlines; line += (uint64_t)gridDim.x * BT) {
        uint32_t v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            v[c] = excl[(uint64_t)c * nlines + line] - excl[(uint64_t)c * nlines];
        lines[line * 8] = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// ---- queries -----------------------------------------------------------------------------------------------------------
// One lane per pattern.  start/end = the rows [start, end) of T's rotations that begin with the pattern, (0, 0) when
// there are none; err = 1 for an empty pattern ("Pattern can not be empty").
template <int LAYOUT>
__global__ __launch_bounds__(BT) void count_kernel(Index x, const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
                                                   uint32_t *__restrict__ out_start, uint32_t *__restrict__ out_end,
                                                   uint32_t *__restrict__ out_err)
{
    __shared__ uint8_t code[256];
    __shared__ uint32_t Cs[256];
    code[threadIdx.x] = x.dense[threadIdx.x];
    Cs[threadIdx.x] = x.C[threadIdx.x];
    __syncthreads();
    for (uint64_t p = blockIdx.x * (uint64_t)BT + threadIdx.x; p < npat; p += (uint64_t)gridDim.x * BT) {
        const uint64_t a = off[p], b = off[p + 1];
        uint32_t s = 0, e = x.N;
        for (uint64_t k = b; k > a && s < e;) {
            const uint8_t ch = pat[--k];
            if (ch == NULL_CHAR) { // C['$'] = 0, occ('$', i) = [i > primary]
                s = s > x.primary ? 1u : 0u;
                e = e > x.primary ? 1u : 0u;
                continue;
            }
            const uint32_t c = code[ch];
            if (c == 0xFFu) {
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
        if (s >= e)
            s = e = 0;
        out_start[p] = s;
        out_end[p] = e;
        out_err[p] = b > a ? 0u : 1u;
        if (b <= a)
            out_start[p] = out_end[p] = 0;
    }
}

__global__ __launch_bounds__(BT) void widths_kernel(const uint32_t *__restrict__ s, const uint32_t *__restrict__ e, uint64_t npat,
                                                    uint64_t *__restrict__ w)
{
    for (uint64_t p = blockIdx.x * (uint64_t)BT + threadIdx.x; p < npat; p += (uint64_t)gridDim.x * BT)
        w[p] = e[p] > s[p] ? (uint64_t)(e[p] - s[p]) : 0;
}

// one wave per pattern: out[first[p] + t] = SA[start + t], row order; entries at or past `capacity` are not written
__global__ __launch_bounds__(BT) void locate_kernel(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ s, const uint32_t *__restrict__ e,
                                                    const uint64_t *__restrict__ first, uint64_t npat, uint32_t *__restrict__ out, uint64_t capacity)
{
    const int lane = threadIdx.x & 63;
    for (uint64_t p = (blockIdx.x * (uint64_t)BT + threadIdx.x) / 64; p < npat; p += (uint64_t)gridDim.x * (BT / 64)) {
        const uint32_t a = s[p], b = e[p];
        const uint64_t f = first[p];
        for (uint64_t r = (uint64_t)a + lane; r < b; r += 64) {
            const uint64_t o = f + (r - a);
            if (o < capacity)
                out[o] = sa[r];
        }
    }
}

// one wave per request; err: 1 start >= end, 2 end > n, 3 start < 0 (the reference's order), 4 the request's slot
// out_off[i+1] - out_off[i] is shorter than end - start
__global__ __launch_bounds__(BT) void extract_kernel(const uint8_t *__restrict__ t, uint64_t n, const int64_t *__restrict__ rs,
                                                     const int64_t *__restrict__ re, uint64_t nreq, const uint64_t *__restrict__ out_off,
                                                     uint8_t *__restrict__ out, uint32_t *__restrict__ err)
{
    const int lane = threadIdx.x & 63;
    for (uint64_t q = (blockIdx.x * (uint64_t)BT + threadIdx.x) / 64; q < nreq; q += (uint64_t)gridDim.x * (BT / 64)) {
        const int64_t a = rs[q], b = re[q];
        uint32_t code = 0;
        if (a >= b)
            code = 1;
        else if (b > (int64_t)n)
            code = 2;
        else if (a < 0)
            code = 3;
        else if (out_off[q + 1] < out_off[q] || out_off[q + 1] - out_off[q] < (uint64_t)(b - a))
            code = 4;
        if (lane == 0)
            err[q] = code;
        if (code)
            continue;
        uint8_t *dst = out + out_off[q];
        for (int64_t i = lane; i < b - a; i += 64)
            dst[i] = t[a + i];
    }
}

__global__ __launch_bounds__(BT) void transform_kernel(const uint8_t *__restrict__ L, uint64_t N, uint8_t *__restrict__ out)
{
    for (uint64_t j = blockIdx.x * (uint64_t)BT + threadIdx.x; j < N; j += (uint64_t)gridDim.x * BT)
        out[j] = L[j];
}

// general-layout blocks / nucleotide lines cover rows [0, N] (a range end can be N)
uint64_t gen_blocks(uint64_t N) { return N / GEN_ROWS + 1; }
uint64_t nuc_lines(uint64_t N) { return N / NUC_SYMS + 1; }

// workspace of the build, carved in this order (base == nullptr: sizes only)
struct BuildWork {
    uint64_t *ka, *kb;                          // keys A, B
    uint32_t *va, *vb, *rank, *shared, *bhist;  // vals A, B; rank; the shared region (below); the byte histogram
    uint8_t *scratch;                           // of the scans over `shared`
    size_t bytes;
};

BuildWork build_carve(uint64_t n, uint8_t *base)
{
    const uint64_t N = n + 1, nb = radix_blocks(N);
    Carve c{base};
    BuildWork w{};
    w.ka = c.take<uint64_t>(N);
    w.kb = c.take<uint64_t>(N);
    w.va = c.take<uint32_t>(N);
    w.vb = c.take<uint32_t>(N);
    w.rank = c.take<uint32_t>(N);
    // head flags + their scan, the radix histogram + its scan, and later the occurrence counts + their scan share one
    // region: the largest of the three
    const uint64_t occ_items = std::max<uint64_t>(gen_blocks(N) * 255, nuc_lines(N) * 4);
    const uint64_t shared_items = std::max<uint64_t>(std::max<uint64_t>(N + 1, 256 * nb + 1), occ_items + 1);
    w.shared = c.take<uint32_t>(shared_items);
    w.bhist = c.take<uint32_t>(256);
    w.scratch = c.take<uint8_t>(scan_scratch_bytes<uint32_t>(shared_items));
    w.bytes = c.used;
    return w;
}

// The one place that chooses the occurrence layout.  POLYHIP_BWT_GENERAL=1 forces the general layout (testing aid:
// tests/test_bwt_gpu.py runs every case in both).
int choose_layout(uint32_t sigma) { return (sigma <= 4 && !env_is("POLYHIP_BWT_GENERAL", '1')) ? 0 : 1; }

// d_text (n bytes, device) -> a built handle.  Synchronises `st` (the byte histogram and one group count per round are
// read back).
int build(BwtHandle *h, const uint8_t *d_seq, uint64_t n, void *d_work, size_t work_bytes, hipStream_t st)
{
    const uint64_t N = n + 1;
    const BuildWork w = build_carve(n, static_cast<uint8_t *>(d_work));
    PH_REQUIRE(work_bytes >= w.bytes, "polyhip_bwt_create_dev: workspace of %zu bytes, %zu needed", work_bytes, w.bytes);
    uint64_t *ka = w.ka, *kb = w.kb;
    uint32_t *va = w.va, *vb = w.vb, *rank = w.rank, *shared = w.shared, *bhist = w.bhist;
    uint8_t *scratch = w.scratch;

    h->n = n;
    PH_HIP(hipMalloc(&h->d_text, N));
    PH_HIP(hipMemcpyAsync(h->d_text, d_seq, n, hipMemcpyDeviceToDevice, st));
    PH_HIP(hipMemsetAsync(h->d_text + n, NULL_CHAR, 1, st));

    // 1. alphabet, the reference's New errors, the layout
    PH_HIP(hipMemsetAsync(bhist, 0, 256 * sizeof(uint32_t), st));
    hipLaunchKernelGGL(byte_hist_kernel, dim3(grid_for(n)), dim3(BT), 0, st, h->d_text, n, bhist);
    PH_HIP(hipGetLastError());
    uint32_t hist[256];
    PH_HIP(hipMemcpyAsync(hist, bhist, sizeof hist, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    if (hist[NULL_CHAR])
        return set_error(POLYHIP_ERR_INVALID, "Provided sequence contains the nullChar $. BWT cannot be constructed");
    uint8_t dense[256], code_of[256]; // dense: 0..sigma-1 for the occurrence tables; code_of: '$' 0, bytes 1..sigma for sorting
    uint32_t C[256] = {0};
    uint32_t sigma = 0, below = 1;
    memset(dense, 0xFF, sizeof dense);
    memset(code_of, 0, sizeof code_of);
    for (int b = 0; b < 256; ++b)
        if (hist[b]) {
            dense[b] = (uint8_t)sigma;
            C[sigma] = below;
            below += hist[b];
            code_of[b] = (uint8_t)(++sigma);
        }
    h->x.layout = choose_layout(sigma);
    h->x.sigma = sigma;
    h->x.N = (uint32_t)N;
    PH_HIP(hipMalloc(&h->d_tables, 256 + 256 * sizeof(uint32_t) + 256));
    PH_HIP(hipMemcpyAsync(h->d_tables, dense, 256, hipMemcpyHostToDevice, st));
    PH_HIP(hipMemcpyAsync(h->d_tables + 256, C, sizeof C, hipMemcpyHostToDevice, st));
    PH_HIP(hipMemcpyAsync(h->d_tables + 256 + sizeof C, code_of, 256, hipMemcpyHostToDevice, st));
    h->x.dense = h->d_tables;
    h->x.C = reinterpret_cast<const uint32_t *>(h->d_tables + 256);
    const uint8_t *d_code_of = h->d_tables + 256 + sizeof C;

    // 2. suffix array: round 0 on k packed symbols, then doubling until every rank is unique
    const int cbits = bits_for(sigma);
    const int k = 64 / cbits;
    hipLaunchKernelGGL(seed_keys_kernel, dim3(grid_for(N)), dim3(BT), 0, st, h->d_text, N, d_code_of, cbits, k, ka, va);
    PH_HIP(hipGetLastError());
    const int B = bits_for(N - 1);
    uint64_t hstep = (uint64_t)k;
    int key_bits = k * cbits;
    for (int round = 0;; ++round) {
        if (int r = radix_sort(ka, va, kb, vb, N, key_bits, shared, scratch, st))
            return r;
        hipLaunchKernelGGL(head_flags_kernel, dim3(grid_for(N)), dim3(BT), 0, st, ka, N, shared);
        PH_HIP(hipGetLastError());
        PH_HIP(scan_excl<uint32_t>(shared, shared, N, scratch, st));
        uint32_t groups = 0;
        PH_HIP(hipMemcpyAsync(&groups, shared + N, sizeof groups, hipMemcpyDeviceToHost, st));
        PH_HIP(hipStreamSynchronize(st));
        h->rounds = round + 1;
        if (groups == N)
            break;
        PH_REQUIRE(round < 40, "polyhip_bwt: suffix sort did not converge (internal error)");
        hipLaunchKernelGGL(rerank_kernel, dim3(grid_for(N)), dim3(BT), 0, st, va, shared, N, rank);
        PH_HIP(hipGetLastError());
        hipLaunchKernelGGL(pair_keys_kernel, dim3(grid_for(N)), dim3(BT), 0, st, rank, N, hstep, B, ka, va);
        PH_HIP(hipGetLastError());
        hstep *= 2;
        key_bits = 2 * B;
    }
    PH_HIP(hipMalloc(&h->d_sa, N * sizeof(uint32_t)));
    PH_HIP(hipMemcpyAsync(h->d_sa, va, N * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));

    // 3. L, primary row, occurrence structure
    const uint64_t Lpad = h->x.layout == 0 ? nuc_lines(N) * NUC_SYMS : gen_blocks(N) * GEN_ROWS;
    PH_HIP(hipMalloc(&h->d_L, Lpad));
    uint32_t *d_primary = bhist;
    hipLaunchKernelGGL(last_column_kernel, dim3(grid_for(Lpad)), dim3(BT), 0, st, h->d_text, h->d_sa, N, Lpad, h->d_L, d_primary);
    PH_HIP(hipGetLastError());
    PH_HIP(hipMemcpyAsync(&h->x.primary, d_primary, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (h->x.layout == 0) {
        const uint64_t nl = nuc_lines(N);
        PH_HIP(hipMalloc(&h->d_lines, nl * 128));
        hipLaunchKernelGGL(nuc_pack_kernel, dim3(grid_for(nl)), dim3(BT), 0, st, h->d_L, h->d_tables, nl, h->d_lines, shared);
        PH_HIP(hipGetLastError());
        PH_HIP(scan_excl<uint32_t>(shared, shared, 4 * nl, scratch, st));
        hipLaunchKernelGGL(nuc_counts_kernel, dim3(grid_for(nl)), dim3(BT), 0, st, shared, nl, h->d_lines);
        PH_HIP(hipGetLastError());
        h->x.lines = h->d_lines;
    } else {
        const uint64_t nbk = gen_blocks(N);
        PH_HIP(hipMalloc(&h->d_cp, nbk * sigma * sizeof(uint32_t)));
        PH_HIP(hipMemsetAsync(shared, 0, nbk * sigma * sizeof(uint32_t), st));
        hipLaunchKernelGGL(gen_block_counts_kernel, dim3(grid_for(nbk * 64)), dim3(BT), 0, st, h->d_L, h->d_tables, nbk, shared);
        PH_HIP(hipGetLastError());
        PH_HIP(scan_excl<uint32_t>(shared, shared, nbk * sigma, scratch, st));
        hipLaunchKernelGGL(gen_checkpoints_kernel, dim3(grid_for(nbk * sigma)), dim3(BT), 0, st, shared, nbk, sigma, h->d_cp);
        PH_HIP(hipGetLastError());
        h->x.L = h->d_L;
        h->x.cp = h->d_cp;
    }
    PH_HIP(hipStreamSynchronize(st));
    return POLYHIP_OK;
}

int create_common(const uint8_t *seq, uint64_t n, bool on_device, void *d_work, size_t work_bytes, hipStream_t st_user,
                  polyhip_bwt **out)
{
    PH_REQUIRE(out, "polyhip_bwt_create: null output handle");
    *out = nullptr;
    if (n == 0)
        return set_error(POLYHIP_ERR_INVALID, "Provided sequence must not by empty. BWT cannot be constructed");
    PH_REQUIRE(seq, "polyhip_bwt_create: null sequence");
    PH_REQUIRE(n < 0xFFFFFFFFull, "polyhip_bwt_create: a sequence of %llu bytes is too long (suffix array entries are uint32: "
                                   "at most 2^32 - 2 bytes)", (unsigned long long)n);
    auto *h = new BwtHandle();
    auto fail = [&](int r) {
        delete h;
        return r;
    };
    if (hipGetDevice(&h->dev) != hipSuccess)
        return fail(set_error(POLYHIP_ERR_HIP, "polyhip_bwt_create: no usable HIP device"));
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        h->stream = nullptr;
        return fail(set_error(POLYHIP_ERR_HIP, "polyhip_bwt_create: hipStreamCreate failed"));
    }
    hipStream_t st = on_device ? st_user : h->stream;
    DevBuf seqbuf, work;
    const uint8_t *d_seq = seq;
    if (!on_device) {
        if (seqbuf.alloc(n) != hipSuccess || hipMemcpyAsync(seqbuf.p, seq, n, hipMemcpyHostToDevice, st) != hipSuccess)
            return fail(set_error(POLYHIP_ERR_HIP, "polyhip_bwt_create: upload of %llu bytes failed", (unsigned long long)n));
        d_seq = seqbuf.as<uint8_t>();
        work_bytes = build_carve(n, nullptr).bytes;
        if (work.alloc(work_bytes) != hipSuccess)
            return fail(set_error(POLYHIP_ERR_HIP, "polyhip_bwt_create: workspace of %zu bytes", work_bytes));
        d_work = work.p;
    }
    PH_REQUIRE(d_work, "polyhip_bwt_create_dev: null workspace");
    const int r = build(h, d_seq, n, d_work, work_bytes, st);
    if (r != POLYHIP_OK)
        return fail(r);
    *out = reinterpret_cast<polyhip_bwt *>(h);
    return POLYHIP_OK;
}


int count_launch(const BwtHandle *h, const uint8_t *d_pat, const uint64_t *d_off, uint64_t npat, uint32_t *d_s, uint32_t *d_e,
                 uint32_t *d_err, hipStream_t st)
{
    if (npat == 0)
        return POLYHIP_OK;
    if (h->x.layout == 0)
        hipLaunchKernelGGL(count_kernel<0>, dim3(grid_for(npat)), dim3(BT), 0, st, h->x, d_pat, d_off, npat, d_s, d_e, d_err);
    else
        hipLaunchKernelGGL(count_kernel<1>, dim3(grid_for(npat)), dim3(BT), 0, st, h->x, d_pat, d_off, npat, d_s, d_e, d_err);
    PH_HIP(hipGetLastError());
    return POLYHIP_OK;
}

// d_first[0..npat] = exclusive scan of the widths (scratch: scan_scratch_bytes<uint64_t>(npat), taken from d_first's tail)
int locate_launch(const BwtHandle *h, const uint32_t *d_s, const uint32_t *d_e, uint64_t npat, uint64_t *d_first, uint32_t *d_out,
                  uint64_t capacity, uint8_t *scratch, hipStream_t st)
{
    hipLaunchKernelGGL(widths_kernel, dim3(grid_for(npat)), dim3(BT), 0, st, d_s, d_e, npat, d_first);
    PH_HIP(hipGetLastError());
    PH_HIP(scan_excl<uint64_t>(d_first, d_first, npat, scratch, st));
    if (npat && capacity) {
        hipLaunchKernelGGL(locate_kernel, dim3(grid_for(npat * 64)), dim3(BT), 0, st, h->d_sa, d_s, d_e, d_first, npat, d_out, capacity);
        PH_HIP(hipGetLastError());
    }
    return POLYHIP_OK;
}

bool offsets_ok(const uint64_t *off, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i])
            return false;
    return true;
}

} // namespace
} // namespace polyhip

using namespace polyhip;

extern "C" {

size_t polyhip_bwt_workspace_bytes(uint64_t n) { return build_carve(n, nullptr).bytes; }

int polyhip_bwt_create(const uint8_t *seq, uint64_t n, polyhip_bwt **out)
{
    return create_common(seq, n, false, nullptr, 0, nullptr, out);
}

int polyhip_bwt_create_dev(const uint8_t *d_seq, uint64_t n, void *d_work, size_t work_bytes, polyhip_stream_t stream,
                           polyhip_bwt **out)
{
    return create_common(d_seq, n, true, d_work, work_bytes, as_stream(stream), out);
}

int polyhip_bwt_destroy(polyhip_bwt *h)
{
    if (!h)
        return POLYHIP_OK;
    BwtHandle *b = reinterpret_cast<BwtHandle *>(h);
    DeviceScope ds;
    (void)ds.enter(b->dev);
    delete b;
    return POLYHIP_OK;
}

int64_t polyhip_bwt_len(const polyhip_bwt *h)
{
    if (!h)
        return set_error(POLYHIP_ERR_INVALID, "polyhip_bwt_len: null handle");
    return (int64_t)as_h(h)->n;
}

int polyhip_bwt_layout(const polyhip_bwt *h)
{
    if (!h)
        return set_error(POLYHIP_ERR_INVALID, "polyhip_bwt_layout: null handle");
    return as_h(h)->x.layout;
}

int polyhip_bwt_rounds(const polyhip_bwt *h)
{
    if (!h)
        return set_error(POLYHIP_ERR_INVALID, "polyhip_bwt_rounds: null handle");
    return as_h(h)->rounds;
}

int polyhip_bwt_transform(const polyhip_bwt *hp, uint8_t *out)
{
    PH_REQUIRE(hp && out, "polyhip_bwt_transform: null argument");
    const BwtHandle *h = as_h(hp);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    PH_HIP(hipMemcpyAsync(out, h->d_L, h->n + 1, hipMemcpyDeviceToHost, h->stream));
    PH_HIP(hipStreamSynchronize(h->stream));
    return POLYHIP_OK;
}

int polyhip_bwt_transform_dev(const polyhip_bwt *hp, uint8_t *d_out, polyhip_stream_t stream)
{
    PH_REQUIRE(hp && d_out, "polyhip_bwt_transform_dev: null argument");
    const BwtHandle *h = as_h(hp);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    hipLaunchKernelGGL(transform_kernel, dim3(grid_for(h->n + 1)), dim3(BT), 0, as_stream(stream), h->d_L, h->n + 1, d_out);
    PH_HIP(hipGetLastError());
    return POLYHIP_OK;
}

int polyhip_bwt_suffix_array(const polyhip_bwt *hp, uint32_t *out)
{
    PH_REQUIRE(hp && out, "polyhip_bwt_suffix_array: null argument");
    const BwtHandle *h = as_h(hp);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    PH_HIP(hipMemcpyAsync(out, h->d_sa, (h->n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    PH_HIP(hipStreamSynchronize(h->stream));
    return POLYHIP_OK;
}

int polyhip_bwt_count_dev(const polyhip_bwt *hp, const uint8_t *d_pat, const uint64_t *d_off, uint64_t npat, uint32_t *d_start,
                          uint32_t *d_end, uint32_t *d_err, polyhip_stream_t stream)
{
    PH_REQUIRE(hp, "polyhip_bwt_count_dev: null handle");
    PH_REQUIRE(npat == 0 || (d_off && d_start && d_end && d_err), "polyhip_bwt_count_dev: null argument");
    const BwtHandle *h = as_h(hp);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    return count_launch(h, d_pat, d_off, npat, d_start, d_end, d_err, as_stream(stream));
}

int polyhip_bwt_count(const polyhip_bwt *hp, const uint8_t *pat, const uint64_t *off, uint64_t npat, uint32_t *start, uint32_t *end,
                      uint32_t *err)
{
    PH_REQUIRE(hp, "polyhip_bwt_count: null handle");
    if (npat == 0)
        return POLYHIP_OK;
    PH_REQUIRE(off && start && end && err && (pat || off[npat] == off[0]), "polyhip_bwt_count: null argument");
    PH_REQUIRE(offsets_ok(off, npat), "polyhip_bwt_count: offsets are not ascending");
    const BwtHandle *h = as_h(hp);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    hipStream_t st = h->stream;
    const uint64_t nbytes = off[npat];
    DevBuf dp, doff, dout;
    PH_HIP(dp.alloc(nbytes));
    PH_HIP(doff.alloc((npat + 1) * sizeof(uint64_t)));
    PH_HIP(dout.alloc(3 * npat * sizeof(uint32_t)));
    SyncOnExit sync(st);
    if (nbytes)
        PH_HIP(hipMemcpyAsync(dp.p, pat, nbytes, hipMemcpyHostToDevice, st));
    PH_HIP(hipMemcpyAsync(doff.p, off, (npat + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    uint32_t *o = dout.as<uint32_t>();
    if (int r = count_launch(h, dp.as<uint8_t>(), doff.as<uint64_t>(), npat, o, o + npat, o + 2 * npat, st))
        return r;
    PH_HIP(hipMemcpyAsync(start, o, npat * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(end, o + npat, npat * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(err, o + 2 * npat, npat * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    return POLYHIP_OK;
}

size_t polyhip_bwt_locate_workspace_bytes(uint64_t npat) { return scan_scratch_bytes<uint64_t>(npat); }

int polyhip_bwt_locate_dev(const polyhip_bwt *hp, const uint32_t *d_start, const uint32_t *d_end, uint64_t npat, uint64_t *d_first,
                           uint32_t *d_out, uint64_t capacity, void *d_work, size_t work_bytes, polyhip_stream_t stream)
{
    PH_REQUIRE(hp && d_first, "polyhip_bwt_locate_dev: null argument");
    PH_REQUIRE(npat == 0 || (d_start && d_end), "polyhip_bwt_locate_dev: null intervals");
    PH_REQUIRE(capacity == 0 || d_out, "polyhip_bwt_locate_dev: null output");
    PH_REQUIRE(work_bytes >= scan_scratch_bytes<uint64_t>(npat) && (d_work || scan_scratch_bytes<uint64_t>(npat) == 0),
               "polyhip_bwt_locate_dev: workspace of %zu bytes, %zu needed", work_bytes, scan_scratch_bytes<uint64_t>(npat));
    const BwtHandle *h = as_h(hp);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    return locate_launch(h, d_start, d_end, npat, d_first, d_out, capacity, static_cast<uint8_t *>(d_work), as_stream(stream));
}

int polyhip_bwt_locate(const polyhip_bwt *hp, const uint8_t *pat, const uint64_t *off, uint64_t npat, uint64_t *first, uint32_t *out,
                       uint64_t capacity, uint32_t *err)
{
    PH_REQUIRE(hp && first, "polyhip_bwt_locate: null argument");
    if (npat == 0) {
        first[0] = 0;
        return POLYHIP_OK;
    }
    PH_REQUIRE(off && err && (pat || off[npat] == off[0]), "polyhip_bwt_locate: null argument");
    PH_REQUIRE(capacity == 0 || out, "polyhip_bwt_locate: null output");
    PH_REQUIRE(offsets_ok(off, npat), "polyhip_bwt_locate: offsets are not ascending");
    const BwtHandle *h = as_h(hp);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    hipStream_t st = h->stream;
    const uint64_t nbytes = off[npat];
    DevBuf dp, doff, dse, dfirst, dwork, dout;
    PH_HIP(dp.alloc(nbytes));
    PH_HIP(doff.alloc((npat + 1) * sizeof(uint64_t)));
    PH_HIP(dse.alloc(3 * npat * sizeof(uint32_t)));
    PH_HIP(dfirst.alloc((npat + 1) * sizeof(uint64_t)));
    PH_HIP(dwork.alloc(scan_scratch_bytes<uint64_t>(npat)));
    SyncOnExit sync(st);
    if (nbytes)
        PH_HIP(hipMemcpyAsync(dp.p, pat, nbytes, hipMemcpyHostToDevice, st));
    PH_HIP(hipMemcpyAsync(doff.p, off, (npat + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    uint32_t *o = dse.as<uint32_t>();
    if (int r = count_launch(h, dp.as<uint8_t>(), doff.as<uint64_t>(), npat, o, o + npat, o + 2 * npat, st))
        return r;
    if (int r = locate_launch(h, o, o + npat, npat, dfirst.as<uint64_t>(), nullptr, 0, dwork.as<uint8_t>(), st))
        return r;
    PH_HIP(hipMemcpyAsync(first, dfirst.p, (npat + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(err, o + 2 * npat, npat * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    const uint64_t total = first[npat];
    if (total > capacity)
        return set_error(POLYHIP_ERR_INVALID, "polyhip_bwt_locate: the offsets need %llu entries, the buffer holds %llu",
                         (unsigned long long)total, (unsigned long long)capacity);
    if (total == 0)
        return POLYHIP_OK;
    PH_HIP(dout.alloc(total * sizeof(uint32_t)));
    hipLaunchKernelGGL(locate_kernel, dim3(grid_for(npat * 64)), dim3(BT), 0, st, h->d_sa, o, o + npat, dfirst.as<uint64_t>(), npat,
                       dout.as<uint32_t>(), total);
    PH_HIP(hipGetLastError());
    PH_HIP(hipMemcpyAsync(out, dout.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    return POLYHIP_OK;
}

int polyhip_bwt_extract_dev(const polyhip_bwt *hp, const int64_t *d_start, const int64_t *d_end, uint64_t nreq, const uint64_t *d_out_off,
                            uint8_t *d_out, uint32_t *d_err, polyhip_stream_t stream)
{
    PH_REQUIRE(hp, "polyhip_bwt_extract_dev: null handle");
    if (nreq == 0)
        return POLYHIP_OK;
    PH_REQUIRE(d_start && d_end && d_out_off && d_err, "polyhip_bwt_extract_dev: null argument");
    const BwtHandle *h = as_h(hp);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    hipLaunchKernelGGL(extract_kernel, dim3(grid_for(nreq * 64)), dim3(BT), 0, as_stream(stream), h->d_text, h->n, d_start, d_end, nreq,
                       d_out_off, d_out, d_err);
    PH_HIP(hipGetLastError());
    return POLYHIP_OK;
}

int polyhip_bwt_extract(const polyhip_bwt *hp, const int64_t *start, const int64_t *end, uint64_t nreq, const uint64_t *out_off,
                        uint8_t *out, uint32_t *err)
{
    PH_REQUIRE(hp, "polyhip_bwt_extract: null handle");
    if (nreq == 0)
        return POLYHIP_OK;
    PH_REQUIRE(start && end && out_off && err && (out || out_off[nreq] == out_off[0]), "polyhip_bwt_extract: null argument");
    PH_REQUIRE(out_off[0] == 0 && offsets_ok(out_off, nreq), "polyhip_bwt_extract: output offsets must start at 0 and ascend");
    const BwtHandle *h = as_h(hp);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    hipStream_t st = h->stream;
    const uint64_t nbytes = out_off[nreq];
    DevBuf dreq, doff, derr, dout;
    PH_HIP(dreq.alloc(2 * nreq * sizeof(int64_t)));
    PH_HIP(doff.alloc((nreq + 1) * sizeof(uint64_t)));
    PH_HIP(derr.alloc(nreq * sizeof(uint32_t)));
    PH_HIP(dout.alloc(nbytes));
    SyncOnExit sync(st);
    int64_t *dr = dreq.as<int64_t>();
    PH_HIP(hipMemcpyAsync(dr, start, nreq * sizeof(int64_t), hipMemcpyHostToDevice, st));
    PH_HIP(hipMemcpyAsync(dr + nreq, end, nreq * sizeof(int64_t), hipMemcpyHostToDevice, st));
    PH_HIP(hipMemcpyAsync(doff.p, out_off, (nreq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(extract_kernel, dim3(grid_for(nreq * 64)), dim3(BT), 0, st, h->d_text, h->n, dr, dr + nreq, nreq,
                       doff.as<uint64_t>(), dout.as<uint8_t>(), derr.as<uint32_t>());
    PH_HIP(hipGetLastError());
    if (nbytes)
        PH_HIP(hipMemcpyAsync(out, dout.p, nbytes, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(err, derr.p, nreq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    return POLYHIP_OK;
}

} // extern "C"
