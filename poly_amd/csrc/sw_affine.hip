// sw_affine.hip -- batched Smith-Waterman with affine gaps (Gotoh) for gfx950: score pass, end cell and aligned strings.
//
// The definition (include/polyhip.h, above polyhip_sw_affine_batch):
//   E[i][j] = max(H[i][j-1] + go, E[i][j-1] + ge)      gap in A
//   F[i][j] = max(H[i-1][j] + go, F[i-1][j] + ge)      gap in B
//   H[i][j] = max(0, H[i-1][j-1] + S(a_i, b_j), F[i][j], E[i][j])
// argmax = first maximum in row-major order; a three-state traceback (H, F, E) that prefers diagonal, then F, then E, and
// inside a gap prefers opening over extending.
//
// One kernel template, swa_kernel<RB, LDS, SHARED, TB>, one pair per lane:
//   * A's rows go in bands of RB rows.  A lane keeps H[i][j-1] and E[i][j-1] of its RB rows in registers and sweeps the
//     columns once per band; F and the diagonal run down the column as scalars of the lane.  The band's last row (H and F
//     per column) goes through a global scratch laid out [wave][j][lane] (one 8-byte load and store per lane and column,
//     512 contiguous bytes per wave), loaded one column ahead of its use.
//   * The grid is persistent: a wave takes 64 pairs at a time until the batch is through, so the scratch is sized by the
//     waves in flight, not by the batch.  The lanes of a wave loop to the wave's most rows and columns under a mask.
//   * Cells are int32, -inf = -2^30: exact while absmax * (lenA + lenB) < 2^30.
//   * LDS: scores come from the compact table [ncodes + 1][ncodesB + 1] in LDS (table_fits), else from the 256 x 256
//     table in global memory.  The code tables of both alphabets are in LDS either way.
//   * SHARED (score pass, one B for all pairs): 64 column codes are loaded by the wave at once and the column's code is
//     read from its lane (v_readlane) once per wave.
//   * TB = false: the score pass.  Every row keeps its own running maximum and first column (strict >), and the rows
//     are folded in order after the band, which is the row-major-first maximum.
//   * TB = true: the traceback.  The same sweep over the pair's window (rows 1..endA, the last min(endB, W_p) columns up
//     to endB, zero boundary on the left) writes 4 direction bits per cell -- 2 bits for H's source (stop, diagonal,
//     F, E), 1 bit "F opened from H", 1 bit "E opened from H" --, eight rows to a word, [band][column][RB / 8 words] in
//     the pair's own run of the direction workspace.  The lane then walks its three states back from (endA, endB) and
//     writes the strings right-aligned into the pair's slots; the packing is the linear traceback's (k3t::pack_slots).
//
// choose() is the one place that reads the testing aid (POLYHIP_SWA_CHUNK_PAIRS) and fixes the forms that run.  The read
// mapper (map_reads.hip) drives score_pass and traceback_pass on its own device arrays through sw_affine.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "host_pipeline.h"

#include "sw_affine.h"
#include "sw_scoring.h"

namespace polyhip {
namespace k3a {

constexpr int THREADS = 256;
constexpr int RB = 32;            // rows per band (what the compiler makes of it)
constexpr int NEG = -(1 << 30);   // -inf of E and F
constexpr int64_t RANGE = 1ll << 30;

// words of direction bits of a pair's window, a multiple of 4 (the kernel stores a band's column as one uint4)
uint64_t dir_words(uint32_t eA, uint32_t ncol)
{
    return (uint64_t)((eA + RB - 1) / RB) * ncol * (RB / 8);
}

struct KArgs {
    const uint8_t *A;
    const uint64_t *offA;
    uint64_t npairs;
    const uint8_t *B;
    const uint64_t *offB; // null: one shared B of lenB bytes
    uint32_t lenB;
    const uint8_t *codeA, *codeB;
    const int32_t *table; // LDS: the compact table [na][nb]; else the 256 x 256 one
    int na, nb;
    int go, ge, smax;
    int2 *band; // [wave][band_cols][64 lanes]: (H, F) of the band's last row
    uint32_t band_cols;
    int64_t *score;
    uint32_t *endA, *endB, *err;
    // the traceback's
    const uint64_t *dirOff; // per pair: where its direction words start
    uint32_t *dir;
    uint8_t *alnA, *alnB;
    uint32_t *alnLen;
    uint32_t stride;
};

template <int RBT, bool LDS, bool SHARED, bool TB>
__global__ __launch_bounds__(THREADS, 2) void swa_kernel(const KArgs k)
{
    static_assert(RBT % 8 == 0 && (RBT & (RBT - 1)) == 0, "RB");
    static_assert(!(SHARED && TB), "the traceback reads every pair's own window of B");
    constexpr int WPB = RBT / 8; // direction words per band and column
    extern __shared__ __attribute__((aligned(16))) int32_t smem[]; // [na][nb] (LDS only), then codeA[256], codeB[256]
    const int tid = threadIdx.x, lane = tid & 63;
    const int tcells = LDS ? k.na * k.nb : 0;
    uint8_t *cA = reinterpret_cast<uint8_t *>(smem + tcells);
    uint8_t *cB = cA + 256;
    if (LDS)
        for (int t = tid; t < tcells; t += THREADS)
            smem[t] = k.table[t];
    cA[tid] = k.codeA[tid];
    cB[tid] = k.codeB[tid];
    __syncthreads();
    const int32_t *tbl = LDS ? smem : k.table;
    const uint32_t pad_row = LDS ? (uint32_t)((k.na - 1) * k.nb) : 0u; // a row of zeros for the rows beyond the pair's
    const int go = k.go, ge = k.ge;

    const uint32_t wslot = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (THREADS / 64) + (tid >> 6))), nwaves = gridDim.x * (THREADS / 64);
    int2 *ws = k.band + (size_t)wslot * k.band_cols * 64 + lane;

    // the shared B's first byte outside SecondAlphabet, once per wave
    uint32_t bbad = 0xFFFFFFFFu;
    if (SHARED) {
        for (uint32_t c = lane; c < k.lenB; c += 64)
            if (cB[k.B[c]] == 0xFFu) {
                bbad = c;
                break;
            }
        for (int d = 32; d >= 1; d >>= 1)
            bbad = min(bbad, (uint32_t)__shfl_xor((int)bbad, d, 64));
    }

    for (uint64_t base = (uint64_t)wslot * 64; base < k.npairs; base += (uint64_t)nwaves * 64) {
        const uint64_t pair = base + lane;
        const bool active = pair < k.npairs;
        const uint8_t *a = k.A, *b = k.B;
        uint32_t m = 0, n = 0;
        if (active) {
            const uint64_t o0 = k.offA[pair];
            m = (uint32_t)(k.offA[pair + 1] - o0);
            a = k.A + o0;
            if (k.offB) {
                const uint64_t p0 = k.offB[pair];
                n = (uint32_t)(k.offB[pair + 1] - p0);
                b = k.B + p0;
            } else {
                n = k.lenB;
            }
        }
        uint32_t rows = 0, ncol = 0, c_s = 1; // rows and columns of this lane's DP; its first column (1-based)
        uint32_t e = 0, eA = 0, eB = 0;
        if (!TB) {
            // the first failing Score() in row-major order: a[0], then the first invalid b[j], then the first invalid a[i]
            if (m > 0 && n > 0) {
                if (cA[a[0]] == 0xFFu) {
                    e = (1u << 8) | a[0];
                } else {
                    if (SHARED) {
                        if (bbad != 0xFFFFFFFFu)
                            e = (2u << 8) | k.B[bbad];
                    } else {
                        for (uint32_t j = 0; j < n && !e; ++j)
                            if (cB[b[j]] == 0xFFu)
                                e = (2u << 8) | b[j];
                    }
                    for (uint32_t i = 1; i < m && !e; ++i)
                        if (cA[a[i]] == 0xFFu)
                            e = (1u << 8) | a[i];
                }
                if (!e) {
                    rows = m;
                    ncol = n;
                }
            }
        } else if (active && k.err[pair] == 0u) {
            eA = k.endA[pair];
            eB = k.endB[pair];
            ncol = window_cols(eA, eB, k.score[pair], k.smax, ge);
            if (ncol > 0) {
                rows = eA;
                c_s = eB - ncol + 1u;
            }
        }
        const uint32_t rmax = dpp_wave_max(rows), cmax = dpp_wave_max(ncol);
        uint32_t *dirp = TB && rows > 0 ? k.dir + k.dirOff[pair] : nullptr;
        int best = 0;
        uint32_t bi = 0, bj = 0;

        for (uint32_t b0 = 0; b0 < rmax; b0 += RBT) {
            const bool bact = b0 < rows;          // this lane has rows in the band
            const bool first = b0 == 0;           // (uniform) the row above is row 0: H = 0, F = -inf
            const bool more = b0 + RBT < rmax;    // (uniform) a band follows: it needs this band's last row
            uint32_t ro[RBT / 2]; // the rows' offsets into the table, two per register
#pragma unroll
            for (int r2 = 0; r2 < RBT / 2; ++r2) {
                uint32_t pk = 0;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint32_t i = b0 + 2 * r2 + h;
                    uint32_t off = pad_row;
                    if (i < rows)
                        off = LDS ? (uint32_t)cA[a[i]] * (uint32_t)k.nb : (uint32_t)a[i] * 256u;
                    pk |= off << (16 * h);
                }
                ro[r2] = pk;
            }
            int Hr[RBT], Er[RBT]; // H[i][j-1], E[i][j-1]
            int rbest[TB ? 1 : RBT];
            uint32_t rj[TB ? 1 : RBT];
#pragma unroll
            for (int r = 0; r < RBT; ++r) {
                Hr[r] = 0;
                Er[r] = NEG;
                if constexpr (!TB) {
                    rbest[r] = 0;
                    rj[r] = 0;
                }
            }
            int dtop = 0; // H[b0][j-1]
            int2 up = make_int2(0, NEG);
            if (!first && bact && ncol > 0)
                up = ws[0];
            uint32_t mycode = 0; // SHARED: the code of column (c & ~63) + lane
            for (uint32_t c = 0; c < cmax; ++c) {
                const int2 cur = up;
                if (!first && bact && c + 1 < ncol)
                    up = ws[(size_t)(c + 1) * 64]; // one column ahead of its use
                uint32_t cb = 0;
                if (SHARED) {
                    if ((c & 63u) == 0u) {
                        const uint32_t cc = c + lane;
                        mycode = 0;
                        if (cc < k.lenB)
                            mycode = LDS ? (uint32_t)cB[k.B[cc]] : (uint32_t)k.B[cc];
                    }
                    cb = (uint32_t)__builtin_amdgcn_readlane((int)mycode, (int)(c & 63u));
                }
                if (bact && c < ncol) {
                    if (!SHARED) {
                        const uint32_t sym = b[c_s - 1u + c];
                        cb = LDS ? (uint32_t)cB[sym] : sym;
                    }
                    int diag = dtop, hup = cur.x, fup = cur.y;
                    dtop = cur.x;
                    uint32_t w[WPB];
#pragma unroll
                    for (int q = 0; q < WPB; ++q)
                        w[q] = 0;
                    int sv[RBT]; // the column's scores, all fetched before the chain down the column starts
#pragma unroll
                    for (int r = 0; r < RBT; ++r) {
                        const uint32_t rof = (r & 1) ? ro[r >> 1] >> 16 : ro[r >> 1] & 0xFFFFu;
                        sv[r] = tbl[rof + cb];
                    }
#pragma unroll
                    for (int r = 0; r < RBT; ++r) {
                        const int s = sv[r];
                        const int hl = Hr[r];
                        const int eo = hl + go, fo = hup + go; // the gap opened from H
                        const int ev = max(eo, Er[r] + ge);
                        const int fv = max(fo, fup + ge);
                        const int d = diag + s;
                        const int h = max(max(d, 0), max(ev, fv));
                        if constexpr (TB) {
                            const uint32_t src = h == 0 ? 0u : (h == d ? 1u : (h == fv ? 2u : 3u));
                            const uint32_t nib = src | (fv == fo ? 4u : 0u) | (ev == eo ? 8u : 0u);
                            w[r >> 3] |= nib << (4 * (r & 7));
                            // the row's bits are made here: left alone the compiler sinks the compares of all rows to the end
                            // of the column and keeps six values per row alive for them (227 registers at 16 rows)
                            asm volatile("" : "+v"(w[r >> 3]));
                        } else {
                            rj[r] = h > rbest[r] ? c + 1u : rj[r]; // strict: the row's first column with its maximum
                            rbest[r] = max(rbest[r], h);
                        }
                        diag = hl;
                        Hr[r] = h;
                        Er[r] = ev;
                        hup = h;
                        fup = fv;
                    }
                    if (more)
                        ws[(size_t)c * 64] = make_int2(hup, fup);
                    if constexpr (TB) {
                        uint32_t *dst = dirp + ((size_t)(b0 / RBT) * ncol + c) * WPB;
                        if constexpr (WPB == 4) {
                            *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
                        } else {
#pragma unroll
                            for (int q = 0; q < WPB; ++q)
                                dst[q] = w[q];
                        }
                    }
                }
            }
            if constexpr (!TB) {
#pragma unroll
                for (int r = 0; r < RBT; ++r)
                    if (b0 + r < rows && rbest[r] > best) { // rows in order, strict: row-major first
                        best = rbest[r];
                        bi = b0 + r + 1u;
                        bj = rj[r];
                    }
            }
        }

        if (!TB) {
            if (active) {
                const bool hit = e == 0u && best > 0;
                k.score[pair] = hit ? (int64_t)best : 0;
                k.endA[pair] = hit ? bi : 0u;
                k.endB[pair] = hit ? bj : 0u;
                k.err[pair] = e;
            }
        } else if (active) {
            // the three-state walk over this lane's own direction words
            uint32_t len = 0;
            if (rows > 0) {
                uint8_t *oa = k.alnA + (size_t)pair * k.stride, *ob = k.alnB + (size_t)pair * k.stride;
                uint32_t i = eA, j = eB;
                int state = 0; // 0 = H, 1 = F, 2 = E
                while (i > 0 && j >= c_s && len < k.stride) {
                    const uint32_t i1 = i - 1u;
                    const uint32_t word = dirp[((size_t)(i1 / RBT) * ncol + (j - c_s)) * WPB + ((i1 % RBT) >> 3)];
                    const uint32_t nib = (word >> (4 * (i1 & 7u))) & 15u;
                    uint8_t ca, cb2;
                    if (state == 0) {
                        const uint32_t src = nib & 3u;
                        if (src == 0u)
                            break;
                        if (src != 1u) {
                            state = src == 2u ? 1 : 2;
                            continue;
                        }
                        ca = a[i1];
                        cb2 = b[j - 1u];
                        --i;
                        --j;
                    } else if (state == 1) {
                        ca = a[i1];
                        cb2 = '-';
                        if (nib & 4u)
                            state = 0;
                        --i;
                    } else {
                        ca = '-';
                        cb2 = b[j - 1u];
                        if (nib & 8u)
                            state = 0;
                        --j;
                    }
                    oa[k.stride - 1u - len] = ca; // the strings are built by prepending: filled from the back
                    ob[k.stride - 1u - len] = cb2;
                    ++len;
                }
            }
            k.alnLen[pair] = len;
        }
    }
}

// What runs (Choice: sw_affine.h), and the only place that reads the testing aid
Choice choose(const polyhip_scoring *sc, int cus)
{
    Choice c{};
    c.rb = RB;
    c.lds = table_fits(sc);
    c.smem = c.lds ? table_smem(sc) : 512;
    // the kernels hold two workgroups per CU at their register count with a small table; a large table holds fewer and
    // the surplus workgroups simply queue
    c.max_blocks = (unsigned)std::max(cus, 1) * 2u;
    c.chunk_pairs = 1ull << 20;
    if (const char *e = getenv("POLYHIP_SWA_CHUNK_PAIRS")) { // testing aid: pairs per chunk of the traceback
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 1)
            c.chunk_pairs = v;
    }
    c.dir_cap = 1ull << 30;
    c.slot_cap = 512ull << 20;
    c.band_cap = 8ull << 30;
    return c;
}

// workgroups of a persistent grid over npairs pairs whose band scratch holds `cols` columns per wave
unsigned grid_blocks(const Choice &c, uint64_t npairs, uint64_t cols)
{
    uint64_t blocks = std::min<uint64_t>((npairs + THREADS - 1) / THREADS, c.max_blocks);
    const uint64_t per_block = std::max<uint64_t>(cols, 1) * 64 * sizeof(int2) * (THREADS / 64);
    blocks = std::min(blocks, std::max<uint64_t>(c.band_cap / per_block, 1));
    return (unsigned)std::max<uint64_t>(blocks, 1);
}
size_t band_bytes(unsigned blocks, uint64_t cols)
{
    return (size_t)blocks * (THREADS / 64) * std::max<uint64_t>(cols, 1) * 64 * sizeof(int2);
}

static void fill_args(KArgs &k, const polyhip_scoring *sc, const Choice &c, int go, int ge)
{
    k.codeA = sc->d_codeA;
    k.codeB = sc->d_codeB;
    k.table = c.lds ? sc->d_lutcc : sc->d_lut;
    k.na = sc->ncodes + 1;
    k.nb = sc->ncodesB + 1;
    k.go = go;
    k.ge = ge;
    k.smax = sc->smax;
}

// The score pass on device pointers: d_band holds band_bytes(blocks, lenB) bytes.  lenB: the shared B's length, or the
// longest B of the batch.
int score_pass(const polyhip_scoring *sc, const Choice &c, int go, int ge, const uint8_t *d_A, const uint64_t *d_offA,
               uint64_t npairs, const uint8_t *d_B, const uint64_t *d_offB, uint32_t lenB, int64_t *d_score, uint32_t *d_endA,
               uint32_t *d_endB, uint32_t *d_err, void *d_band, unsigned blocks, hipStream_t st)
{
    KArgs k{};
    fill_args(k, sc, c, go, ge);
    k.A = d_A;
    k.offA = d_offA;
    k.npairs = npairs;
    k.B = d_B;
    k.offB = d_offB;
    k.lenB = lenB;
    k.band = static_cast<int2 *>(d_band);
    k.band_cols = std::max<uint32_t>(lenB, 1);
    k.score = d_score;
    k.endA = d_endA;
    k.endB = d_endB;
    k.err = d_err;
    const bool shared = d_offB == nullptr;
    auto kern = c.lds ? (shared ? swa_kernel<RB, true, true, false> : swa_kernel<RB, true, false, false>)
                      : (shared ? swa_kernel<RB, false, true, false> : swa_kernel<RB, false, false, false>);
    PH_HIP(launch<THREADS>(kern, blocks, c.smem, st, k));
    return POLYHIP_OK;
}

// The traceback of pairs [0, npairs) (a chunk: every pointer is the chunk's own) from the score pass's outputs:
// d_dirOff[p] = where pair p's dir_words(endA, window_cols) words start in d_dir; d_band holds band_bytes(blocks,
// max_cols) bytes, max_cols = the chunk's widest window; the strings go right-aligned into stride-byte slots.
int traceback_pass(const polyhip_scoring *sc, const Choice &c, int go, int ge, const uint8_t *d_A, const uint64_t *d_offA,
                   uint64_t npairs, const uint8_t *d_B, const uint64_t *d_offB, uint32_t lenB, const int64_t *d_score,
                   const uint32_t *d_endA, const uint32_t *d_endB, const uint32_t *d_err, const uint64_t *d_dirOff,
                   uint32_t *d_dir, void *d_band, uint32_t max_cols, unsigned blocks, uint8_t *d_alnA, uint8_t *d_alnB,
                   uint32_t *d_alnLen, uint32_t stride, hipStream_t st)
{
    KArgs k{};
    fill_args(k, sc, c, go, ge);
    k.A = d_A;
    k.offA = d_offA;
    k.npairs = npairs;
    k.B = d_B;
    k.offB = d_offB;
    k.lenB = lenB;
    k.band = static_cast<int2 *>(d_band);
    k.band_cols = std::max<uint32_t>(max_cols, 1);
    k.score = const_cast<int64_t *>(d_score);
    k.endA = const_cast<uint32_t *>(d_endA);
    k.endB = const_cast<uint32_t *>(d_endB);
    k.err = const_cast<uint32_t *>(d_err);
    k.dirOff = d_dirOff;
    k.dir = d_dir;
    k.alnA = d_alnA;
    k.alnB = d_alnB;
    k.alnLen = d_alnLen;
    k.stride = stride;
    auto kern = c.lds ? swa_kernel<RB, true, false, true> : swa_kernel<RB, false, false, true>;
    PH_HIP(launch<THREADS>(kern, blocks, c.smem, st, k));
    return POLYHIP_OK;
}

static polyhip_sw_affine_info &last_info()
{
    static thread_local polyhip_sw_affine_info info{};
    return info;
}

struct TbChunk {
    uint64_t i0 = 0, m = 0, words = 0;
    uint32_t stride = 1, max_cols = 0;
};

// both entry points: the score pass, then (strings) the traceback in chunks of pairs and the packing of its strings
static int run(const char *who, const polyhip_scoring *sc, int64_t gap_open, int64_t gap_extend, const uint8_t *A,
               const uint64_t *offA, uint64_t npairs, const uint8_t *B, const uint64_t *offB, uint64_t lenB, int64_t *score,
               uint32_t *endA, uint32_t *endB, uint32_t *err, bool strings, uint8_t *alnA, uint8_t *alnB, uint64_t *alnOff,
               uint64_t aln_capacity)
{
    if (!(gap_open <= gap_extend && gap_extend <= -1))
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: gap_open %lld, gap_extend %lld: need gap_open <= gap_extend <= -1", who,
                         (long long)gap_open, (long long)gap_extend);
    PH_REQUIRE(sc, "%s: null scoring", who);
    PH_REQUIRE(!strings || alnOff, "%s: null pointer", who);
    if (strings)
        alnOff[0] = 0;
    polyhip_sw_affine_info &info = last_info();
    info = polyhip_sw_affine_info{};
    if (npairs == 0)
        return POLYHIP_OK;
    PH_REQUIRE(offA && score && endA && endB && err, "%s: null pointer", who);
    PH_REQUIRE(!strings || aln_capacity == 0 || (alnA && alnB), "%s: null pointer", who);
    PH_REQUIRE(npairs < (1ull << 32), "%s: too many pairs", who);
    // the handle's device, whatever the calling thread's current one is
    int cur = -1;
    PH_HIP(hipGetDevice(&cur));
    struct DeviceScope {
        int back;
        ~DeviceScope()
        {
            if (back >= 0)
                (void)hipSetDevice(back);
        }
    } scope{-1};
    if (cur != sc->device) {
        PH_HIP(hipSetDevice(sc->device));
        scope.back = cur;
    }
    HostStreams &hs = host_streams(); // the calling thread's own stream, never the null stream
    PH_HIP(hs.init());
    hipStream_t st = hs.s[0];
    PairStage in;
    if (int rc0 = in.load(who, A, offA, npairs, B, offB, lenB, st)) {
        (void)hipStreamSynchronize(st);
        return rc0;
    }
    const uint64_t maxA = in.maxA, maxB = in.maxB;
    const int64_t absmax = std::max<int64_t>(std::max<int64_t>(std::llabs((long long)sc->smin), std::llabs((long long)sc->smax)), -gap_open);
    if (absmax >= RANGE || (maxA + maxB) >= (uint64_t)RANGE || absmax * (int64_t)(maxA + maxB) >= RANGE) {
        (void)hipStreamSynchronize(st);
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: scores could leave the int32 cells (|s|max %lld, lengths %llu + %llu: the product must stay below 2^30)",
                         who, (long long)absmax, (unsigned long long)maxA, (unsigned long long)maxB);
    }
    const int go = (int)gap_open, ge = (int)gap_extend;
    int cus = 0;
    PH_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, sc->device));
    const Choice c = choose(sc, cus);
    info.pairs = npairs;
    info.rows_per_band = (uint64_t)c.rb;
    info.table_in_lds = c.lds ? 1 : 0;

    DevBuf dscore, dea, deb, derr, dband;
    PH_HIP(dscore.alloc(npairs * 8));
    PH_HIP(dea.alloc(npairs * 4));
    PH_HIP(deb.alloc(npairs * 4));
    PH_HIP(derr.alloc(npairs * 4));
    {
        const unsigned blocks = grid_blocks(c, npairs, maxB);
        PH_HIP(dband.alloc(band_bytes(blocks, maxB)));
        SyncOnExit sync(st);
        if (int rc = score_pass(sc, c, go, ge, in.A(), in.offA(), npairs, in.B(), in.offB(), (uint32_t)maxB, dscore.as<int64_t>(),
                                dea.as<uint32_t>(), deb.as<uint32_t>(), derr.as<uint32_t>(), dband.p, blocks, st))
            return rc;
        PH_HIP(hipMemcpyAsync(score, dscore.p, npairs * 8, hipMemcpyDeviceToHost, st));
        PH_HIP(hipMemcpyAsync(endA, dea.p, npairs * 4, hipMemcpyDeviceToHost, st));
        PH_HIP(hipMemcpyAsync(endB, deb.p, npairs * 4, hipMemcpyDeviceToHost, st));
        PH_HIP(hipMemcpyAsync(err, derr.p, npairs * 4, hipMemcpyDeviceToHost, st));
        PH_HIP(hipStreamSynchronize(st));
    }
    dband.reset();
    for (uint64_t p = 0; p < npairs; ++p)
        if (err[p] == 0u)
            info.cells += (offA[p + 1] - offA[p]) * (offB ? offB[p + 1] - offB[p] : lenB);
    if (!strings)
        return POLYHIP_OK;

    // ---- the traceback: every pair's direction words sized from its own window, chunks of pairs under the caps
    std::vector<uint64_t> dirOff(npairs);
    std::vector<TbChunk> chunks;
    {
        TbChunk ch;
        for (uint64_t p = 0; p < npairs; ++p) {
            uint32_t ncol = 0, sb = 0;
            if (err[p] == 0u) {
                ncol = window_cols(endA[p], endB[p], score[p], sc->smax, ge);
                sb = string_bound(endA[p], endB[p], score[p], sc->smax, ge);
            }
            const uint64_t w = ncol ? dir_words(endA[p], ncol) : 0;
            info.tb_cells += (uint64_t)(ncol ? endA[p] : 0) * ncol;
            const uint32_t stride = std::max(ch.stride, std::max<uint32_t>(sb, 1));
            if (ch.m > 0 && (ch.m >= c.chunk_pairs || (ch.words + w) * 4 > c.dir_cap || (ch.m + 1) * (uint64_t)stride > c.slot_cap)) {
                chunks.push_back(ch);
                ch = TbChunk{};
                ch.i0 = p;
            }
            dirOff[p] = ch.words;
            ch.words += w;
            ch.m += 1;
            ch.stride = std::max(ch.stride, std::max<uint32_t>(sb, 1));
            ch.max_cols = std::max(ch.max_cols, ncol);
        }
        chunks.push_back(ch);
    }
    info.chunks = chunks.size();
    uint64_t max_m = 0, max_words = 0, max_slot = 0, max_band = 0;
    for (const TbChunk &ch : chunks) {
        max_m = std::max(max_m, ch.m);
        max_words = std::max(max_words, ch.words);
        max_slot = std::max(max_slot, ch.m * (uint64_t)ch.stride);
        max_band = std::max<uint64_t>(max_band, band_bytes(grid_blocks(c, ch.m, ch.max_cols), ch.max_cols));
    }
    DevBuf ddirOff, ddir, dalA, dalB, dlen, dpA, dpB, doff, dbsum;
    PH_HIP(ddirOff.alloc(max_m * 8));
    PH_HIP(ddir.alloc(max_words * 4 + 16));
    PH_HIP(dband.alloc(max_band));
    PH_HIP(dalA.alloc(max_slot));
    PH_HIP(dalB.alloc(max_slot));
    PH_HIP(dlen.alloc(max_m * 4));
    PH_HIP(dpA.alloc(max_slot));
    PH_HIP(dpB.alloc(max_slot));
    PH_HIP(doff.alloc((max_m + 1) * 8));
    PH_HIP(dbsum.alloc(k3t::pack_bsum_bytes(max_m)));
    SyncOnExit sync(st);
    uint64_t base = 0;     // packed bytes of the chunks finished so far
    bool overflow = false; // the caller's string buffers are too small: the offsets are still completed
    for (const TbChunk &ch : chunks) {
        const uint64_t i0 = ch.i0, m = ch.m;
        PH_HIP(hipMemcpyAsync(ddirOff.p, dirOff.data() + i0, m * 8, hipMemcpyHostToDevice, st));
        if (int rc = traceback_pass(sc, c, go, ge, in.A(), in.offA() + i0, m, in.B(), in.offB() ? in.offB() + i0 : nullptr,
                                    (uint32_t)maxB, dscore.as<int64_t>() + i0, dea.as<uint32_t>() + i0, deb.as<uint32_t>() + i0,
                                    derr.as<uint32_t>() + i0, ddirOff.as<uint64_t>(), ddir.as<uint32_t>(), dband.p, ch.max_cols,
                                    grid_blocks(c, m, ch.max_cols), dalA.as<uint8_t>(), dalB.as<uint8_t>(), dlen.as<uint32_t>(),
                                    ch.stride, st))
            return rc;
        PH_HIP(k3t::pack_slots(st, dlen.as<uint32_t>(), m, dbsum.as<uint64_t>(), base, dalA.as<uint8_t>(), dalB.as<uint8_t>(),
                               ch.stride, doff.as<uint64_t>(), dpA.as<uint8_t>(), dpB.as<uint8_t>()));
        PH_HIP(hipMemcpyAsync(alnOff + i0, doff.p, (m + 1) * 8, hipMemcpyDeviceToHost, st));
        PH_HIP(hipStreamSynchronize(st)); // the chunk's total decides what is copied
        const uint64_t total = alnOff[i0 + m] - base;
        if (base + total > aln_capacity) {
            overflow = true;
        } else if (total) {
            PH_HIP(hipMemcpyAsync(alnA + base, dpA.p, total, hipMemcpyDeviceToHost, st));
            PH_HIP(hipMemcpyAsync(alnB + base, dpB.p, total, hipMemcpyDeviceToHost, st));
            PH_HIP(hipStreamSynchronize(st));
        }
        base += total;
    }
    if (overflow)
        return set_error(POLYHIP_ERR_INVALID,
                         "%s: the strings need %llu bytes per buffer, aln_capacity is %llu (scores, ends and alnOff are "
                         "complete: call again with buffers of alnOff[npairs] bytes)",
                         who, (unsigned long long)base, (unsigned long long)aln_capacity);
    return POLYHIP_OK;
}

} // namespace k3a
} // namespace polyhip

using namespace polyhip;

extern "C" {

int polyhip_sw_affine_batch(const polyhip_scoring *sc, int64_t gap_open, int64_t gap_extend, const uint8_t *A,
                            const uint64_t *offA, uint64_t npairs, const uint8_t *B, const uint64_t *offB, uint64_t lenB,
                            int64_t *score, uint32_t *endA, uint32_t *endB, uint32_t *err)
{
    return k3a::run("polyhip_sw_affine_batch", sc, gap_open, gap_extend, A, offA, npairs, B, offB, lenB, score, endA, endB, err,
                    false, nullptr, nullptr, nullptr, 0);
}

int polyhip_sw_affine_align_batch_packed(const polyhip_scoring *sc, int64_t gap_open, int64_t gap_extend, const uint8_t *A,
                                         const uint64_t *offA, uint64_t npairs, const uint8_t *B, const uint64_t *offB,
                                         uint64_t lenB, int64_t *score, uint32_t *endA, uint32_t *endB, uint32_t *err,
                                         uint8_t *alnA, uint8_t *alnB, uint64_t *alnOff, uint64_t aln_capacity)
{
    return k3a::run("polyhip_sw_affine_align_batch_packed", sc, gap_open, gap_extend, A, offA, npairs, B, offB, lenB, score, endA,
                    endB, err, true, alnA, alnB, alnOff, aln_capacity);
}

int polyhip_sw_affine_last_info(polyhip_sw_affine_info *info)
{
    PH_REQUIRE(info, "polyhip_sw_affine_last_info: null pointer");
    *info = k3a::last_info();
    return POLYHIP_OK;
}

} // extern "C"
