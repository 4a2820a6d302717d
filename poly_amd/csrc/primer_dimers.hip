// primer_dimers.hip -- polyhip_primer_stack_dg, polyhip_primer_dimer_matrix, polyhip_primer_dimer_screen: which primers of a pool
// bind each other.  The definition is the comment above the calls in include/polyhip.h; tests/dimers_oracle.py restates it in
// plain Python.  All of it is integer work; the only atomics are a 64-bit minimum and 32-bit sums, neither of which depends on
// the order of arrival.
//
//   prepare_kernel  a lane per primer: err, and for a valid primer of L bytes the four position masks (bit k: byte k is
//                   "ACGT"[c]) as they stand (the x side) and of the reversed primer (the y side: bit k is byte L - 1 - k), and
//                   the prefix sums P of the stack energies, dg(run [i0, i1]) = P[i1] - P[i0].  A bad primer has length 0 and
//                   empty masks
//   pair_kernel     a block per (x, chunk of 1024 y), a lane per y.  x is the same in the whole block: its masks are scalars and
//                   its P sits in LDS.  The lane keeps y's four reversed masks in registers over all shifts.  At shift s the
//                   x masks move by s (scalar shifts), position k of the reversed y faces position k + s of x, the pairing mask
//                   is four ANDs of x's masks with y's complement masks, the stacks are M & M >> 1.  Every maximal run of stack
//                   bits is taken off with count-trailing-zeros (an add of the lowest bit carries through the run); the run
//                   through x's bit m - 2 is the 3' one, found with one count-leading-zeros.  Only the two smallest energies
//                   are kept here -- where they sit is found again by detail_kernel, for one pair per row.
//                   Matrix: the two energies go to their cells.  Screen: a lane keeps the best of its y in ascending order
//                   (strict <), the wave's smallest (dg, j) goes into the row's key by a 64-bit atomic minimum, the wave's
//                   counts by atomic adds
//   detail_kernel   screen, a lane per row: the key's partner once more, shifts ascending and runs ascending with a strict <,
//                   which is the definition's tie rule: shift, pos, pairs
#include "host_pipeline.h"
#include "device_prims.h"

namespace polyhip {
namespace {

constexpr uint32_t MAX_PRIMER = 64, NONE = 0xFFFFFFFFu;
constexpr int CHUNK = 1024;                   // y per block and x
constexpr int32_t MIN_STACK = -30000;         // a table entry is MIN_STACK..0: a run's energy is above -2^21
constexpr uint32_t KEY_BIAS = 0x40000000u;    // dg + KEY_BIAS is unsigned and keeps the order
constexpr uint64_t MATRIX_CELLS = 1ull << 30; // the matrix call's limit
constexpr uint64_t LAUNCH_PAIRS = 1ull << 32; // the screen cuts X into row blocks of about this many pairs

// POLYHIP_DIMER_LAUNCH_PAIRS=<n> overrides LAUNCH_PAIRS (testing aid, read per call: more than one row block at a size a test can
// check)
inline uint64_t launch_pairs()
{
    if (const char *e = getenv("POLYHIP_DIMER_LAUNCH_PAIRS")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 1 && v <= LAUNCH_PAIRS)
            return v;
    }
    return LAUNCH_PAIRS;
}

// one set of primers on the device, n of them: plane c of fwd / rev is [c * n, (c + 1) * n); P has 64 entries per primer
struct DevSide {
    const uint64_t *fwd, *rev;
    const uint32_t *len; // 0: a bad primer
    const int32_t *P;
    uint64_t n;
};

__device__ __forceinline__ uint32_t nt_code(uint32_t b)
{
    const uint32_t u = b & ~0x20u; // the letters' case bit; no other byte becomes one of ACGT by it
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

__global__ __launch_bounds__(BT) void prepare_kernel(uint64_t n, const uint8_t *__restrict__ bytes, const uint64_t *__restrict__ off,
                                                     const int32_t *__restrict__ stack, uint64_t *__restrict__ fwd,
                                                     uint64_t *__restrict__ rev, uint32_t *__restrict__ len, int32_t *__restrict__ P,
                                                     uint32_t *__restrict__ err)
{
    const uint64_t off0 = off[0];
    for (uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BT) {
        const uint64_t L64 = off[i + 1] - off[i];
        const uint32_t e = L64 == 0 ? 1u : L64 > MAX_PRIMER ? 2u : 0u;
        const uint32_t L = e ? 0u : (uint32_t)L64;
        const uint8_t *p = bytes + (off[i] - off0);
        uint64_t f0 = 0, f1 = 0, f2 = 0, f3 = 0, r0 = 0, r1 = 0, r2 = 0, r3 = 0;
        int32_t sum = 0;
        uint32_t prev = 4;
        int32_t *Pi = P + i * 64;
        for (uint32_t k = 0; k < 64; ++k) {
            uint32_t c = 4;
            if (k < L) {
                c = nt_code(p[k]);
                const uint64_t fb = 1ull << k, rb = 1ull << (L - 1 - k);
                f0 |= c == 0 ? fb : 0ull, f1 |= c == 1 ? fb : 0ull, f2 |= c == 2 ? fb : 0ull, f3 |= c == 3 ? fb : 0ull;
                r0 |= c == 0 ? rb : 0ull, r1 |= c == 1 ? rb : 0ull, r2 |= c == 2 ? rb : 0ull, r3 |= c == 3 ? rb : 0ull;
                if (prev < 4 && c < 4)
                    sum += stack[4 * prev + c];
            }
            Pi[k] = k < L ? sum : 0; // P[k]: the stacks left of position k
            prev = c;
        }
        fwd[i] = f0, fwd[n + i] = f1, fwd[2 * n + i] = f2, fwd[3 * n + i] = f3;
        rev[i] = r0, rev[n + i] = r1, rev[2 * n + i] = r2, rev[3 * n + i] = r3;
        len[i] = L;
        err[i] = e;
    }
}

__device__ __forceinline__ uint64_t moved(uint64_t x, int s) { return s >= 0 ? x >> s : x << -s; }

// the smallest energy of a run, and of a run that holds x's 3' base, over every shift at which a y of up to nmax bytes meets x;
// 0 where there is none.  x0..x3, m, nmax and Ps (x's P, 64 entries in LDS) are the same in every lane
__device__ __forceinline__ void pair_energies(uint64_t x0, uint64_t x1, uint64_t x2, uint64_t x3, int m, const int32_t *Ps, uint64_t y0,
                                              uint64_t y1, uint64_t y2, uint64_t y3, int nmax, int &any, int &end)
{
    any = 0;
    end = 0;
    const int p_last = Ps[(m - 1) & 63];
    for (int s = 1 - nmax; s < m; ++s) {
        const uint64_t M = (moved(x0, s) & y3) | (moved(x1, s) & y2) | (moved(x2, s) & y1) | (moved(x3, s) & y0);
        uint64_t S = M & (M >> 1); // bit k: k and k + 1 are both paired; bit 63 is never set
        const int e = m - 2 - s;   // where x's last stack sits
        if (e >= 0 && e <= 62) {
            const int run = __clzll((long long)~(S << (63 - e))); // the stack bits from e downwards; the low bits of the moved S are 0
            end = min(end, p_last - Ps[(m - 1 - run) & 63]);
        }
        while (S) {
            const uint64_t up = S + (S & (0 - S)); // clears the lowest run and sets the bit above it
            const int k0 = __ffsll((unsigned long long)S) - 1, k1 = __ffsll((unsigned long long)up) - 1;
            any = min(any, Ps[(k1 + s) & 63] - Ps[(k0 + s) & 63]);
            S &= up;
        }
    }
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) { return ~dpp_wave_max(~v); }

// rows [row0, row0 + rows) of X against all of Y.  SCREEN: keys and counts of the row; else the cells of the two planes
template <bool SCREEN>
__global__ __launch_bounds__(BT) void pair_kernel(uint64_t row0, uint64_t rows, uint32_t nchunks, DevSide X, DevSide Y,
                                                  int32_t *__restrict__ dg_any, int32_t *__restrict__ dg_end,
                                                  unsigned long long *__restrict__ key_any, unsigned long long *__restrict__ key_end,
                                                  uint32_t *__restrict__ cnt_any, uint32_t *__restrict__ cnt_end, int any_thr, int end_thr)
{
    __shared__ int32_t Ps[64];
    const uint64_t items = rows * nchunks;
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) { // the same in the whole block
        const uint64_t xi = row0 + it / nchunks;
        const uint64_t j0 = (it % nchunks) * (uint64_t)CHUNK;
        const int m = (int)X.len[xi];
        if (SCREEN && m == 0)
            continue; // a bad x: the row keeps its empty key and its zero counts
        const uint64_t x0 = X.fwd[xi], x1 = X.fwd[X.n + xi], x2 = X.fwd[2 * X.n + xi], x3 = X.fwd[3 * X.n + xi];
        __syncthreads(); // the last item's readers are through
        if (threadIdx.x < 64)
            Ps[threadIdx.x] = X.P[xi * 64 + threadIdx.x];
        __syncthreads();
        int best_any = 0, best_end = 0;
        uint32_t j_any = NONE, j_end = NONE, n_any = 0, n_end = 0;
        for (int r = 0; r < CHUNK / BT; ++r) {
            const uint64_t j = j0 + (uint64_t)r * BT + threadIdx.x;
            const bool in = j < Y.n;
            const int n = in ? (int)Y.len[j] : 0;
            uint64_t y0 = 0, y1 = 0, y2 = 0, y3 = 0;
            if (n)
                y0 = Y.rev[j], y1 = Y.rev[Y.n + j], y2 = Y.rev[2 * Y.n + j], y3 = Y.rev[3 * Y.n + j];
            const int nmax = (int)dpp_wave_max((uint32_t)n);
            int any = 0, end = 0;
            if (m && nmax)
                pair_energies(x0, x1, x2, x3, m, Ps, y0, y1, y2, y3, nmax, any, end);
            if (SCREEN) {
                n_any += (uint32_t)__popcll(__ballot(n && any <= any_thr)); // the wave's count, in every lane
                n_end += (uint32_t)__popcll(__ballot(n && end <= end_thr));
                if (any < best_any) // a y without a run, a bad one among them, is never below 0
                    best_any = any, j_any = (uint32_t)j;
                if (end < best_end)
                    best_end = end, j_end = (uint32_t)j;
            } else if (in) {
                if (dg_any)
                    dg_any[xi * Y.n + j] = any;
                if (dg_end)
                    dg_end[xi * Y.n + j] = end;
            }
        }
        if (SCREEN) {
            // the wave's smallest (dg, j): first the energy, then the lowest j among the lanes that have it
            const uint32_t a = wave_min((uint32_t)best_any + KEY_BIAS), b = wave_min((uint32_t)best_end + KEY_BIAS);
            const uint32_t ja = wave_min((uint32_t)best_any + KEY_BIAS == a ? j_any : NONE);
            const uint32_t jb = wave_min((uint32_t)best_end + KEY_BIAS == b ? j_end : NONE);
            if ((threadIdx.x & 63) == 0) {
                if (a < KEY_BIAS)
                    atomicMin(&key_any[xi], (unsigned long long)a << 32 | ja);
                if (b < KEY_BIAS)
                    atomicMin(&key_end[xi], (unsigned long long)b << 32 | jb);
                if (n_any)
                    atomicAdd(&cnt_any[xi], n_any);
                if (n_end)
                    atomicAdd(&cnt_end[xi], n_end);
            }
        }
    }
}

// the outputs of row i from its two keys: the partner's pair once more, under the tie rule
__global__ __launch_bounds__(BT) void detail_kernel(uint64_t nx, DevSide X, DevSide Y, const unsigned long long *__restrict__ key_any,
                                                    const unsigned long long *__restrict__ key_end, int32_t *__restrict__ any_dg,
                                                    uint32_t *__restrict__ any_partner, uint32_t *__restrict__ any_shift,
                                                    uint32_t *__restrict__ any_pos, uint32_t *__restrict__ any_pairs,
                                                    int32_t *__restrict__ end_dg, uint32_t *__restrict__ end_partner,
                                                    uint32_t *__restrict__ end_shift, uint32_t *__restrict__ end_pairs)
{
    for (uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x; i < nx; i += (uint64_t)gridDim.x * BT) {
        const int m = (int)X.len[i];
        const uint64_t x0 = X.fwd[i], x1 = X.fwd[X.n + i], x2 = X.fwd[2 * X.n + i], x3 = X.fwd[3 * X.n + i];
        const int32_t *P = X.P + i * 64;
        for (int which = 0; which < 2; ++which) {
            const unsigned long long key = which ? key_end[i] : key_any[i];
            const uint32_t j = (uint32_t)key;
            int dg = 1, shift = 0, pos = 0, pairs = 0; // dg == 1: nothing yet; an energy is at most 0
            if (j != NONE) {
                const int n = (int)Y.len[j];
                const uint64_t y0 = Y.rev[j], y1 = Y.rev[Y.n + j], y2 = Y.rev[2 * Y.n + j], y3 = Y.rev[3 * Y.n + j];
                for (int s = 1 - n; s < m; ++s) {
                    const uint64_t M = (moved(x0, s) & y3) | (moved(x1, s) & y2) | (moved(x2, s) & y1) | (moved(x3, s) & y0);
                    uint64_t S = M & (M >> 1);
                    if (which) {
                        const int e = m - 2 - s;
                        if (e < 0 || e > 62)
                            continue;
                        const int run = __clzll((long long)~(S << (63 - e)));
                        const int d = P[m - 1] - P[(m - 1 - run) & 63];
                        if (run && d < dg)
                            dg = d, shift = s + n - 1, pos = m - 1 - run, pairs = run + 1;
                    } else {
                        while (S) {
                            const uint64_t up = S + (S & (0 - S));
                            const int k0 = __ffsll((unsigned long long)S) - 1, k1 = __ffsll((unsigned long long)up) - 1;
                            const int d = P[(k1 + s) & 63] - P[(k0 + s) & 63];
                            if (d < dg)
                                dg = d, shift = s + n - 1, pos = k0 + s, pairs = k1 - k0 + 1;
                            S &= up;
                        }
                    }
                }
            }
            if (dg > 0)
                dg = 0;
            if (which) {
                end_dg[i] = dg, end_partner[i] = j, end_shift[i] = (uint32_t)shift, end_pairs[i] = (uint32_t)pairs;
            } else {
                any_dg[i] = dg, any_partner[i] = j, any_shift[i] = (uint32_t)shift, any_pos[i] = (uint32_t)pos;
                any_pairs[i] = (uint32_t)pairs;
            }
        }
    }
}

// the library's nearest-neighbour table (c_nn of primers.hip) times ten: dH in 0.1 kcal/mol, dS in 0.1 cal/(mol K), in the order
// AA AC AG AT CA CC CG CT GA GC GG GT TA TC TG TT
constexpr int64_t NN_H10[16] = {-76, -84, -78, -72, -85, -80, -106, -78, -82, -98, -80, -84, -72, -82, -85, -76};
constexpr int64_t NN_S10[16] = {-213, -224, -210, -204, -227, -199, -272, -210, -222, -244, -199, -224, -213, -222, -227, -213};
constexpr uint32_t MIN_TEMP_MK = 273150, MAX_TEMP_MK = 338000;

// one side as the caller hands it over
struct HostSide {
    const uint8_t *bytes;
    const uint64_t *off;
    uint64_t n;
    uint32_t *err;
};

thread_local polyhip_dimer_info t_info{};

struct ScreenOut {
    int32_t *any_dg;
    uint32_t *any_partner, *any_shift, *any_pos, *any_pairs;
    int32_t *end_dg;
    uint32_t *end_partner, *end_shift, *end_pairs, *any_count, *end_count;
};

// both calls: scr == nullptr is the matrix call
int dimers(const char *who, const int32_t *stack, const int32_t *thresholds, HostSide hx, HostSide hy, int32_t *dg_any, int32_t *dg_end,
           const ScreenOut *scr)
{
    for (int t = 0; t < 16; ++t)
        PH_REQUIRE(stack[t] >= MIN_STACK && stack[t] <= 0, "%s: stack_dg[%d] = %d, an entry is %d..0", who, t, stack[t], MIN_STACK);
    if (scr) {
        PH_REQUIRE(thresholds[0] <= 0, "%s: any_threshold = %d, a threshold is at most 0", who, thresholds[0]);
        PH_REQUIRE(thresholds[1] <= 0, "%s: end_threshold = %d, a threshold is at most 0", who, thresholds[1]);
    }
    const bool pool = !hy.bytes && !hy.off && hy.n == 0;
    PH_REQUIRE(pool || (hy.bytes && hy.off && hy.n > 0),
               "%s: Y, offY and ny are all given, or NULL, NULL and 0 for the pool of X against itself", who);
    if (scr)
        PH_REQUIRE(scr->any_dg && scr->any_partner && scr->any_shift && scr->any_pos && scr->any_pairs && scr->end_dg && scr->end_partner &&
                       scr->end_shift && scr->end_pairs && scr->any_count && scr->end_count,
                   "%s: null output", who);
    else
        PH_REQUIRE(dg_any || dg_end, "%s: null output: dg_any and dg_end are both NULL", who);
    PH_REQUIRE(hx.err && (pool || hy.err), "%s: null output: %s", who, hx.err ? "errY" : "errX");
    PH_REQUIRE(hx.n == 0 || (hx.bytes && hx.off), "%s: null X or offX", who);
    for (uint64_t i = 0; i < hx.n; ++i)
        PH_REQUIRE(hx.off[i + 1] >= hx.off[i], "%s: offX is not ascending at %llu", who, (unsigned long long)i);
    for (uint64_t i = 0; i < hy.n; ++i)
        PH_REQUIRE(hy.off[i + 1] >= hy.off[i], "%s: offY is not ascending at %llu", who, (unsigned long long)i);
    const uint64_t ny = pool ? hx.n : hy.n;
    if (scr) {
        if (ny >= 0xFFFFFFFFull)
            return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %llu primers in Y, a partner is a 32-bit index below 2^32 - 1", who,
                             (unsigned long long)ny);
    } else if (hx.n && ny > MATRIX_CELLS / hx.n) {
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %llu x %llu cells, the matrix holds at most 2^30 (tile the call)", who,
                         (unsigned long long)hx.n, (unsigned long long)ny);
    }
    t_info = polyhip_dimer_info{};
    if (hx.n == 0)
        return POLYHIP_OK;

    // the counters need the lengths alone
    uint64_t good[2] = {0, 0}, bases[2] = {0, 0};
    const HostSide *side[2] = {&hx, pool ? &hx : &hy};
    for (int q = 0; q < 2; ++q)
        for (uint64_t i = 0; i < side[q]->n; ++i) {
            const uint64_t L = side[q]->off[i + 1] - side[q]->off[i];
            if (L >= 1 && L <= MAX_PRIMER)
                ++good[q], bases[q] += L;
        }
    const uint64_t nsides = pool ? 1 : 2, nx = hx.n;

    HostStreams &hs = host_streams();
    PH_HIP(hs.init());
    hipStream_t st = hs.s[0];
    Arena w;
    size_t o_bytes[2], o_off[2], o_fwd[2], o_rev[2], o_len[2], o_P[2], o_err[2];
    for (uint64_t q = 0; q < nsides; ++q) {
        const HostSide &h = *side[q];
        o_bytes[q] = w.reserve(h.off[h.n] - h.off[0]);
        o_off[q] = w.reserve((h.n + 1) * 8);
        o_fwd[q] = w.reserve(h.n * 32);
        o_rev[q] = w.reserve(h.n * 32);
        o_len[q] = w.reserve(h.n * 4);
        o_P[q] = w.reserve(h.n * 256);
        o_err[q] = w.reserve(h.n * 4);
    }
    const uint64_t cells = scr ? 0 : nx * ny;
    const size_t o_stack = w.reserve(64), o_any = w.reserve(!scr && dg_any ? cells * 4 : 0), o_end = w.reserve(!scr && dg_end ? cells * 4 : 0),
                 o_keys = w.reserve(scr ? nx * 16 : 0), o_cnt = w.reserve(scr ? nx * 8 : 0), o_out = w.reserve(scr ? nx * 36 : 0);
    PH_HIP(w.buf.alloc(w.used));
    SyncOnExit sync(st);
    uint64_t launches = 0;
    PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_stack), stack, 64, hipMemcpyHostToDevice, st));
    DevSide ds[2];
    for (uint64_t q = 0; q < nsides; ++q) {
        const HostSide &h = *side[q];
        const uint64_t nbytes = h.off[h.n] - h.off[0];
        if (nbytes)
            PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_bytes[q]), h.bytes + h.off[0], nbytes, hipMemcpyHostToDevice, st));
        PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_off[q]), h.off, (h.n + 1) * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(prepare_kernel, dim3(grid_for(h.n)), dim3(BT), 0, st, h.n, w.at<uint8_t>(o_bytes[q]), w.at<uint64_t>(o_off[q]),
                           w.at<int32_t>(o_stack), w.at<uint64_t>(o_fwd[q]), w.at<uint64_t>(o_rev[q]), w.at<uint32_t>(o_len[q]),
                           w.at<int32_t>(o_P[q]), w.at<uint32_t>(o_err[q]));
        PH_HIP(hipGetLastError());
        ++launches;
        PH_HIP(hipMemcpyAsync(h.err, w.at<uint8_t>(o_err[q]), h.n * 4, hipMemcpyDeviceToHost, st));
        ds[q] = DevSide{w.at<uint64_t>(o_fwd[q]), w.at<uint64_t>(o_rev[q]), w.at<uint32_t>(o_len[q]), w.at<int32_t>(o_P[q]), h.n};
    }
    if (pool)
        ds[1] = ds[0];
    const uint32_t nchunks = (uint32_t)((ny + CHUNK - 1) / CHUNK);
    if (!scr) {
        int32_t *d_any = dg_any ? w.at<int32_t>(o_any) : nullptr, *d_end = dg_end ? w.at<int32_t>(o_end) : nullptr;
        hipLaunchKernelGGL(pair_kernel<false>, dim3(grid_for(nx * nchunks, 1, 256 * 64)), dim3(BT), 0, st, (uint64_t)0, nx, nchunks, ds[0],
                           ds[1], d_any, d_end, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr,
                           (uint32_t *)nullptr, 0, 0);
        PH_HIP(hipGetLastError());
        ++launches;
        if (dg_any)
            PH_HIP(hipMemcpyAsync(dg_any, d_any, cells * 4, hipMemcpyDeviceToHost, st));
        if (dg_end)
            PH_HIP(hipMemcpyAsync(dg_end, d_end, cells * 4, hipMemcpyDeviceToHost, st));
    } else {
        unsigned long long *k_any = w.at<unsigned long long>(o_keys), *k_end = k_any + nx;
        uint32_t *c_any = w.at<uint32_t>(o_cnt), *c_end = c_any + nx;
        PH_HIP(hipMemsetAsync(k_any, 0xFF, nx * 16, st)); // the empty key, above every real one; its low word is "no partner"
        PH_HIP(hipMemsetAsync(c_any, 0, nx * 8, st));
        const uint64_t rows_max = std::max<uint64_t>(1, launch_pairs() / ny);
        for (uint64_t row0 = 0; row0 < nx; row0 += rows_max) {
            const uint64_t rows = std::min(rows_max, nx - row0);
            hipLaunchKernelGGL(pair_kernel<true>, dim3(grid_for(rows * nchunks, 1, 256 * 64)), dim3(BT), 0, st, row0, rows, nchunks, ds[0],
                               ds[1], (int32_t *)nullptr, (int32_t *)nullptr, k_any, k_end, c_any, c_end, (int)thresholds[0],
                               (int)thresholds[1]);
            PH_HIP(hipGetLastError());
            ++launches;
        }
        uint32_t *o = w.at<uint32_t>(o_out); // nine arrays of nx
        hipLaunchKernelGGL(detail_kernel, dim3(grid_for(nx)), dim3(BT), 0, st, nx, ds[0], ds[1], k_any, k_end, (int32_t *)o, o + nx,
                           o + 2 * nx, o + 3 * nx, o + 4 * nx, (int32_t *)(o + 5 * nx), o + 6 * nx, o + 7 * nx, o + 8 * nx);
        PH_HIP(hipGetLastError());
        ++launches;
        void *dst[9] = {scr->any_dg,      scr->any_partner, scr->any_shift, scr->any_pos, scr->any_pairs, scr->end_dg,
                        scr->end_partner, scr->end_shift,   scr->end_pairs};
        for (int k = 0; k < 9; ++k)
            PH_HIP(hipMemcpyAsync(dst[k], o + (uint64_t)k * nx, nx * 4, hipMemcpyDeviceToHost, st));
        PH_HIP(hipMemcpyAsync(scr->any_count, c_any, nx * 4, hipMemcpyDeviceToHost, st));
        PH_HIP(hipMemcpyAsync(scr->end_count, c_end, nx * 4, hipMemcpyDeviceToHost, st));
    }
    PH_HIP(hipStreamSynchronize(st));
    t_info = polyhip_dimer_info{hx.n + hy.n, hx.n + hy.n - good[0] - (pool ? 0 : good[1]), good[0] * good[1],
                                good[1] * bases[0] + good[0] * bases[1] - good[0] * good[1], launches};
    return POLYHIP_OK;
}

} // namespace
} // namespace polyhip

using namespace polyhip;

extern "C" {

int polyhip_primer_stack_dg(uint32_t temp_mK, int32_t out[16])
{
    PH_REQUIRE(out, "polyhip_primer_stack_dg: null argument");
    PH_REQUIRE(temp_mK >= MIN_TEMP_MK && temp_mK <= MAX_TEMP_MK, "polyhip_primer_stack_dg: temp_mK = %u, it is %u..%u", temp_mK, MIN_TEMP_MK,
               MAX_TEMP_MK);
    for (int t = 0; t < 16; ++t) {
        const int64_t num = NN_H10[t] * 1000000 - (int64_t)temp_mK * NN_S10[t];
        const int64_t mag = ((num < 0 ? -num : num) + 5000) / 10000;
        out[t] = (int32_t)(num < 0 ? -mag : mag);
    }
    return POLYHIP_OK;
}

int polyhip_primer_dimer_matrix(const int32_t stack_dg[16], const uint8_t *X, const uint64_t *offX, uint64_t nx, const uint8_t *Y,
                                const uint64_t *offY, uint64_t ny, int32_t *dg_any, int32_t *dg_end, uint32_t *errX, uint32_t *errY)
{
    PH_REQUIRE(stack_dg, "polyhip_primer_dimer_matrix: null stack_dg");
    return dimers("polyhip_primer_dimer_matrix", stack_dg, nullptr, HostSide{X, offX, nx, errX}, HostSide{Y, offY, ny, errY}, dg_any, dg_end,
                  nullptr);
}

int polyhip_primer_dimer_screen(const polyhip_dimer_params *params, const uint8_t *X, const uint64_t *offX, uint64_t nx, const uint8_t *Y,
                                const uint64_t *offY, uint64_t ny, int32_t *any_dg, uint32_t *any_partner, uint32_t *any_shift,
                                uint32_t *any_pos, uint32_t *any_pairs, int32_t *end_dg, uint32_t *end_partner, uint32_t *end_shift,
                                uint32_t *end_pairs, uint32_t *any_count, uint32_t *end_count, uint32_t *errX, uint32_t *errY)
{
    PH_REQUIRE(params, "polyhip_primer_dimer_screen: null params");
    const int32_t thresholds[2] = {params->any_threshold, params->end_threshold};
    const ScreenOut scr{any_dg, any_partner, any_shift, any_pos, any_pairs, end_dg, end_partner, end_shift, end_pairs, any_count, end_count};
    return dimers("polyhip_primer_dimer_screen", params->stack_dg, thresholds, HostSide{X, offX, nx, errX}, HostSide{Y, offY, ny, errY},
                  nullptr, nullptr, &scr);
}

int polyhip_primer_dimer_last_info(polyhip_dimer_info *info)
{
    PH_REQUIRE(info, "polyhip_primer_dimer_last_info: null argument");
    *info = t_info;
    return POLYHIP_OK;
}

} // extern "C"
