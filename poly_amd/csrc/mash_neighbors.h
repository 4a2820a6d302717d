// mash_neighbors.h -- K2 neighbour lists: the all-vs-all join answered as CSR (threshold and top-k) instead of a dense matrix.
//
// Included at the END of mash_distance.hip: it uses that file's index (layout, build, item formats), its dense-join
// geometry and its merge (similarity_count), and changes none of them.  See DESIGN.md, K2, "neighbour lists".
//
//   blocks    Y is processed in column blocks of at most one dense stripe (about 105k columns at SketchSize <= 1023); the
//             existing index is built per block, in the same workspace, and all rows of X are joined against it
//   join      rowjoin_nbr_kernel: the walk rowjoin_dense_kernel uses (BucketWalk: descriptors a row ahead, DENSE_U buckets per
//             wave; one LDS atomic per item, 10- or 16-bit counters), then a flush that COMPACTS: the counter dwords are read, tested
//             against min_shared and the self column, and the survivors -- (column, shared), ascending column -- go to a
//             segment of a temporary list that the row reserves with one atomic; the counters are cleared in the same pass.
//             An irregular row (flagsX) fills the same counters from the reference's merge, a regular row adds its irregular
//             columns (flagsY / irrY) the same way: one flush, one test, for every kind of pair.
//   assemble  one pass with reserved segments: (row, block) -> (position, count), a scan over the rows' totals gives
//             first[], and a wave per row copies its segments (k == 0) or selects the k best of them (k > 0) into the
//             caller's cols / shared / dist.  Rows in order, blocks in order, a segment in ascending column: canonical
//             whatever order the atomics ran in.
//   overflow  the temporary list holds max(1024 per row, ny) entries; a row range that needs more is cut into pieces and
//             joined again (the true counts are known either way).
#pragma once

namespace polyhip {
namespace k2 {

constexpr uint32_t NBR_PER_MAX = 3; // counter fields per dword at most (10-bit counters)

template <int BITS, bool COMPACT, bool REG>
__global__ __launch_bounds__(DENSE_THREADS) void rowjoin_nbr_kernel(
    const uint32_t *__restrict__ X, uint64_t nx, uint32_t sx, const uint8_t *__restrict__ flagsX, int merge_all,
    const uint32_t *__restrict__ Y, uint32_t ncols, uint32_t sy, const uint32_t *__restrict__ irrY,
    const uint32_t *__restrict__ start, const void *__restrict__ items_v, uint32_t nbk, const uint32_t *__restrict__ hdr,
    uint32_t ndw, uint32_t id_bits, uint32_t min_shared, int has_self, long long self_rel, uint32_t col0,
    uint32_t *__restrict__ segcnt, unsigned long long *__restrict__ segpos, unsigned long long *__restrict__ cursor,
    uint32_t *__restrict__ tcols, uint16_t *__restrict__ tshared, unsigned long long tempcap)
{
    constexpr uint32_t NWAVES = DENSE_THREADS / 64;
    if ((hdr[H_FMT] != 0u) != COMPACT) // the index says which item format it holds; the other instantiation has nothing to do
        return;
    constexpr uint32_t PER = 32 / BITS, FMASK = (1u << BITS) - 1u;
    static_assert(PER <= NBR_PER_MAX && PER * NWAVES <= 64, "the flush scans PER * NWAVES wave totals in one wave");
    typedef BucketWalk<COMPACT, REG> Walk;
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
    uint32_t *dense = dyn; // (REG: no row stage behind the counters)
    __shared__ uint32_t ndist;
    __shared__ uint32_t wcnt[NBR_PER_MAX * NWAVES];
    __shared__ unsigned long long rowpos;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t id_mask = (1u << id_bits) - 1u;
    const Walk walk{X, sx, start, static_cast<const typename Walk::Item *>(items_v), nbk, hdr[H_SHIFT], id_bits, dyn + ndw, &ndist, tid};
    const uint32_t nirr = hdr[H_NIRRY];
    // consecutive rows on one XCD, as in rowjoin_dense_kernel
    const uint32_t G = gridDim.x, per_xcd = G / 8u;
    const bool by_xcd = per_xcd != 0 && G % 8u == 0;
    const uint64_t off = by_xcd ? (uint64_t)(blockIdx.x % 8u) * per_xcd + blockIdx.x / 8u : blockIdx.x;
    // column c = field c / ndw of dword c % ndw (what a compact item has worked out already)
    const uint32_t kmul = (uint32_t)(((1ull << 32) + ndw - 1) / ndw);
    auto bump = [&](uint32_t col, uint32_t by) {
        const uint32_t k = __umulhi(col, kmul);
        atomicAdd(&dense[col - k * ndw], by << (BITS * k));
    };
    auto consume = [&](const typename Walk::Item it, uint32_t key, uint32_t lim) {
        if constexpr (COMPACT) {
            if (it - key < lim)
                atomicAdd(reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(dense) + ((it >> 3) & 0x3FFFCu)), 1u << (it & 31u));
        } else {
            if (it.x == key && it.y < lim)
                bump(it.y & id_mask, 1u);
        }
    };
    auto load_row = [&](uint64_t k, RowAhead &q) { // my k-th row of X; an irregular one (or every one) is the merge's
        const uint64_t r = k * G + off;
        q = RowAhead{};
        if (r < nx)
            walk.load_row(q, r, merge_all ? 1u : flagsX[r]);
    };
    // the counters start at zero and every flush leaves them so
    for (uint32_t t = tid * 4; t < ndw; t += DENSE_THREADS * 4) // ndw is a multiple of 8
        *reinterpret_cast<uint4 *>(dense + t) = make_uint4(0, 0, 0, 0);
    lds_barrier();
    RowAhead cur, nxt;
    load_row(0, cur);
    walk.load_bounds(cur);
    load_row(1, nxt);
    for (uint64_t k = 0; cur.i >= 0; ++k) {
        const uint64_t i = (uint64_t)cur.i;
        const bool work = !cur.skip; // wave-uniform
        typename Walk::Desc desc;
        if (work)
            desc = walk.describe(cur);
        // issue the loads of the rows ahead now: they land while this row's buckets are walked
        RowAhead nn;
        walk.load_bounds(nxt);
        load_row(k + 2, nn);
        cur = nxt;
        nxt = nn;
        if (work) {
            walk.walk(desc, consume);
            // the row's irregular columns never entered the index: the reference's merge, into the same counters
            for (uint32_t q = tid; q < nirr; q += DENSE_THREADS) {
                const uint32_t j = irrY[q];
                const uint32_t c = similarity_count(X + i * sx, sx, Y + (uint64_t)j * sy, sy);
                if (c)
                    bump(j, c);
            }
        } else {
            // an irregular row: every column through the merge
            for (uint32_t j = tid; j < ncols; j += DENSE_THREADS) {
                const uint32_t c = similarity_count(X + i * sx, sx, Y + (uint64_t)j * sy, sy);
                if (c)
                    bump(j, c);
            }
        }
        lds_barrier();
        // ---- the compacting flush.  Wave w owns the counter dwords [w * WD, (w + 1) * WD): within a field the order (wave,
        // trip, lane) is ascending column, so a survivor's place in the row is
        //     (survivors of the fields below) + (of this field in the waves below) + (in this wave so far) + (in the lanes below)
        // -- pass 1 counts per (field, wave), one wave-sized scan turns the PER * NWAVES totals into bases, pass 2 reads the
        // dwords again, writes the survivors and clears what it read.  Nearly all dwords are zero: a trip whose 64 dwords are
        // all zero is one LDS read and one ballot.
        const uint32_t WD = (((ndw + NWAVES - 1) / NWAVES) + 63u) & ~63u;
        const uint32_t w_lo = min((uint32_t)wave * WD, ndw), w_hi = min(w_lo + WD, ndw);
        const long long selfc = has_self ? self_rel + (long long)i : -1ll;
        uint32_t cnt[PER];
#pragma unroll
        for (uint32_t f = 0; f < PER; ++f)
            cnt[f] = 0;
        for (uint32_t t0 = w_lo; t0 < w_hi; t0 += 64) {
            const uint32_t t = t0 + lane;
            const uint32_t d = t < w_hi ? dense[t] : 0u;
            if (__ballot(d != 0u) == 0ull)
                continue;
#pragma unroll
            for (uint32_t f = 0; f < PER; ++f) {
                const uint32_t c = (d >> (BITS * f)) & FMASK, col = f * ndw + t;
                const bool pass = c >= min_shared && col < ncols && (long long)col != selfc;
                cnt[f] += (uint32_t)__builtin_popcountll(__ballot(pass));
            }
        }
        if (lane == 0) {
#pragma unroll
            for (uint32_t f = 0; f < PER; ++f)
                wcnt[f * NWAVES + wave] = cnt[f];
        }
        lds_barrier();
        uint32_t mine = (uint32_t)lane < PER * NWAVES ? wcnt[lane] : 0u, incl = mine;
#pragma unroll
        for (int dlt = 1; dlt < 64; dlt <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, dlt, 64);
            if (lane >= dlt)
                incl += up;
        }
        const uint32_t total = (uint32_t)__shfl((int)incl, (int)(PER * NWAVES - 1), 64);
        uint32_t base[PER];
#pragma unroll
        for (uint32_t f = 0; f < PER; ++f)
            base[f] = (uint32_t)__shfl((int)(incl - mine), (int)(f * NWAVES + wave), 64);
        if (tid == 0) {
            const unsigned long long p = total ? atomicAdd(cursor, (unsigned long long)total) : 0ull;
            rowpos = p;
            segcnt[i] = total;
            segpos[i] = p;
        }
        lds_barrier();
        const unsigned long long pos = rowpos;
        const bool store = pos + total <= tempcap; // (wave-uniform; a list that does not fit is joined again in smaller pieces)
        for (uint32_t t0 = w_lo; t0 < w_hi; t0 += 64) {
            const uint32_t t = t0 + lane;
            const uint32_t d = t < w_hi ? dense[t] : 0u;
            if (__ballot(d != 0u) == 0ull)
                continue;
            if (d)
                dense[t] = 0;
#pragma unroll
            for (uint32_t f = 0; f < PER; ++f) {
                const uint32_t c = (d >> (BITS * f)) & FMASK, col = f * ndw + t;
                const bool pass = c >= min_shared && col < ncols && (long long)col != selfc;
                const uint64_t m = __ballot(pass);
                if (pass && store) {
                    const unsigned long long p = pos + base[f] + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
                    tcols[p] = col0 + col;
                    tshared[p] = (uint16_t)c;
                }
                base[f] += (uint32_t)__builtin_popcountll(m);
            }
        }
        lds_barrier();
    }
}

// ---- first[] from the (row, block) counts: three small kernels (per-1024-row sums, their scan, the rows' own scan)
__device__ __forceinline__ unsigned long long nbr_row_out(const uint32_t *__restrict__ segcnt, uint64_t nr, uint32_t nblocks,
                                                          uint64_t i, uint32_t k)
{
    unsigned long long t = 0;
    for (uint32_t b = 0; b < nblocks; ++b)
        t += segcnt[(uint64_t)b * nr + i];
    return k ? min(t, (unsigned long long)k) : t;
}

// exclusive scan of one value per thread over a 1024-thread workgroup; *total = the workgroup's sum
__device__ __forceinline__ unsigned long long nbr_block_scan(unsigned long long v, unsigned long long *wsum, unsigned long long *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long up = __shfl_up(incl, d, 64);
        if (lane >= d)
            incl += up;
    }
    __syncthreads(); // (wsum of the call before has been read)
    if (lane == 63)
        wsum[wave] = incl;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (int w = 0; w < 16; ++w) {
        const unsigned long long s = wsum[w];
        before += w < wave ? s : 0ull;
        all += s;
    }
    *total = all;
    return before + incl - v;
}

__global__ __launch_bounds__(1024) void nbr_sums_kernel(const uint32_t *__restrict__ segcnt, uint64_t nr, uint32_t nblocks, uint32_t k,
                                                       unsigned long long *__restrict__ bsum)
{
    __shared__ unsigned long long wsum[16];
    const uint64_t i = (uint64_t)blockIdx.x * 1024 + threadIdx.x;
    unsigned long long total;
    (void)nbr_block_scan(i < nr ? nbr_row_out(segcnt, nr, nblocks, i, k) : 0ull, wsum, &total);
    if (threadIdx.x == 0)
        bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void nbr_scan_sums_kernel(unsigned long long *__restrict__ bsum, uint64_t nb,
                                                            unsigned long long *__restrict__ totals)
{
    __shared__ unsigned long long wsum[16];
    unsigned long long carry = 0;
    for (uint64_t b0 = 0; b0 < nb; b0 += 1024) {
        const uint64_t b = b0 + threadIdx.x;
        unsigned long long total;
        const unsigned long long ex = nbr_block_scan(b < nb ? bsum[b] : 0ull, wsum, &total);
        if (b < nb)
            bsum[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0)
        totals[0] = carry; // entries of this row range after top-k
}

__global__ __launch_bounds__(1024) void nbr_first_kernel(const uint32_t *__restrict__ segcnt, uint64_t nr, uint32_t nblocks, uint32_t k,
                                                        const unsigned long long *__restrict__ bsum,
                                                        const unsigned long long *__restrict__ totals, unsigned long long out_base,
                                                        unsigned long long *__restrict__ first)
{
    __shared__ unsigned long long wsum[16];
    const uint64_t i = (uint64_t)blockIdx.x * 1024 + threadIdx.x;
    unsigned long long total;
    const unsigned long long ex = nbr_block_scan(i < nr ? nbr_row_out(segcnt, nr, nblocks, i, k) : 0ull, wsum, &total);
    if (i < nr)
        first[i] = out_base + bsum[blockIdx.x] + ex;
    if (i == nr - 1)
        first[nr] = out_base + totals[0];
}

// ---- a wave per row: the row's segments, block after block, into its place in the caller's list.  k == 0: a copy
// (ascending column).  k > 0: selection -- the survivor with the largest (shared, then SMALLER column) below the one
// written last, k times; the candidates are a few hundred per row, read from L2.  The cost is k * candidates / 64 reads
// per row on ONE wave: right for a short list (k = 10 of a few hundred; measured in DESIGN.md, K2 "neighbour lists"), slow
// for a large k against rows of tens of thousands of candidates -- there is no workgroup-per-row form for long rows yet,
// so the entry points refuse k above POLYHIP_MASH_NEIGHBORS_MAX_K.
__global__ __launch_bounds__(THREADS) void nbr_assemble_kernel(uint64_t nr, uint32_t nblocks, const uint32_t *__restrict__ segcnt,
                                                              const unsigned long long *__restrict__ segpos,
                                                              const uint32_t *__restrict__ tcols, const uint16_t *__restrict__ tshared,
                                                              const unsigned long long *__restrict__ first, uint32_t k, double smaller,
                                                              uint32_t *__restrict__ cols, uint16_t *__restrict__ shared,
                                                              double *__restrict__ dist, unsigned long long cap,
                                                              const unsigned long long *__restrict__ cursor, unsigned long long tempcap)
{
    if (cursor[0] > tempcap) // the temporary list overflowed: the host joins these rows again in pieces
        return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * THREADS + threadIdx.x) >> 6, nwaves = (uint64_t)gridDim.x * (THREADS / 64);
    for (uint64_t i = wave; i < nr; i += nwaves) {
        const unsigned long long o = first[i], n_out = first[i + 1] - o;
        if (o >= cap || n_out == 0)
            continue;
        if (k == 0) {
            unsigned long long run = o;
            for (uint32_t b = 0; b < nblocks; ++b) {
                const uint32_t cnt = segcnt[(uint64_t)b * nr + i];
                const unsigned long long pos = segpos[(uint64_t)b * nr + i];
                for (uint32_t e = lane; e < cnt; e += 64) {
                    const unsigned long long dst = run + e;
                    if (dst < cap) {
                        const uint32_t c = tshared[pos + e];
                        cols[dst] = tcols[pos + e];
                        shared[dst] = (uint16_t)c;
                        if (dist)
                            dist[dst] = 1 - (double)c / smaller;
                    }
                }
                run += cnt;
            }
            continue;
        }
        unsigned long long prev = ~0ull; // key = shared << 32 | ~column: larger is better
        for (unsigned long long sel = 0; sel < n_out && o + sel < cap; ++sel) {
            unsigned long long best = 0;
            for (uint32_t b = 0; b < nblocks; ++b) {
                const uint32_t cnt = segcnt[(uint64_t)b * nr + i];
                const unsigned long long pos = segpos[(uint64_t)b * nr + i];
                for (uint32_t e = lane; e < cnt; e += 64) {
                    const unsigned long long key = ((unsigned long long)tshared[pos + e] << 32) | (0xFFFFFFFFu - tcols[pos + e]);
                    if (key < prev && key > best)
                        best = key;
                }
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1)
                best = max(best, (unsigned long long)__shfl_xor(best, d, 64));
            if (lane == 0) {
                const uint32_t c = (uint32_t)(best >> 32);
                cols[o + sel] = 0xFFFFFFFFu - (uint32_t)best;
                shared[o + sel] = (uint16_t)c;
                if (dist)
                    dist[o + sel] = 1 - (double)c / smaller;
            }
            prev = best;
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
struct NbrGeom {
    int bits;            // counter width: the one compact items of a Y block are made for (a function of sy alone)
    uint32_t per;
    bool reg, merge_all; // a thread per row element / rows beyond the LDS stage: every pair through the merge
    size_t row_bytes;
    uint64_t block_cols; // columns of a Y block
};

struct NbrLayout {
    size_t index_bytes, off_flagsX, off_scal, off_bsum, off_segcnt, off_segpos, off_tcols, off_tshared, total;
    uint64_t tempcap, nblocks;
};

} // namespace k2
} // namespace polyhip

static k2::NbrGeom nbr_geom(uint32_t sx, uint32_t sy)
{
    k2::NbrGeom g;
    g.bits = sy <= 1023u ? 10 : 16;
    g.per = 32u / (uint32_t)g.bits;
    g.reg = reg_rows(sx);
    const size_t lds_max = 160 * 1024 - 1024, stage = g.reg ? 0 : (size_t)5 * sx * 4;
    g.merge_all = stage + 32 * 1024 > lds_max;
    g.row_bytes = g.merge_all ? 0 : stage;
    const size_t sdw_cap = g.per == 3 ? 37832u : 46328u; // (the multiply-high `column / ndw`, as in dense_geom)
    const uint64_t dwords = std::min<size_t>(((lds_max - g.row_bytes) / 4) & ~(size_t)7, sdw_cap);
    g.block_cols = dwords * g.per;
    // no wider than one stripe of the geometry the index is built for: the build then makes compact items
    const DenseGeom gY = dense_geom(sy, sy, 1);
    if (gY.stripe_cols)
        g.block_cols = std::min<uint64_t>(g.block_cols, gY.stripe_cols);
    // and no more hashes than ONE index takes (shared_counts_impl: ny * sy < 2^32)
    g.block_cols = std::max<uint64_t>(std::min<uint64_t>(g.block_cols, 0xFFFFFFFFull / sy), 1);
    return g;
}

static k2::NbrLayout nbr_layout(uint64_t nx, uint32_t sx, uint64_t ny, uint32_t sy)
{
    k2::NbrLayout L;
    const k2::NbrGeom g = nbr_geom(sx, sy);
    const uint64_t bc = std::min<uint64_t>(std::max<uint64_t>(ny, 1), g.block_cols);
    L.nblocks = ny ? (ny + bc - 1) / bc : 0;
    L.index_bytes = k2::layout(0, 1, bc, sy).off_flagsX;
    // the temporary list: 1024 entries per row, or a whole row of Y, but never more than there are pairs
    const unsigned __int128 pairs = (unsigned __int128)nx * ny;
    const uint64_t want = std::max<uint64_t>(std::max<uint64_t>(nx * 1024ull, ny), 1ull << 20);
    L.tempcap = pairs < want ? (uint64_t)pairs : want;
    size_t o = L.index_bytes;
    L.off_flagsX = o; o += k2::al(nx);
    L.off_scal = o; o += k2::al(64);
    L.off_bsum = o; o += k2::al(((nx + 1023) / 1024 + 1) * 8);
    L.off_segcnt = o; o += k2::al(L.nblocks * nx * 4);
    L.off_segpos = o; o += k2::al(L.nblocks * nx * 8);
    L.off_tcols = o; o += k2::al(L.tempcap * 4);
    L.off_tshared = o; o += k2::al(L.tempcap * 2);
    L.total = o;
    return L;
}

static thread_local polyhip_neighbors_info g_nbr_info;

namespace {
struct NbrCall {
    const uint32_t *dX, *dY;
    uint64_t nx, ny;
    uint32_t sx, sy, min_shared, k;
    int exclude_self;
    uint64_t self_offset;
    unsigned long long *d_first;
    uint32_t *d_cols;
    uint16_t *d_shared;
    double *d_dist;
    uint64_t capacity;
    uint8_t *w;
    k2::NbrLayout L;
    k2::NbrGeom g;
    hipStream_t st;
    polyhip_stream_t stream;
    int64_t block_in_index = -1; // the Y block whose index the workspace holds
    polyhip_neighbors_info info{};
};
} // namespace

// rows [r0, r0 + nr) of X against all of Y; their entries start at *out_base of the caller's list
static int nbr_rows(NbrCall &c, uint64_t r0, uint64_t nr, uint64_t *out_base)
{
    using namespace k2;
    uint8_t *w = c.w;
    const NbrLayout &L = c.L;
    uint32_t *hdr = reinterpret_cast<uint32_t *>(w);
    uint8_t *flagsX = w + L.off_flagsX;
    unsigned long long *scal = reinterpret_cast<unsigned long long *>(w + L.off_scal); // [0] cursor, [1] entries after top-k
    unsigned long long *bsum = reinterpret_cast<unsigned long long *>(w + L.off_bsum);
    uint32_t *segcnt = reinterpret_cast<uint32_t *>(w + L.off_segcnt);
    unsigned long long *segpos = reinterpret_cast<unsigned long long *>(w + L.off_segpos);
    uint32_t *tcols = reinterpret_cast<uint32_t *>(w + L.off_tcols);
    uint16_t *tshared = reinterpret_cast<uint16_t *>(w + L.off_tshared);
    const uint32_t *dx = c.dX + r0 * (uint64_t)c.sx;
    const bool fill = c.d_cols != nullptr;
    hipStream_t st = c.st;

    PH_HIP(hipMemsetAsync(scal, 0, 64, st));
    PH_HIP(hipMemsetAsync(flagsX, 0, nr, st));
    if (!c.g.merge_all)
        hipLaunchKernelGGL(check_kernel<false>, dim3(check_grid(nr)), dim3(THREADS), 0, st, dx, nr, c.sx, flagsX, hdr, 0, 0xFFFFFFFEu, 0u,
                           0u, 0u, (uint32_t *)nullptr, 0u);
    const uint64_t bc = std::min<uint64_t>(c.ny, c.g.block_cols);
    for (uint64_t b = 0; b < L.nblocks; ++b) {
        const uint64_t c0 = b * bc, m = std::min<uint64_t>(bc, c.ny - c0);
        const uint32_t *dy = c.dY + c0 * (uint64_t)c.sy;
        const Layout LI = layout(0, 1, m, c.sy);
        if (c.block_in_index != (int64_t)b) {
            if (int rc = polyhip_mash_index_build_dev(dy, m, c.sy, w, L.index_bytes, c.stream))
                return rc;
            c.block_in_index = (int64_t)b;
            ++c.info.index_builds;
        }
        const uint32_t id_bits = id_bits_of(m);
        const uint32_t ndw = (uint32_t)((((m + c.g.per - 1) / c.g.per) + 7) & ~7ull);
        const size_t smem = (size_t)ndw * 4 + c.g.row_bytes;
        // the build makes compact items for dense_geom(sy, sy, m) alone: where that rules them out only the 8-byte
        // instantiation is launched (as the dense path's allow_compact does); otherwise the device decided (H_FMT) and the
        // instantiation that does not match returns at once
        const bool may_compact = dense_geom(c.sy, c.sy, m).compact_ok;
        const unsigned blocks = (unsigned)std::min<uint64_t>(nr, 256ull);
        const long long self_rel = (long long)(c.self_offset + r0) - (long long)c0;
#define PH_K2_NBR_LAUNCH(BITS_, COMPACT_, REG_)                                                                               \
    do {                                                                                                                      \
        auto kern = rowjoin_nbr_kernel<BITS_, COMPACT_, REG_>;                                                                \
        if ((COMPACT_) && !may_compact)                                                                                       \
            break;                                                                                                            \
        if (b == 0) /* the first block is the widest: one attribute call per instantiation and row range */                    \
            PH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,      \
                                       (int)smem));                                                                           \
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(DENSE_THREADS), smem, st, dx, nr, c.sx, flagsX, c.g.merge_all ? 1 : 0, dy, \
                           (uint32_t)m, c.sy, reinterpret_cast<const uint32_t *>(w + LI.off_irrY),                            \
                           reinterpret_cast<const uint32_t *>(w + LI.off_start), static_cast<const void *>(w + LI.off_items), \
                           LI.nbk, hdr, ndw, id_bits, c.min_shared, c.exclude_self ? 1 : 0, self_rel, (uint32_t)c0,           \
                           segcnt + b * nr, segpos + b * nr, scal, tcols, tshared,                                            \
                           (unsigned long long)(fill ? L.tempcap : 0));                                                       \
    } while (0)
        const bool reg = c.g.reg && !c.g.merge_all;
        if (c.g.bits == 10) {
            if (reg) {
                PH_K2_NBR_LAUNCH(10, false, true);
                PH_K2_NBR_LAUNCH(10, true, true);
            } else {
                PH_K2_NBR_LAUNCH(10, false, false);
                PH_K2_NBR_LAUNCH(10, true, false);
            }
        } else {
            if (reg) {
                PH_K2_NBR_LAUNCH(16, false, true);
                PH_K2_NBR_LAUNCH(16, true, true);
            } else {
                PH_K2_NBR_LAUNCH(16, false, false);
                PH_K2_NBR_LAUNCH(16, true, false);
            }
        }
#undef PH_K2_NBR_LAUNCH
    }
    // first[] and the assembly are enqueued behind the join without waiting for it: the cursor (did the temporary list hold
    // everything?) and the range's total come back in ONE synchronisation, and the assembly checks the cursor for itself
    const unsigned nb = (unsigned)((nr + 1023) / 1024);
    hipLaunchKernelGGL(nbr_sums_kernel, dim3(nb), dim3(1024), 0, st, segcnt, nr, (uint32_t)L.nblocks, c.k, bsum);
    hipLaunchKernelGGL(nbr_scan_sums_kernel, dim3(1), dim3(1024), 0, st, bsum, (uint64_t)nb, scal + 1);
    hipLaunchKernelGGL(nbr_first_kernel, dim3(nb), dim3(1024), 0, st, segcnt, nr, (uint32_t)L.nblocks, c.k, bsum, scal + 1,
                       (unsigned long long)*out_base, c.d_first + r0);
    if (fill && *out_base < c.capacity) {
        const unsigned grid = (unsigned)std::min<uint64_t>((nr + THREADS / 64 - 1) / (THREADS / 64), 256ull * 8ull);
        hipLaunchKernelGGL(nbr_assemble_kernel, dim3(grid), dim3(THREADS), 0, st, nr, (uint32_t)L.nblocks, segcnt, segpos, tcols, tshared,
                           c.d_first + r0, c.k, (double)std::min(c.sx, c.sy), c.d_cols, c.d_shared, c.d_dist,
                           (unsigned long long)c.capacity, scal, (unsigned long long)L.tempcap);
    }
    PH_HIP(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    PH_HIP(hipMemcpyAsync(h, scal, 16, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    if (fill && h[0] > L.tempcap && nr > 1) {
        // more survivors than the temporary list holds: the same rows again in as many pieces as the count asks for (a
        // piece that still does not fit is cut again; a single row has at most ny entries and always fits)
        const uint64_t pieces = std::min<uint64_t>(nr, h[0] / L.tempcap + 1);
        for (uint64_t p = 0; p < pieces; ++p) {
            const uint64_t a = (uint64_t)(((unsigned __int128)nr * p) / pieces), b = (uint64_t)(((unsigned __int128)nr * (p + 1)) / pieces);
            if (int rc = nbr_rows(c, r0 + a, b - a, out_base))
                return rc;
        }
        return POLYHIP_OK;
    }
    ++c.info.row_chunks;
    c.info.entries_thresholded += h[0];
    *out_base += h[1];
    return POLYHIP_OK;
}

// statuses and messages of shared_counts_impl, in its order; then the list's own
static int nbr_check_args(uint64_t nx, uint32_t sx, uint64_t ny, uint32_t sy, uint32_t min_shared, uint32_t k)
{
    if (sx == 0 || sy == 0)
        return set_error(POLYHIP_ERR_PANIC,
                         "mash.Similarity with SketchSize 0 indexes Sketches[-1] (mash.go:117): the reference panics");
    PH_REQUIRE(sx <= 65535 && sy <= 65535, "polyhip_mash_shared_counts: SketchSize > 65535 does not fit the u16 counts");
    PH_REQUIRE(min_shared >= 1, "polyhip_mash_neighbors: min_shared 0 (pairs without a shared hash are never listed)");
    PH_REQUIRE(nx < (1ull << 31) && ny <= (1ull << 31), "polyhip_mash_neighbors: more than 2^31 sketches");
    // the selection is k rounds over a row's candidates on one wave (nbr_assemble_kernel): bounded, so that no call can
    // turn it into a kernel that runs for minutes
    PH_REQUIRE(k <= POLYHIP_MASH_NEIGHBORS_MAX_K, "polyhip_mash_neighbors: k %u is above POLYHIP_MASH_NEIGHBORS_MAX_K (%u)", k,
               (unsigned)POLYHIP_MASH_NEIGHBORS_MAX_K);
    return POLYHIP_OK;
}

extern "C" {

size_t polyhip_mash_neighbors_workspace_bytes(uint64_t nx, uint32_t sx, uint64_t ny, uint32_t sy)
{
    return nbr_layout(nx, sx, ny, std::max<uint32_t>(sy, 1u)).total;
}

int polyhip_mash_neighbors_dev(const uint32_t *d_X, uint64_t nx, uint32_t sx, const uint32_t *d_Y, uint64_t ny, uint32_t sy,
                               uint32_t min_shared, uint32_t k, int exclude_self, uint64_t self_offset, uint64_t *d_first,
                               uint32_t *d_cols, uint16_t *d_shared, double *d_dist, uint64_t capacity, void *d_work,
                               size_t work_bytes, polyhip_stream_t stream)
{
    g_nbr_info = polyhip_neighbors_info{};
    if (int rc = nbr_check_args(nx, sx, ny, sy, min_shared, k))
        return rc;
    PH_REQUIRE(d_first, "polyhip_mash_neighbors: null pointer");
    hipStream_t st = as_stream(stream);
    if (nx == 0 || ny == 0) {
        PH_HIP(hipMemsetAsync(d_first, 0, (nx + 1) * 8, st));
        return POLYHIP_OK;
    }
    PH_REQUIRE(d_X && d_Y && d_work && (d_cols == nullptr) == (d_shared == nullptr) && (d_cols || !d_dist),
               "polyhip_mash_neighbors: null pointer");
    NbrCall c;
    c.dX = d_X, c.dY = d_Y, c.nx = nx, c.ny = ny, c.sx = sx, c.sy = sy, c.min_shared = min_shared, c.k = k;
    c.exclude_self = exclude_self, c.self_offset = self_offset;
    c.d_first = reinterpret_cast<unsigned long long *>(d_first), c.d_cols = d_cols, c.d_shared = d_shared, c.d_dist = d_dist;
    c.capacity = d_cols ? capacity : 0;
    c.w = static_cast<uint8_t *>(d_work);
    c.L = nbr_layout(nx, sx, ny, sy);
    c.g = nbr_geom(sx, sy);
    c.st = st, c.stream = stream;
    PH_REQUIRE(work_bytes >= c.L.total, "polyhip_mash_neighbors: workspace too small (%zu < %zu)", work_bytes, c.L.total);
    uint64_t out_base = 0;
    const int rc = nbr_rows(c, 0, nx, &out_base);
    c.info.column_blocks = (uint32_t)c.L.nblocks;
    c.info.assembly = 1;
    c.info.entries = out_base;
    c.info.devices = 1;
    g_nbr_info = c.info;
    return rc;
}

int polyhip_mash_neighbors_last_info(polyhip_neighbors_info *info)
{
    PH_REQUIRE(info, "polyhip_mash_neighbors_last_info: null pointer");
    *info = g_nbr_info;
    return POLYHIP_OK;
}

} // extern "C"

namespace {
struct NbrShard {
    std::vector<uint64_t> first;
    std::vector<uint32_t> cols;
    std::vector<uint16_t> shared;
    std::vector<double> dist;
    polyhip_neighbors_info info{};
};
} // namespace

// one device: rows of X against all of Y, the list into host vectors (at most `capacity` entries of it)
static int neighbors_one(const uint32_t *X, uint64_t nx, uint32_t sx, const uint32_t *Y, uint64_t ny, uint32_t sy, uint32_t min_shared,
                         uint32_t k, int exclude_self, uint64_t self_offset, bool want_entries, bool want_dist, uint64_t capacity,
                         NbrShard &out)
{
    HostStreams &hs = host_streams();
    PH_HIP(hs.init());
    hipStream_t st = hs.s[0];
    SyncOnExit sync(st);
    DevBuf dX, dY, dW, dF, dC, dS, dD;
    PH_HIP(dX.alloc(nx * (size_t)sx * 4));
    PH_HIP(dY.alloc(ny * (size_t)sy * 4));
    PH_HIP(hipMemcpyAsync(dY.p, Y, ny * (size_t)sy * 4, hipMemcpyHostToDevice, st));
    PH_HIP(hipMemcpyAsync(dX.p, X, nx * (size_t)sx * 4, hipMemcpyHostToDevice, st));
    const size_t wb = polyhip_mash_neighbors_workspace_bytes(nx, sx, ny, sy);
    PH_HIP(dW.alloc(wb));
    PH_HIP(dF.alloc((nx + 1) * 8));
    out.first.assign(nx + 1, 0);
    // device buffers for exactly what the caller can take (never more than there are pairs, or k per row): ONE join per
    // call whatever the capacity; a caller whose buffers were too small reads the true count in first[nx] and repeats
    const unsigned __int128 pairs = (unsigned __int128)nx * ny;
    uint64_t n = want_entries ? (pairs < capacity ? (uint64_t)pairs : capacity) : 0;
    if (k)
        n = std::min<uint64_t>(n, nx * (uint64_t)k);
    if (n) {
        PH_HIP(dC.alloc(n * 4));
        PH_HIP(dS.alloc(n * 2));
        if (want_dist)
            PH_HIP(dD.alloc(n * 8));
    }
    if (int rc = polyhip_mash_neighbors_dev(dX.as<uint32_t>(), nx, sx, dY.as<uint32_t>(), ny, sy, min_shared, k, exclude_self,
                                            self_offset, dF.as<uint64_t>(), n ? dC.as<uint32_t>() : nullptr,
                                            n ? dS.as<uint16_t>() : nullptr, n && want_dist ? dD.as<double>() : nullptr, n, dW.p, wb,
                                            st))
        return rc;
    PH_HIP(hipMemcpyAsync(out.first.data(), dF.p, (nx + 1) * 8, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    (void)polyhip_mash_neighbors_last_info(&out.info);
    n = std::min<uint64_t>(n, out.first[nx]);
    if (n == 0)
        return POLYHIP_OK;
    out.cols.resize(n);
    out.shared.resize(n);
    PH_HIP(hipMemcpyAsync(out.cols.data(), dC.p, n * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(out.shared.data(), dS.p, n * 2, hipMemcpyDeviceToHost, st));
    if (want_dist) {
        out.dist.resize(n);
        PH_HIP(hipMemcpyAsync(out.dist.data(), dD.p, n * 8, hipMemcpyDeviceToHost, st));
    }
    PH_HIP(hipStreamSynchronize(st));
    return POLYHIP_OK;
}

extern "C" {

int polyhip_mash_neighbors(const uint32_t *X, uint64_t nx, uint32_t sx, const uint32_t *Y, uint64_t ny, uint32_t sy,
                           uint32_t min_shared, uint32_t k, int exclude_self, uint64_t self_offset, uint64_t *first, uint32_t *cols,
                           uint16_t *shared, double *dist, uint64_t capacity)
{
    g_nbr_info = polyhip_neighbors_info{};
    if (int rc = nbr_check_args(nx, sx, ny, sy, min_shared, k))
        return rc;
    PH_REQUIRE(first, "polyhip_mash_neighbors: null pointer");
    if (nx == 0 || ny == 0) {
        std::fill(first, first + nx + 1, 0ull);
        return POLYHIP_OK;
    }
    PH_REQUIRE(X && Y && (cols == nullptr) == (shared == nullptr) && (cols || !dist), "polyhip_mash_neighbors: null pointer");
    std::shared_ptr<md::Pool> P = md::pool();
    const size_t nsh = P ? md::size(*P) : 1;
    std::vector<NbrShard> sh(nsh);
    auto r_of = [&](size_t q) { return (uint64_t)(((unsigned __int128)nx * q) / nsh); };
    auto one = [&](size_t q) {
        const uint64_t r0 = r_of(q), r1 = r_of(q + 1);
        if (r0 == r1)
            return (int)POLYHIP_OK;
        // rows of X shard over the devices, every device sees all of Y; a shard cannot know where its entries start in the
        // caller's list, so it may have to return as many as the caller can take
        return neighbors_one(X + r0 * (uint64_t)sx, r1 - r0, sx, Y, ny, sy, min_shared, k, exclude_self, self_offset + r0,
                             cols != nullptr, dist != nullptr, capacity, sh[q]);
    };
    if (int rc = P ? md::run(*P, one) : one(0))
        return rc;
    // the lists concatenate in row order
    polyhip_neighbors_info info{};
    uint64_t base = 0;
    for (size_t q = 0; q < nsh; ++q) {
        const uint64_t r0 = r_of(q), r1 = r_of(q + 1);
        if (r0 == r1)
            continue;
        const NbrShard &s = sh[q];
        for (uint64_t i = 0; i < r1 - r0; ++i)
            first[r0 + i] = base + s.first[i];
        const uint64_t room = base < capacity ? capacity - base : 0, n = std::min<uint64_t>(room, s.cols.size());
        if (cols && n) {
            std::copy(s.cols.begin(), s.cols.begin() + n, cols + base);
            std::copy(s.shared.begin(), s.shared.begin() + n, shared + base);
            if (dist)
                std::copy(s.dist.begin(), s.dist.begin() + n, dist + base);
        }
        base += s.first[r1 - r0];
        info.column_blocks = std::max(info.column_blocks, s.info.column_blocks);
        info.index_builds += s.info.index_builds;
        info.row_chunks += s.info.row_chunks;
        info.entries_thresholded += s.info.entries_thresholded;
        ++info.devices;
    }
    first[nx] = base;
    info.entries = base;
    info.assembly = 1;
    g_nbr_info = info;
    return POLYHIP_OK;
}

} // extern "C"
