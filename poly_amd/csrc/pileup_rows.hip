// pileup_rows.hip -- polyhip_pileup_rows: the mapped reads as the text rows of the six-column pileup format, one row per text
// position, one token and one quality byte per read.  The definition is the comment above polyhip_pileup_rows in
// include/polyhip.h; tests/pileup_rows_oracle.py restates it in plain Python.
//
//   order_kernel          one lane per rank: order[r] < n and seen once, else a flag (the host refuses before anything is written)
//   walk_entries          (pileup_walk.h) err of every entry, exactly as polyhip_pileup (qual == NULL) or polyhip_pileup_qual
//                         (qual != NULL) judge it: the judging walk alone
//   count_kernel          one lane per rank: the tokens of the entry at that rank, |[ref_start, ref_end) ∩ region| for a used
//                         entry (every column with b != '-' is one token, so no walk is needed), and its dropped leading runs
//   scan_excl<uint64>     the first item of every rank; the total goes to the host (more than 2^32 - 1 is refused)
//   item_kernel           one wave per rank, 64 columns per step, the pileup's walk (ColumnWalk): the lane of a column with b != '-' in the
//                         region writes item base[r] + (p - first position): key p - lo, entry, column, the token's byte length
//                         and its quality byte, and adds one to depth[p - lo] (an integer histogram)
//   radix_sort            the items by key, bits_for(L - 1) bits.  The sort is stable and the items stand in rank order, so
//                         within a position they stay in rank order: the key needs no rank field
//   gather_kernel, scan_excl<uint64>   the token lengths in sorted order and their offsets
//   scan_excl<uint32>     depth -> the first sorted item of every position
//   rowsize_kernel        one lane per position: header, token bytes, d quality bytes, tabs, newline; rows and the longest row
//   scan_excl<uint64>     row_off; the total goes to the host, which compares it with the capacity
//   header_kernel         one lane per position: name, position, reference byte, depth, the fixed bytes of the row
//   token_kernel          one lane per sorted item: its token at row_off + header + (its offset within the position) and its
//                         quality byte behind the row's tokens
//
// Where a byte goes is decided by scans and by the stable sort alone; the only atomics are the depth histogram, the order
// check's seen counters (they decide one flag) and the info counters, all integers.  The walk carries nothing about runs
// from step to step: a token owns the I run right behind its column and the D run right behind that (a D column owns a D run
// only behind an I run: D columns that follow it directly continue its own run), so the lane of a column reads ahead
// over its own runs, when it sizes the token and again when it writes it.  Long runs are rare and a lane that copies its
// own run is slow only for that token; they get no wave of their own.
#include "device_prims.h"
#include "host_pipeline.h"
#include "pileup_call.h"
#include "pileup_walk.h"

namespace polyhip {
namespace {

enum : int { RINFO_DROPPED = QINFO_WORDS, RINFO_ROWS, RINFO_MAXROW, RINFO_WORDS };
constexpr uint32_t OUT_OFFSET = 33, MAPQ_TOP = 93;

__device__ __forceinline__ uint32_t dec_digits(uint64_t v)
{
    uint32_t d = 1;
    while (v >= 10) {
        v /= 10;
        ++d;
    }
    return d;
}

// v in decimal, nd = dec_digits(v) bytes; returns the byte behind it
__device__ __forceinline__ uint8_t *put_dec(uint8_t *dst, uint64_t v, uint32_t nd)
{
    for (uint32_t k = nd; k-- > 0;) {
        dst[k] = (uint8_t)('0' + v % 10);
        v /= 10;
    }
    return dst + nd;
}

__device__ __forceinline__ uint8_t letter(uint32_t c, bool reverse) { return (uint8_t)(reverse ? "acgtn" : "ACGTN")[base_class(c)]; }

__global__ __launch_bounds__(BT) void order_kernel(uint64_t n, const uint32_t *__restrict__ order, uint32_t *seen, uint32_t *flag)
{
    for (uint64_t r = (uint64_t)blockIdx.x * BT + threadIdx.x; r < n; r += (uint64_t)gridDim.x * BT) {
        const uint32_t o = order[r];
        if (o >= n || atomicAdd(&seen[o], 1u) != 0)
            atomicOr(flag, 1u);
    }
}

// cnt[r]: tokens of the entry at rank r.  An entry order[r] >= n (the host refuses the call) counts nothing.
__global__ __launch_bounds__(BT) void count_kernel(Entries E, uint64_t lo, uint64_t L, uint64_t *cnt, unsigned long long *info)
{
    const uint64_t off0 = E.n ? E.alnOff[0] : 0;
    for (uint64_t r0 = (uint64_t)blockIdx.x * BT; r0 < E.n; r0 += (uint64_t)gridDim.x * BT) {
        const uint64_t r = r0 + threadIdx.x;
        uint32_t dropped = 0;
        if (r < E.n) {
            const uint64_t i = E.order ? E.order[r] : r;
            uint64_t c = 0;
            if (i < E.n && entry_used(E, i)) {
                const uint64_t from = std::max<uint64_t>(E.ref_start[i], lo), to = std::min<uint64_t>(E.ref_end[i], lo + L);
                c = to > from ? to - from : 0;
                // the runs that open the entry: an I run, a D run, or an I run and the D run behind it
                const uint64_t ncol = E.alnOff[i + 1] - E.alnOff[i];
                const uint8_t *a = E.alnA + (E.alnOff[i] - off0), *b = E.alnB + (E.alnOff[i] - off0);
                if (b[0] == '-') { // a used entry has a column
                    uint64_t k = 1;
                    while (k < ncol && b[k] == '-')
                        ++k;
                    dropped = k < ncol && a[k] == '-' ? 2u : 1u;
                } else if (a[0] == '-') {
                    dropped = 1u;
                }
            }
            cnt[r] = c;
        }
        const uint64_t total = (uint64_t)__popcll(__ballot(dropped >= 1)) + (uint64_t)__popcll(__ballot(dropped == 2));
        if ((threadIdx.x & 63) == 0 && total)
            atomicAdd(&info[RINFO_DROPPED], (unsigned long long)total);
    }
}

// the I run right behind column c and the D run right behind that, which a D column owns only behind an I run
__device__ __forceinline__ void runs_behind(const uint8_t *a, const uint8_t *b, uint32_t c, uint32_t ncols, bool is_d, uint32_t &nI, uint32_t &nD)
{
    uint32_t e = c + 1;
    while (e < ncols && b[e] == '-')
        ++e;
    nI = e - (c + 1);
    nD = 0;
    if (!is_d || nI) {
        const uint32_t e0 = e;
        while (e < ncols && a[e] == '-')
            ++e;
        nD = e - e0;
    }
}

__global__ __launch_bounds__(BT) void item_kernel(Entries E, uint32_t qbase, uint64_t lo, uint64_t L, const uint64_t *__restrict__ first_item,
                                                  uint64_t *key, uint32_t *val, uint32_t *ent, uint32_t *col, uint32_t *len, uint8_t *qb,
                                                  uint32_t *depth)
{
    const int lane = threadIdx.x & 63;
    const uint64_t off0 = E.alnOff[0], qoff0 = E.qual ? E.qualOff[0] : 0;
    for (uint64_t r = (uint64_t)blockIdx.x * PU_WAVES + (threadIdx.x >> 6); r < E.n; r += (uint64_t)gridDim.x * PU_WAVES) {
        const uint64_t t0 = first_item[r];
        if (first_item[r + 1] == t0) // not used, or nothing of it in the region
            continue;
        const uint64_t i = E.order ? E.order[r] : r;
        const uint32_t ncols = (uint32_t)(E.alnOff[i + 1] - E.alnOff[i]);
        const uint64_t rs = E.ref_start[i], re = E.ref_end[i], from = std::max<uint64_t>(rs, lo);
        const uint8_t *a = E.alnA + (E.alnOff[i] - off0), *b = E.alnB + (E.alnOff[i] - off0);
        const bool reverse = E.flags[i] & 2u;
        const uint8_t *q = nullptr;
        uint64_t m = 0, abase = 0, last = 0;
        bool no_read_base = true;
        if (E.qual) {
            q = E.qual + (E.qualOff[i] - qoff0);
            m = E.qualOff[i + 1] - E.qualOff[i];
            abase = E.read_start[i];
            uint64_t nA = 0; // the read bases of the entry: a D column behind the last one borrows its quality
            for (uint32_t base = 0; base < ncols; base += 64) {
                const uint32_t c = base + lane;
                nA += (uint64_t)__popcll(__ballot(c < ncols && a[c] != '-'));
            }
            no_read_base = nA == 0;
            last = abase + nA - 1;
        }
        ColumnWalk S(rs, abase);
        for (uint32_t base = 0; base < ncols; base += 64) {
            S.load(a, b, base, ncols, lane);
            const uint32_t c = base + lane;
            const bool ga = S.ga;
            const uint64_t p = S.p;
            if (S.v && !S.gb && p - lo < L) { // p < lo wraps to a value above L
                const uint64_t t = t0 + (p - from);
                uint32_t nI, nD;
                runs_behind(a, b, c, ncols, ga, nI, nD);
                const uint32_t bytes = (p == rs ? 2u : 0u) + 1u + (nI ? 1u + dec_digits(nI) + nI : 0u) + (nD ? 1u + dec_digits(nD) + nD : 0u) +
                                       (p + 1 == re ? 1u : 0u);
                uint8_t quality = (uint8_t)(MAPQ_TOP + OUT_OFFSET); // '~'
                if (q) { // err[i] == 0: every index below is inside the entry's string, every byte in qbase .. qbase + 93
                    uint64_t x = S.x(lane);
                    if (ga)
                        x = std::min(x, last);
                    quality = ga && no_read_base ? (uint8_t)OUT_OFFSET : (uint8_t)((uint32_t)q[reverse ? m - 1 - x : x] - qbase + OUT_OFFSET);
                }
                key[t] = p - lo;
                val[t] = (uint32_t)t;
                ent[t] = (uint32_t)i;
                col[t] = c;
                len[t] = bytes;
                qb[t] = quality;
                atomicAdd(&depth[p - lo], 1u);
            }
            S.advance();
            if (S.tbase >= lo + L) // the rest of the entry lies behind the region
                break;
        }
    }
}

__global__ __launch_bounds__(BT) void gather_kernel(uint64_t N, const uint32_t *__restrict__ val, const uint32_t *__restrict__ len, uint64_t *slen)
{
    for (uint64_t s = (uint64_t)blockIdx.x * BT + threadIdx.x; s < N; s += (uint64_t)gridDim.x * BT)
        slen[s] = len[val[s]];
}

struct RowShape {
    uint64_t lo, L, pos_origin, name_len;
    uint32_t all_positions;
    const uint32_t *first;  // L + 1: the first sorted item of a position
    const uint64_t *tokoff; // N + 1: the byte offset of a sorted item's token among all tokens
};

// name \t pos \t R \t d \t
__device__ __forceinline__ uint64_t header_bytes(const RowShape &S, uint64_t j, uint32_t d)
{
    return S.name_len + dec_digits(S.lo + j - S.pos_origin + 1) + dec_digits(d) + 5;
}

__global__ __launch_bounds__(BT) void rowsize_kernel(RowShape S, uint64_t *rowlen, unsigned long long *info)
{
    for (uint64_t j0 = (uint64_t)blockIdx.x * BT; j0 < S.L; j0 += (uint64_t)gridDim.x * BT) {
        const uint64_t j = j0 + threadIdx.x;
        uint64_t bytes = 0;
        if (j < S.L) {
            const uint32_t f0 = S.first[j], f1 = S.first[j + 1], d = f1 - f0;
            if (d)
                bytes = header_bytes(S, j, d) + (S.tokoff[f1] - S.tokoff[f0]) + 1 + d + 1;
            else if (S.all_positions)
                bytes = header_bytes(S, j, 0) + 4; // * \t * \n
            rowlen[j] = bytes;
        }
        const uint64_t nrows = (uint64_t)__popcll(__ballot(bytes != 0));
        uint64_t longest = bytes;
#pragma unroll
        for (int dlt = 32; dlt >= 1; dlt >>= 1)
            longest = std::max(longest, (uint64_t)__shfl_xor(longest, dlt, 64));
        if ((threadIdx.x & 63) == 0 && nrows) {
            atomicAdd(&info[RINFO_ROWS], (unsigned long long)nrows);
            atomicMax(&info[RINFO_MAXROW], (unsigned long long)longest);
        }
    }
}

__global__ __launch_bounds__(BT) void header_kernel(RowShape S, const uint64_t *__restrict__ row_off, const uint8_t *__restrict__ name,
                                                    const uint8_t *__restrict__ ref, uint8_t *text)
{
    for (uint64_t j = (uint64_t)blockIdx.x * BT + threadIdx.x; j < S.L; j += (uint64_t)gridDim.x * BT) {
        const uint64_t at = row_off[j], bytes = row_off[j + 1] - at;
        if (bytes == 0)
            continue;
        const uint32_t f0 = S.first[j], f1 = S.first[j + 1], d = f1 - f0;
        uint8_t *w = text + at;
        for (uint64_t k = 0; k < S.name_len; ++k)
            w[k] = name[k];
        w += S.name_len;
        *w++ = '\t';
        const uint64_t pos = S.lo + j - S.pos_origin + 1;
        w = put_dec(w, pos, dec_digits(pos));
        *w++ = '\t';
        const uint32_t rb = ref[S.lo + j];
        *w++ = rb >= 0x21 && rb <= 0x7e ? (uint8_t)rb : (uint8_t)'N';
        *w++ = '\t';
        w = put_dec(w, d, dec_digits(d));
        *w++ = '\t';
        if (d == 0) {
            w[0] = '*';
            w[1] = '\t';
            w[2] = '*';
            w[3] = '\n';
        } else {
            w[S.tokoff[f1] - S.tokoff[f0]] = '\t';
            text[at + bytes - 1] = '\n';
        }
    }
}

__global__ __launch_bounds__(BT) void token_kernel(Entries E, RowShape S, uint64_t N, const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                   const uint32_t *__restrict__ ent, const uint32_t *__restrict__ col,
                                                   const uint8_t *__restrict__ qb, const uint64_t *__restrict__ row_off, uint8_t *text)
{
    const uint64_t off0 = E.alnOff[0];
    for (uint64_t s = (uint64_t)blockIdx.x * BT + threadIdx.x; s < N; s += (uint64_t)gridDim.x * BT) {
        const uint64_t j = key[s];
        const uint32_t t = val[s], i = ent[t], c = col[t];
        const uint32_t f0 = S.first[j], f1 = S.first[j + 1];
        const uint64_t tokens_at = row_off[j] + header_bytes(S, j, f1 - f0);
        uint8_t *w = text + tokens_at + (S.tokoff[s] - S.tokoff[f0]);
        text[tokens_at + (S.tokoff[f1] - S.tokoff[f0]) + 1 + (s - f0)] = qb[t];
        const uint32_t ncols = (uint32_t)(E.alnOff[i + 1] - E.alnOff[i]);
        const uint8_t *a = E.alnA + (E.alnOff[i] - off0), *b = E.alnB + (E.alnOff[i] - off0);
        const bool reverse = E.flags[i] & 2u;
        const uint64_t p = S.lo + j;
        const uint32_t ca = a[c], cb = b[c];
        if (p == E.ref_start[i]) {
            *w++ = '^';
            *w++ = (uint8_t)(std::min<uint32_t>(E.mapq ? E.mapq[i] : 255u, MAPQ_TOP) + OUT_OFFSET);
        }
        *w++ = ca == '-' ? (uint8_t)'*' : fold(ca) == fold(cb) ? (uint8_t)(reverse ? ',' : '.') : letter(ca, reverse);
        uint32_t nI, nD;
        runs_behind(a, b, c, ncols, ca == '-', nI, nD);
        if (nI) {
            *w++ = '+';
            w = put_dec(w, nI, dec_digits(nI));
            for (uint32_t k = 0; k < nI; ++k)
                *w++ = letter(a[c + 1 + k], reverse);
        }
        if (nD) {
            *w++ = '-';
            w = put_dec(w, nD, dec_digits(nD));
            for (uint32_t k = 0; k < nD; ++k)
                *w++ = letter(b[c + 1 + nI + k], reverse);
        }
        if (p + 1 == E.ref_end[i])
            *w = '$';
    }
}

thread_local polyhip_pileup_rows_info t_rinfo{};

} // namespace
} // namespace polyhip

using namespace polyhip;

extern "C" {

int polyhip_pileup_rows(const polyhip_pileup_rows_params *params, uint64_t n, const uint32_t *flags, const uint8_t *mapq,
                        const uint32_t *ref_start, const uint32_t *ref_end, const uint32_t *read_start, const uint8_t *alnA,
                        const uint8_t *alnB, const uint64_t *alnOff, const uint8_t *qual, const uint64_t *qualOff, const uint8_t *ref,
                        uint64_t ref_len, const uint32_t *order, const uint8_t *name, uint64_t name_len, uint64_t *ntext, uint8_t *text,
                        uint64_t text_capacity, uint64_t *row_off, uint32_t *err)
{
    const char *who = "polyhip_pileup_rows";
    PH_REQUIRE(params, "%s: null params", who);
    if (int rc = check_region(who, params->region_lo, params->region_hi, ref_len))
        return rc;
    PH_REQUIRE(params->pos_origin <= params->region_lo, "%s: pos_origin = %llu is above region_lo = %llu", who,
               (unsigned long long)params->pos_origin, (unsigned long long)params->region_lo);
    PH_REQUIRE(params->all_positions <= 1, "%s: all_positions = %u, it is 0 or 1", who, params->all_positions);
    if (int rc = check_qual_offset(who, params->qual_offset))
        return rc;
    PH_REQUIRE(name && name_len, "%s: the name is null or empty", who);
    for (uint64_t k = 0; k < name_len; ++k)
        PH_REQUIRE(name[k] >= 0x21 && name[k] <= 0x7e, "%s: byte %llu of the name is 0x%02x, outside 0x21..0x7e", who, (unsigned long long)k,
                   (unsigned)name[k]);
    if (n >> 32)
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %llu entries, order is uint32 and names fewer than 2^32", who, (unsigned long long)n);
    PH_REQUIRE(params->min_mapq == 0 || mapq, "%s: min_mapq = %u needs mapq, which is null", who, params->min_mapq);
    const uint64_t lo = params->region_lo, L = params->region_hi - params->region_lo;
    PH_REQUIRE(ref && ntext && (text || text_capacity == 0), "%s: null argument", who);
    const Entries H{n, params->min_mapq, flags, mapq, ref_start, ref_end, read_start, alnA, alnB, alnOff, qual, qualOff, err, order};
    if (int rc = check_entries(who, H, qual != nullptr))
        return rc;
    const bool with_q = qual != nullptr && n > 0;
    t_rinfo = polyhip_pileup_rows_info{};

    HostStreams &hs = host_streams();
    PH_HIP(hs.init());
    hipStream_t st = hs.s[0];
    Arena w;
    const EntryStage stage(w, H, ref_len, mapq != nullptr, with_q); // mapq whenever it is given: the tokens print it
    const size_t o_order = w.reserve(order ? n * 4 : 0), o_seen = w.reserve(order ? n * 4 : 0), o_name = w.reserve(name_len),
                 o_cnt = w.reserve((n + 1) * 8), o_info = w.reserve((RINFO_WORDS + 1) * sizeof(unsigned long long)),
                 o_scan = w.reserve(scan_scratch_bytes<uint64_t>(n));
    PH_HIP(w.buf.alloc(w.used));
    SyncOnExit sync(st);
    Entries E;
    PH_HIP(stage.upload(w, ref, st, E));
    if (order && n) {
        PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_order), order, n * 4, hipMemcpyHostToDevice, st));
        E.order = w.at<uint32_t>(o_order);
    }
    PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_name), name, name_len, hipMemcpyHostToDevice, st));
    // the info words and, behind them, the word the order check raises
    PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_info), 0, (RINFO_WORDS + 1) * sizeof(unsigned long long), st));
    unsigned long long *d_info = w.at<unsigned long long>(o_info);
    uint32_t *d_flag = reinterpret_cast<uint32_t *>(d_info + RINFO_WORDS);
    if (n) {
        if (order) {
            PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_seen), 0, n * 4, st));
            hipLaunchKernelGGL(order_kernel, dim3(grid_for(n)), dim3(BT), 0, st, n, w.at<uint32_t>(o_order), w.at<uint32_t>(o_seen), d_flag);
            PH_HIP(hipGetLastError());
        }
        PH_HIP(walk_entries(E, WalkArgs{lo, L, ref_len, stage.ref(w), 0u, params->qual_offset, nullptr, nullptr, d_info}, false, with_q, st));
        hipLaunchKernelGGL(count_kernel, dim3(grid_for(n)), dim3(BT), 0, st, E, lo, L, w.at<uint64_t>(o_cnt), d_info);
        PH_HIP(hipGetLastError());
    }
    PH_HIP(scan_excl<uint64_t>(w.at<uint64_t>(o_cnt), w.at<uint64_t>(o_cnt), n, w.at<uint8_t>(o_scan), st));
    unsigned long long info[RINFO_WORDS + 1];
    uint64_t N = 0;
    PH_HIP(hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(&N, w.at<uint64_t>(o_cnt) + n, sizeof N, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    PH_REQUIRE((uint32_t)info[RINFO_WORDS] == 0, "%s: order is not a permutation of 0..%llu", who, (unsigned long long)(n ? n - 1 : 0));
    *ntext = 0;
    if (n) {
        PH_HIP(hipMemcpyAsync(err, E.err, n * 4, hipMemcpyDeviceToHost, st));
        PH_HIP(hipStreamSynchronize(st));
    }
    t_rinfo.entries = n;
    t_rinfo.used = info[INFO_USED];
    t_rinfo.skipped_mapq = info[INFO_SKIPPED];
    t_rinfo.bad = info[INFO_BAD];
    t_rinfo.columns = info[INFO_COLUMNS];
    t_rinfo.dropped_events = info[RINFO_DROPPED];
    if (N > 0xFFFFFFFFull)
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %llu tokens, one call holds at most 2^32 - 1: split the region", who, (unsigned long long)N);
    t_rinfo.tokens = N;
    if (L == 0) {
        if (row_off)
            row_off[0] = 0;
        return POLYHIP_OK;
    }

    // the items, their sort and the row sizes
    const uint64_t nb = radix_blocks(N);
    Arena x;
    const size_t o_ka = x.reserve(N * 8), o_kb = x.reserve(N * 8), o_va = x.reserve(N * 4), o_vb = x.reserve(N * 4), o_ent = x.reserve(N * 4),
                 o_col = x.reserve(N * 4), o_len = x.reserve(N * 4), o_qb = x.reserve(N), o_hist = x.reserve((256 * nb + 1) * 4),
                 o_rscan = x.reserve(scan_scratch_bytes<uint32_t>(256 * nb)), o_tok = x.reserve((N + 1) * 8),
                 o_tscan = x.reserve(scan_scratch_bytes<uint64_t>(N)), o_depth = x.reserve((L + 1) * 4),
                 o_dscan = x.reserve(scan_scratch_bytes<uint32_t>(L)), o_row = x.reserve((L + 1) * 8),
                 o_wscan = x.reserve(scan_scratch_bytes<uint64_t>(L));
    PH_HIP(x.buf.alloc(x.used));
    SyncOnExit sync_items(st); // an early return frees x only after its kernels
    uint64_t *ka = x.at<uint64_t>(o_ka), *kb = x.at<uint64_t>(o_kb);
    uint32_t *va = x.at<uint32_t>(o_va), *vb = x.at<uint32_t>(o_vb);
    PH_HIP(hipMemsetAsync(x.at<uint8_t>(o_depth), 0, (L + 1) * 4, st));
    if (N) {
        hipLaunchKernelGGL(item_kernel, dim3(grid_for(n, PU_WAVES, PU_MAX_BLOCKS)), dim3(BT), 0, st, E, params->qual_offset, lo, L,
                           w.at<uint64_t>(o_cnt), ka, va, x.at<uint32_t>(o_ent), x.at<uint32_t>(o_col), x.at<uint32_t>(o_len),
                           x.at<uint8_t>(o_qb), x.at<uint32_t>(o_depth));
        PH_HIP(hipGetLastError());
        const int rc = radix_sort(ka, va, kb, vb, N, bits_for(L - 1), x.at<uint32_t>(o_hist), x.at<uint8_t>(o_rscan), st);
        if (rc != POLYHIP_OK)
            return rc;
        hipLaunchKernelGGL(gather_kernel, dim3(grid_for(N, BT, 1u << 20)), dim3(BT), 0, st, N, va, x.at<uint32_t>(o_len), x.at<uint64_t>(o_tok));
        PH_HIP(hipGetLastError());
    }
    PH_HIP(scan_excl<uint64_t>(x.at<uint64_t>(o_tok), x.at<uint64_t>(o_tok), N, x.at<uint8_t>(o_tscan), st));
    PH_HIP(scan_excl<uint32_t>(x.at<uint32_t>(o_depth), x.at<uint32_t>(o_depth), L, x.at<uint8_t>(o_dscan), st));
    const RowShape S{lo, L, params->pos_origin, name_len, params->all_positions, x.at<uint32_t>(o_depth), x.at<uint64_t>(o_tok)};
    const unsigned lgrid = grid_for(L, BT, 1u << 20);
    hipLaunchKernelGGL(rowsize_kernel, dim3(lgrid), dim3(BT), 0, st, S, x.at<uint64_t>(o_row), d_info);
    PH_HIP(hipGetLastError());
    PH_HIP(scan_excl<uint64_t>(x.at<uint64_t>(o_row), x.at<uint64_t>(o_row), L, x.at<uint8_t>(o_wscan), st));
    uint64_t total = 0;
    if (row_off)
        PH_HIP(hipMemcpyAsync(row_off, x.at<uint8_t>(o_row), (L + 1) * 8, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(&total, x.at<uint64_t>(o_row) + L, sizeof total, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    *ntext = total;
    t_rinfo.rows = info[RINFO_ROWS];
    t_rinfo.max_row_bytes = info[RINFO_MAXROW];
    t_rinfo.text_bytes = total;
    if (total > text_capacity)
        return set_error(POLYHIP_ERR_INVALID, "%s: the text needs %llu bytes, the buffer holds %llu", who, (unsigned long long)total,
                         (unsigned long long)text_capacity);
    if (total == 0)
        return POLYHIP_OK;
    // only now, bounded by the caller's capacity: the text itself
    DevBuf dtext;
    PH_HIP(dtext.alloc(total));
    SyncOnExit sync_text(st);
    hipLaunchKernelGGL(header_kernel, dim3(lgrid), dim3(BT), 0, st, S, x.at<uint64_t>(o_row), w.at<uint8_t>(o_name), stage.ref(w),
                       dtext.as<uint8_t>());
    PH_HIP(hipGetLastError());
    if (N) {
        hipLaunchKernelGGL(token_kernel, dim3(grid_for(N, BT, 1u << 20)), dim3(BT), 0, st, E, S, N, ka, va, x.at<uint32_t>(o_ent),
                           x.at<uint32_t>(o_col), x.at<uint8_t>(o_qb), x.at<uint64_t>(o_row), dtext.as<uint8_t>());
        PH_HIP(hipGetLastError());
    }
    PH_HIP(hipMemcpyAsync(text, dtext.p, total, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    return POLYHIP_OK;
}

int polyhip_pileup_rows_last_info(polyhip_pileup_rows_info *info)
{
    PH_REQUIRE(info, "polyhip_pileup_rows_last_info: null argument");
    *info = t_rinfo;
    return POLYHIP_OK;
}

} // extern "C"
