// dedup.hip -- polyhip_mark_duplicates and polyhip_coord_order: passes over the mapper's arrays that build a key per entry and
// run the library's stable radix sort (device_prims.h) on it.  The definitions are the comments above the two calls in
// include/polyhip.h; tests/dedup_oracle.py restates them in plain Python.
//
//   weight_kernel     (weight_mode 1) one wave per entry over its quality bytes, 64 per step: range check and weight in one pass
//   key_kernel<P>     one lane per entry (per pair with P): err, the end key, the role, lo / hi of a pair, the sort words, and
//                     the smallest and largest value of every word (a wave reduction, one atomic pair per wave and word)
//   sort_words        per word, least significant first: gather_kernel (word - its minimum, through the permutation so far)
//                     and one radix_sort limited to bits_for(the word's range); a word whose range is 0 costs nothing, and
//                     the elements that take no part get one key past the range of the last word, not a bit of their own
//   head_kernel       1 where a sorted element's words, without the weight word, differ from its predecessor's
//   scan_excl         set ids;  set_rep_kernel: the head of each run writes its element to set_rep[id]
//   mark_*_kernel     per sorted element: dup and rep from set_rep[id]
//
// The words of an end set, least significant first: A = fragment << 32 | (2^32 - 1 - w), B = (u + 2^32) << 1 | strand,
// C = (not a candidate) << 32 | rid.  Of a pair set: 2^33 - 1 - W, B of the hi mate, rid of the hi mate, B of the lo mate,
// (not a pair) << 32 | rid of the lo mate.  The sort is stable and starts from the identity, so elements with equal words
// stay in index order: the head of a run is the winner, and no step looks at more than its own element and its neighbour.
#include "device_prims.h"
#include "host_pipeline.h"

namespace polyhip {
namespace {

constexpr int DD_WAVES = BT / 64; // entries a block of the weight kernel walks at a time
constexpr int MAX_WORDS = 5;
// slots of the (min, max) pairs: the end words A, B, C, then the pair words
enum : int { W_A = 0, W_B = 1, W_C = 2, W_P0 = 3, W_P1 = 4, W_P2 = 5, W_P3 = 6, W_P4 = 7, N_SLOTS = 8 };
// the counters behind polyhip_dedup_info, after the 2 * N_SLOTS words of the minima and maxima
enum : int { I_CAND = 0, I_BAD = 1, I_PAIRS = 2, I_FRAGS = 3, I_DUP_PAIRS = 4, I_DUP_FRAGS = 5, N_INFO = 6 };
constexpr uint64_t NOT_IN = 1ull << 32; // in the most significant word: the element takes no part (it sorts last)

struct Words {
    const uint64_t *w[MAX_WORDS]; // least significant first
    int slot[MAX_WORDS];
    int n;
};

__device__ __forceinline__ uint64_t wave_min64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_max64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        v += __shfl_xor(v, d, 64);
    return v;
}

// a thread's running minimum and maximum of one word
struct MinMax {
    uint64_t mn = ~0ull, mx = 0;
    __device__ __forceinline__ void add(uint64_t v)
    {
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    // every lane of the wave calls this; mm[2 * slot] is the minimum, mm[2 * slot + 1] the maximum
    __device__ __forceinline__ void commit(unsigned long long *mm, int slot) const
    {
        const uint64_t a = wave_min64(mn), b = wave_max64(mx);
        if ((threadIdx.x & 63) == 0 && a <= b) {
            atomicMin(&mm[2 * slot], (unsigned long long)a);
            atomicMax(&mm[2 * slot + 1], (unsigned long long)b);
        }
    }
};

__device__ __forceinline__ void add_info(unsigned long long *info, int which, uint64_t mine)
{
    const uint64_t all = wave_sum64(mine);
    if ((threadIdx.x & 63) == 0 && all)
        atomicAdd(&info[which], (unsigned long long)all);
}

// weight_mode 1.  Per mapped entry: qerr = 6 if the quality string is not read_len long, 7 if a byte is out of range, else 0
// and w = the sum of the Q >= minq.  Unmapped entries get 0, 0 and their strings are not read.
__global__ __launch_bounds__(BT) void weight_kernel(uint64_t n, uint32_t minq, uint32_t qoff, const uint32_t *__restrict__ flags,
                                                    const uint32_t *__restrict__ read_len, const uint8_t *__restrict__ qual,
                                                    const uint64_t *__restrict__ qualOff, uint32_t *__restrict__ w,
                                                    uint32_t *__restrict__ qerr)
{
    const int lane = threadIdx.x & 63;
    const uint64_t off0 = qualOff[0]; // the device copy of the strings starts at the first entry's bytes
    for (uint64_t i = (uint64_t)blockIdx.x * DD_WAVES + (threadIdx.x >> 6); i < n; i += (uint64_t)gridDim.x * DD_WAVES) {
        const uint64_t m = qualOff[i + 1] - qualOff[i];
        uint32_t e = 0, sum = 0;
        if (flags[i] & 1u) {
            if (m != (uint64_t)read_len[i]) {
                e = 6;
            } else {
                const uint8_t *q = qual + (qualOff[i] - off0);
                bool bad = false;
                for (uint32_t base = 0; base < (uint32_t)m; base += 64) {
                    const uint32_t c = base + lane;
                    const bool v = c < (uint32_t)m;
                    const uint32_t b = v ? q[c] : qoff;
                    bad |= b < qoff || b > qoff + 93u;
                    const uint32_t Q = b - qoff;
                    sum += v && Q >= minq && Q <= 93u ? Q : 0u;
                }
                if (__ballot(bad))
                    e = 7;
                sum = (uint32_t)__builtin_amdgcn_readlane((int)dpp_incl_scan(sum), 63);
            }
        }
        if (lane == 0) {
            w[i] = e ? 0u : sum;
            qerr[i] = e;
        }
    }
}

struct Judged {
    bool cand;
    uint32_t err, w, rid;
    uint64_t us; // (u + 2^32) << 1 | strand
};

struct EntryArrays {
    const uint32_t *flags, *rid, *ref_start, *ref_end, *read_start, *read_end, *read_len;
};

// err (its quality part, 0 / 6 / 7, comes in through qerr), the weight and the end key of entry i
__device__ __forceinline__ Judged judge(uint64_t i, const EntryArrays &a, const uint32_t *w, const uint32_t *qerr)
{
    Judged j{false, 0, 0, 0, 0};
    const uint32_t f = a.flags[i];
    if (!(f & 1u))
        return j;
    const uint32_t rs = a.read_start[i], re = a.read_end[i], rl = a.read_len[i], fs = a.ref_start[i], fe = a.ref_end[i];
    j.err = (rs > re || re > rl || fs > fe) ? 2u : qerr[i];
    if (j.err)
        return j;
    j.cand = true;
    j.w = w[i];
    j.rid = a.rid ? a.rid[i] : 0u;
    const uint32_t s = f >> 1 & 1u;
    const int64_t u = s ? (int64_t)fe - 1 + (int64_t)(rl - re) : (int64_t)fs - (int64_t)rs;
    j.us = (uint64_t)(u + (int64_t)NOT_IN) << 1 | s;
    return j;
}

// the words of one entry for the end sets, its err and weight, and dup = 0, rep = i until a mark kernel says otherwise
__device__ __forceinline__ void put_entry(uint64_t i, const Judged &j, bool fragment, uint32_t *w, uint32_t *err, uint8_t *dup,
                                          uint32_t *rep, uint64_t *A, uint64_t *B, uint64_t *Cw, MinMax &mA, MinMax &mB, MinMax &mC)
{
    w[i] = j.w;
    err[i] = j.err;
    dup[i] = 0;
    rep[i] = (uint32_t)i;
    const uint64_t a = (fragment ? NOT_IN : 0ull) | (uint64_t)(0xFFFFFFFFu - j.w);
    A[i] = j.cand ? a : 0ull;
    B[i] = j.cand ? j.us : 0ull;
    Cw[i] = j.cand ? (uint64_t)j.rid : NOT_IN;
    if (j.cand) {
        mA.add(a);
        mB.add(j.us);
        mC.add(j.rid);
    }
}

// w and err hold the weights and the quality part of err on entry and the final values afterwards
template <bool PAIRED>
__global__ __launch_bounds__(BT) void key_kernel(uint64_t n, EntryArrays a, uint32_t *w, uint32_t *err, uint8_t *__restrict__ dup,
                                                 uint32_t *__restrict__ rep, uint64_t *__restrict__ A, uint64_t *__restrict__ B,
                                                 uint64_t *__restrict__ Cw, uint64_t *__restrict__ P0, uint64_t *__restrict__ P1,
                                                 uint64_t *__restrict__ P2, uint64_t *__restrict__ P3, uint64_t *__restrict__ P4,
                                                 uint8_t *__restrict__ lo_odd, unsigned long long *mm, unsigned long long *info)
{
    MinMax m[N_SLOTS];
    uint64_t ncand = 0, nbad = 0, npairs = 0, nfrag = 0;
    const uint64_t items = PAIRED ? n / 2 : n;
    for (uint64_t t = (uint64_t)blockIdx.x * BT + threadIdx.x; t < items; t += (uint64_t)gridDim.x * BT) {
        if (!PAIRED) {
            const Judged j = judge(t, a, w, err);
            put_entry(t, j, true, w, err, dup, rep, A, B, Cw, m[W_A], m[W_B], m[W_C]);
            ncand += j.cand;
            nfrag += j.cand;
            nbad += j.err != 0;
        } else {
            const Judged j0 = judge(2 * t, a, w, err), j1 = judge(2 * t + 1, a, w, err);
            const bool pair = j0.cand && j1.cand;
            put_entry(2 * t, j0, !pair, w, err, dup, rep, A, B, Cw, m[W_A], m[W_B], m[W_C]);
            put_entry(2 * t + 1, j1, !pair, w, err, dup, rep, A, B, Cw, m[W_A], m[W_B], m[W_C]);
            ncand += (uint64_t)j0.cand + j1.cand;
            nbad += (uint64_t)(j0.err != 0) + (j1.err != 0);
            npairs += pair;
            nfrag += pair ? 0u : (uint64_t)j0.cand + j1.cand;
            // lo = the mate with the smaller (E, index): mate 1 only when its end is strictly smaller
            const bool odd = pair && (j1.rid < j0.rid || (j1.rid == j0.rid && j1.us < j0.us));
            const Judged &lo = odd ? j1 : j0, &hi = odd ? j0 : j1;
            const uint64_t p0 = 0x1FFFFFFFFull - ((uint64_t)j0.w + j1.w);
            lo_odd[t] = odd ? 1 : 0;
            P0[t] = pair ? p0 : 0ull;
            P1[t] = pair ? hi.us : 0ull;
            P2[t] = pair ? (uint64_t)hi.rid : 0ull;
            P3[t] = pair ? lo.us : 0ull;
            P4[t] = pair ? (uint64_t)lo.rid : NOT_IN;
            if (pair) {
                m[W_P0].add(p0);
                m[W_P1].add(hi.us);
                m[W_P2].add(hi.rid);
                m[W_P3].add(lo.us);
                m[W_P4].add(lo.rid);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < (PAIRED ? N_SLOTS : 3); ++s)
        m[s].commit(mm, s);
    add_info(info, I_CAND, ncand);
    add_info(info, I_BAD, nbad);
    add_info(info, I_PAIRS, npairs);
    add_info(info, I_FRAGS, nfrag);
}

__global__ __launch_bounds__(BT) void iota_kernel(uint64_t n, uint32_t *__restrict__ v)
{
    for (uint64_t j = (uint64_t)blockIdx.x * BT + threadIdx.x; j < n; j += (uint64_t)gridDim.x * BT)
        v[j] = (uint32_t)j;
}

// keys[j] = word[perm[j]] - lo.  An element that took no part in the minimum gets 0 where its word is 0, and cap in the most
// significant word, where it holds NOT_IN: one more than the largest key of those that took part
__global__ __launch_bounds__(BT) void gather_kernel(uint64_t n, const uint64_t *__restrict__ word, const uint32_t *__restrict__ perm,
                                                    uint64_t lo, uint64_t cap, uint64_t *__restrict__ keys)
{
    for (uint64_t j = (uint64_t)blockIdx.x * BT + threadIdx.x; j < n; j += (uint64_t)gridDim.x * BT) {
        const uint64_t v = word[perm[j]];
        const uint64_t k = v >= lo ? v - lo : 0ull;
        keys[j] = k < cap ? k : cap;
    }
}

// head[j] = 1 where sorted element j takes part and starts a run of equal words 1 .. n - 1 (word 0 is the weight)
__global__ __launch_bounds__(BT) void head_kernel(uint64_t n, Words ws, const uint32_t *__restrict__ perm, uint32_t *__restrict__ head)
{
    for (uint64_t j = (uint64_t)blockIdx.x * BT + threadIdx.x; j < n; j += (uint64_t)gridDim.x * BT) {
        const uint32_t x = perm[j];
        uint32_t h = 0;
        if (!(ws.w[ws.n - 1][x] & NOT_IN)) {
            h = j == 0;
            if (j > 0) {
                const uint32_t y = perm[j - 1]; // takes part as well: the others sort last
                for (int q = 1; q < ws.n; ++q)
                    h |= ws.w[q][x] != ws.w[q][y];
            }
        }
        head[j] = h;
    }
}

// sid = the exclusive scan of head: the run of sorted element j is sid[j + 1] - 1
__global__ __launch_bounds__(BT) void set_rep_kernel(uint64_t n, const uint32_t *__restrict__ head, const uint32_t *__restrict__ sid,
                                                     const uint32_t *__restrict__ perm, uint32_t *__restrict__ set_rep)
{
    for (uint64_t j = (uint64_t)blockIdx.x * BT + threadIdx.x; j < n; j += (uint64_t)gridDim.x * BT)
        if (head[j])
            set_rep[sid[j]] = perm[j];
}

// end sets: a fragment that is not the head of its set is a duplicate of the head; pair mates stay as they are
__global__ __launch_bounds__(BT) void mark_ends_kernel(uint64_t n, const uint64_t *__restrict__ A, const uint64_t *__restrict__ Cw,
                                                       const uint32_t *__restrict__ perm, const uint32_t *__restrict__ sid,
                                                       const uint32_t *__restrict__ set_rep, uint8_t *__restrict__ dup,
                                                       uint32_t *__restrict__ rep, unsigned long long *info)
{
    uint64_t ndup = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * BT + threadIdx.x; j < n; j += (uint64_t)gridDim.x * BT) {
        const uint32_t i = perm[j];
        if ((Cw[i] & NOT_IN) || !(A[i] & NOT_IN))
            continue;
        const uint32_t h = set_rep[sid[j + 1] - 1];
        if (h != i) {
            dup[i] = 1;
            rep[i] = h;
            ++ndup;
        }
    }
    add_info(info, I_DUP_FRAGS, ndup);
}

// pair sets: both mates of a pair that is not the head of its set are duplicates, lo of lo and hi of hi
__global__ __launch_bounds__(BT) void mark_pairs_kernel(uint64_t npairs, const uint64_t *__restrict__ P4, const uint8_t *__restrict__ lo_odd,
                                                        const uint32_t *__restrict__ perm, const uint32_t *__restrict__ sid,
                                                        const uint32_t *__restrict__ set_rep, uint8_t *__restrict__ dup,
                                                        uint32_t *__restrict__ rep, unsigned long long *info)
{
    uint64_t ndup = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * BT + threadIdx.x; j < npairs; j += (uint64_t)gridDim.x * BT) {
        const uint32_t p = perm[j];
        if (P4[p] & NOT_IN)
            continue;
        const uint32_t h = set_rep[sid[j + 1] - 1];
        if (h != p) {
            const uint32_t lo = 2 * p + lo_odd[p], hi = lo ^ 1u, hlo = 2 * h + lo_odd[h];
            dup[lo] = 1;
            dup[hi] = 1;
            rep[lo] = hlo;
            rep[hi] = hlo ^ 1u;
            ++ndup;
        }
    }
    add_info(info, I_DUP_PAIRS, ndup);
}

// coord_order: K0 = rid << 32 | ref_start of a placed entry, K1 = 1 for an unplaced one
__global__ __launch_bounds__(BT) void coord_key_kernel(uint64_t n, uint32_t paired, const uint32_t *__restrict__ sam_flag,
                                                       const uint32_t *__restrict__ rid, const uint32_t *__restrict__ ref_start,
                                                       uint64_t *__restrict__ K0, uint64_t *__restrict__ K1, unsigned long long *mm)
{
    MinMax m0, m1;
    for (uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BT) {
        uint64_t at = i;
        bool placed = !(sam_flag[i] & 4u);
        if (!placed && paired) { // n is even
            at = i ^ 1ull;
            placed = !(sam_flag[at] & 4u);
        }
        const uint64_t k = placed ? (uint64_t)(rid ? rid[at] : 0u) << 32 | ref_start[at] : 0ull;
        K0[i] = k;
        K1[i] = placed ? 0ull : 1ull;
        if (placed)
            m0.add(k);
        m1.add(K1[i]);
    }
    m0.commit(mm, 0);
    m1.commit(mm, 1);
}

// the buffers of one sort: (ka, va) and (kb, vb) swap roles, the sorted permutation is va afterwards
struct SortBufs {
    uint64_t *ka, *kb;
    uint32_t *va, *vb, *hist;
    uint8_t *scratch;
};

size_t sort_scratch_bytes(uint64_t N)
{
    return std::max(scan_scratch_bytes<uint32_t>(256 * radix_blocks(N)), scan_scratch_bytes<uint32_t>(N));
}

// the stable order of N elements by their words, least significant first; mm: the minima and maxima of the words of the
// elements that take part, on the host; outsiders: how many take no part (they hold NOT_IN in the last word and sort last)
int sort_words(uint64_t N, const Words &ws, const unsigned long long *mm, uint64_t outsiders, SortBufs &b, hipStream_t st)
{
    const unsigned grid = grid_for(N, BT, 4096);
    hipLaunchKernelGGL(iota_kernel, dim3(grid), dim3(BT), 0, st, N, b.va);
    PH_HIP(hipGetLastError());
    for (int q = 0; q < ws.n; ++q) {
        const uint64_t lo = mm[2 * ws.slot[q]], hi = mm[2 * ws.slot[q] + 1];
        if (hi < lo) // no element takes part
            continue;
        const bool last = q == ws.n - 1 && outsiders > 0;
        if (hi == lo && !last) // one value
            continue;
        const uint64_t top = last ? hi - lo + 1 : hi - lo; // the largest key of this word
        hipLaunchKernelGGL(gather_kernel, dim3(grid), dim3(BT), 0, st, N, ws.w[q], b.va, lo, top, b.ka);
        PH_HIP(hipGetLastError());
        const int rc = radix_sort(b.ka, b.va, b.kb, b.vb, N, bits_for(top), b.hist, b.scratch, st);
        if (rc != POLYHIP_OK)
            return rc;
    }
    return POLYHIP_OK;
}

// head flags, set ids and set_rep of the sorted elements; the number of sets lands in sid[N]
int find_sets(uint64_t N, const Words &ws, const SortBufs &b, uint32_t *head, uint32_t *sid, uint32_t *set_rep, hipStream_t st)
{
    const unsigned grid = grid_for(N, BT, 4096);
    hipLaunchKernelGGL(head_kernel, dim3(grid), dim3(BT), 0, st, N, ws, b.va, head);
    PH_HIP(hipGetLastError());
    PH_HIP(scan_excl<uint32_t>(head, sid, N, b.scratch, st));
    hipLaunchKernelGGL(set_rep_kernel, dim3(grid), dim3(BT), 0, st, N, head, sid, b.va, set_rep);
    PH_HIP(hipGetLastError());
    return POLYHIP_OK;
}

thread_local polyhip_dedup_info t_info{};

} // namespace
} // namespace polyhip

using namespace polyhip;

extern "C" {

int polyhip_mark_duplicates(const polyhip_dedup_params *params, uint64_t n, const uint32_t *flags, const uint32_t *rid,
                            const uint32_t *ref_start, const uint32_t *ref_end, const uint32_t *read_start, const uint32_t *read_end,
                            const uint32_t *read_len, const uint32_t *weight, const uint8_t *qual, const uint64_t *qualOff,
                            uint32_t *weight_out, uint8_t *dup, uint32_t *rep, uint32_t *err)
{
    const char *who = "polyhip_mark_duplicates";
    PH_REQUIRE(params, "%s: null params", who);
    PH_REQUIRE(params->paired <= 1, "%s: paired = %u, it is 0 or 1", who, params->paired);
    PH_REQUIRE(params->weight_mode <= 1, "%s: weight_mode = %u, it is 0 or 1", who, params->weight_mode);
    PH_REQUIRE(params->min_weight_qual <= 93, "%s: min_weight_qual = %u, a quality is 0..93", who, params->min_weight_qual);
    PH_REQUIRE(params->qual_offset <= 162, "%s: qual_offset = %u, qual_offset + 93 must fit a byte", who, params->qual_offset);
    PH_REQUIRE(!params->paired || n % 2 == 0, "%s: paired with %llu entries, mates come in twos", who, (unsigned long long)n);
    if (n >> 32)
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %llu entries, the sort's values are uint32 and hold fewer than 2^32", who,
                         (unsigned long long)n);
    t_info = polyhip_dedup_info{};
    if (n == 0)
        return POLYHIP_OK;
    const bool paired = params->paired, byqual = params->weight_mode == 1;
    PH_REQUIRE(flags && ref_start && ref_end && read_start && read_end && read_len && dup && rep && err &&
                   (!byqual || (qualOff && (qual || qualOff[n] == qualOff[0]))),
               "%s: null argument", who);
    uint64_t nbytes = 0;
    if (byqual) {
        for (uint64_t i = 0; i < n; ++i)
            PH_REQUIRE(qualOff[i + 1] >= qualOff[i], "%s: offsets are not ascending", who);
        for (uint64_t i = 0; i < n; ++i)
            if ((uint64_t)read_len[i] * 93 >> 32)
                return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: entry %llu has %u bases, a weight is uint32 and holds fewer than 2^32 / 93", who,
                                 (unsigned long long)i, read_len[i]);
        nbytes = qualOff[n] - qualOff[0];
    }

    HostStreams &hs = host_streams();
    PH_HIP(hs.init());
    hipStream_t st = hs.s[0];
    const uint64_t np = paired ? n / 2 : 0;
    constexpr size_t n_state = 2 * N_SLOTS + N_INFO;
    Arena w;
    const size_t o_flags = w.reserve(n * 4), o_rid = w.reserve(rid ? n * 4 : 0), o_fs = w.reserve(n * 4), o_fe = w.reserve(n * 4),
                 o_rs = w.reserve(n * 4), o_re = w.reserve(n * 4), o_rl = w.reserve(n * 4), o_w = w.reserve(n * 4),
                 o_err = w.reserve(n * 4), o_dup = w.reserve(n), o_rep = w.reserve(n * 4), o_qual = w.reserve(nbytes),
                 o_qoff = w.reserve(byqual ? (n + 1) * 8 : 0), o_A = w.reserve(n * 8), o_B = w.reserve(n * 8), o_C = w.reserve(n * 8),
                 o_P0 = w.reserve(np * 8), o_P1 = w.reserve(np * 8), o_P2 = w.reserve(np * 8), o_P3 = w.reserve(np * 8),
                 o_P4 = w.reserve(np * 8), o_lo = w.reserve(np), o_ka = w.reserve(n * 8), o_kb = w.reserve(n * 8),
                 o_va = w.reserve(n * 4), o_vb = w.reserve(n * 4), o_hist = w.reserve((256 * radix_blocks(n) + 1) * 4),
                 o_scan = w.reserve(sort_scratch_bytes(n)), o_head = w.reserve(n * 4), o_sid = w.reserve((n + 1) * 4),
                 o_srep = w.reserve(n * 4), o_state = w.reserve(n_state * 8);
    PH_HIP(w.buf.alloc(w.used));
    SyncOnExit sync(st);
    const struct {
        size_t at;
        const void *src;
        size_t bytes;
    } in[] = {{o_flags, flags, n * 4},  {o_rid, rid, rid ? n * 4 : 0}, {o_fs, ref_start, n * 4},
              {o_fe, ref_end, n * 4},   {o_rs, read_start, n * 4},     {o_re, read_end, n * 4},
              {o_rl, read_len, n * 4},  {o_w, weight, !byqual && weight ? n * 4 : 0},
              {o_qual, nbytes ? qual + qualOff[0] : nullptr, nbytes},  {o_qoff, qualOff, byqual ? (n + 1) * 8 : 0}};
    for (const auto &x : in)
        if (x.bytes)
            PH_HIP(hipMemcpyAsync(w.at<uint8_t>(x.at), x.src, x.bytes, hipMemcpyHostToDevice, st));
    unsigned long long state[n_state];
    for (int s = 0; s < N_SLOTS; ++s) {
        state[2 * s] = ~0ull;
        state[2 * s + 1] = 0;
    }
    for (int s = 0; s < N_INFO; ++s)
        state[2 * N_SLOTS + s] = 0;
    PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_state), state, sizeof state, hipMemcpyHostToDevice, st));
    unsigned long long *d_mm = w.at<unsigned long long>(o_state), *d_info = d_mm + 2 * N_SLOTS;

    if (byqual) {
        hipLaunchKernelGGL(weight_kernel, dim3(grid_for(n, DD_WAVES, 1u << 20)), dim3(BT), 0, st, n, params->min_weight_qual,
                           params->qual_offset, w.at<uint32_t>(o_flags), w.at<uint32_t>(o_rl), w.at<uint8_t>(o_qual),
                           w.at<uint64_t>(o_qoff), w.at<uint32_t>(o_w), w.at<uint32_t>(o_err));
        PH_HIP(hipGetLastError());
    } else {
        if (!weight)
            PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_w), 0, n * 4, st));
        PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_err), 0, n * 4, st));
    }
    const EntryArrays ea{w.at<uint32_t>(o_flags), rid ? w.at<uint32_t>(o_rid) : nullptr, w.at<uint32_t>(o_fs), w.at<uint32_t>(o_fe),
                         w.at<uint32_t>(o_rs),    w.at<uint32_t>(o_re),                   w.at<uint32_t>(o_rl)};
    const unsigned kgrid = grid_for(paired ? np : n, BT, 1024);
    if (paired)
        hipLaunchKernelGGL(key_kernel<true>, dim3(kgrid), dim3(BT), 0, st, n, ea, w.at<uint32_t>(o_w), w.at<uint32_t>(o_err),
                           w.at<uint8_t>(o_dup), w.at<uint32_t>(o_rep), w.at<uint64_t>(o_A), w.at<uint64_t>(o_B), w.at<uint64_t>(o_C),
                           w.at<uint64_t>(o_P0), w.at<uint64_t>(o_P1), w.at<uint64_t>(o_P2), w.at<uint64_t>(o_P3), w.at<uint64_t>(o_P4),
                           w.at<uint8_t>(o_lo), d_mm, d_info);
    else
        hipLaunchKernelGGL(key_kernel<false>, dim3(kgrid), dim3(BT), 0, st, n, ea, w.at<uint32_t>(o_w), w.at<uint32_t>(o_err),
                           w.at<uint8_t>(o_dup), w.at<uint32_t>(o_rep), w.at<uint64_t>(o_A), w.at<uint64_t>(o_B), w.at<uint64_t>(o_C),
                           (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr,
                           (uint8_t *)nullptr, d_mm, d_info);
    PH_HIP(hipGetLastError());
    // the words' ranges decide how many passes each sort takes; the counters say whether some element takes no part
    PH_HIP(hipMemcpyAsync(state, d_mm, sizeof state, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    const uint64_t ncand = state[2 * N_SLOTS + I_CAND], npairs = state[2 * N_SLOTS + I_PAIRS];

    SortBufs sb{w.at<uint64_t>(o_ka), w.at<uint64_t>(o_kb), w.at<uint32_t>(o_va), w.at<uint32_t>(o_vb), w.at<uint32_t>(o_hist),
                w.at<uint8_t>(o_scan)};
    uint32_t *head = w.at<uint32_t>(o_head), *sid = w.at<uint32_t>(o_sid), *srep = w.at<uint32_t>(o_srep);
    uint32_t nsets[2] = {0, 0}; // end sets, pair sets
    {
        const Words ws{{w.at<uint64_t>(o_A), w.at<uint64_t>(o_B), w.at<uint64_t>(o_C)}, {W_A, W_B, W_C}, 3};
        int rc = sort_words(n, ws, state, n - ncand, sb, st);
        if (rc == POLYHIP_OK)
            rc = find_sets(n, ws, sb, head, sid, srep, st);
        if (rc != POLYHIP_OK)
            return rc;
        hipLaunchKernelGGL(mark_ends_kernel, dim3(grid_for(n, BT, 1024)), dim3(BT), 0, st, n, w.at<uint64_t>(o_A), w.at<uint64_t>(o_C),
                           sb.va, sid, srep, w.at<uint8_t>(o_dup), w.at<uint32_t>(o_rep), d_info);
        PH_HIP(hipGetLastError());
        PH_HIP(hipMemcpyAsync(&nsets[0], sid + n, 4, hipMemcpyDeviceToHost, st));
    }
    if (paired) {
        const Words ws{{w.at<uint64_t>(o_P0), w.at<uint64_t>(o_P1), w.at<uint64_t>(o_P2), w.at<uint64_t>(o_P3), w.at<uint64_t>(o_P4)},
                       {W_P0, W_P1, W_P2, W_P3, W_P4},
                       5};
        int rc = sort_words(np, ws, state, np - npairs, sb, st);
        if (rc == POLYHIP_OK)
            rc = find_sets(np, ws, sb, head, sid, srep, st);
        if (rc != POLYHIP_OK)
            return rc;
        hipLaunchKernelGGL(mark_pairs_kernel, dim3(grid_for(np, BT, 1024)), dim3(BT), 0, st, np, w.at<uint64_t>(o_P4), w.at<uint8_t>(o_lo),
                           sb.va, sid, srep, w.at<uint8_t>(o_dup), w.at<uint32_t>(o_rep), d_info);
        PH_HIP(hipGetLastError());
        PH_HIP(hipMemcpyAsync(&nsets[1], sid + np, 4, hipMemcpyDeviceToHost, st));
    }
    unsigned long long info[N_INFO];
    PH_HIP(hipMemcpyAsync(dup, w.at<uint8_t>(o_dup), n, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(rep, w.at<uint8_t>(o_rep), n * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(err, w.at<uint8_t>(o_err), n * 4, hipMemcpyDeviceToHost, st));
    if (weight_out)
        PH_HIP(hipMemcpyAsync(weight_out, w.at<uint8_t>(o_w), n * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    t_info = polyhip_dedup_info{n,        info[I_CAND],      info[I_BAD], info[I_PAIRS], info[I_FRAGS], info[I_DUP_PAIRS], info[I_DUP_FRAGS],
                                nsets[1], (uint64_t)nsets[0]};
    return POLYHIP_OK;
}

int polyhip_dedup_last_info(polyhip_dedup_info *info)
{
    PH_REQUIRE(info, "polyhip_dedup_last_info: null argument");
    *info = t_info;
    return POLYHIP_OK;
}

int polyhip_coord_order(uint64_t n, uint32_t paired, const uint32_t *sam_flag, const uint32_t *rid, const uint32_t *ref_start,
                        uint32_t *order)
{
    const char *who = "polyhip_coord_order";
    PH_REQUIRE(paired <= 1, "%s: paired = %u, it is 0 or 1", who, paired);
    PH_REQUIRE(!paired || n % 2 == 0, "%s: paired with %llu entries, mates come in twos", who, (unsigned long long)n);
    if (n >> 32)
        return set_error(POLYHIP_ERR_UNSUPPORTED, "%s: %llu entries, the sort's values are uint32 and hold fewer than 2^32", who,
                         (unsigned long long)n);
    if (n == 0)
        return POLYHIP_OK;
    PH_REQUIRE(sam_flag && ref_start && order, "%s: null argument", who);

    HostStreams &hs = host_streams();
    PH_HIP(hs.init());
    hipStream_t st = hs.s[0];
    Arena w;
    const size_t o_sf = w.reserve(n * 4), o_rid = w.reserve(rid ? n * 4 : 0), o_fs = w.reserve(n * 4), o_K0 = w.reserve(n * 8),
                 o_K1 = w.reserve(n * 8), o_ka = w.reserve(n * 8), o_kb = w.reserve(n * 8), o_va = w.reserve(n * 4),
                 o_vb = w.reserve(n * 4), o_hist = w.reserve((256 * radix_blocks(n) + 1) * 4), o_scan = w.reserve(sort_scratch_bytes(n)),
                 o_mm = w.reserve(4 * 8);
    PH_HIP(w.buf.alloc(w.used));
    SyncOnExit sync(st);
    PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_sf), sam_flag, n * 4, hipMemcpyHostToDevice, st));
    if (rid)
        PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_rid), rid, n * 4, hipMemcpyHostToDevice, st));
    PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_fs), ref_start, n * 4, hipMemcpyHostToDevice, st));
    unsigned long long mm[4] = {~0ull, 0, ~0ull, 0};
    PH_HIP(hipMemcpyAsync(w.at<uint8_t>(o_mm), mm, sizeof mm, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(coord_key_kernel, dim3(grid_for(n, BT, 1024)), dim3(BT), 0, st, n, paired, w.at<uint32_t>(o_sf),
                       rid ? w.at<uint32_t>(o_rid) : (const uint32_t *)nullptr, w.at<uint32_t>(o_fs), w.at<uint64_t>(o_K0),
                       w.at<uint64_t>(o_K1), w.at<unsigned long long>(o_mm));
    PH_HIP(hipGetLastError());
    PH_HIP(hipMemcpyAsync(mm, w.at<uint8_t>(o_mm), sizeof mm, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    SortBufs sb{w.at<uint64_t>(o_ka), w.at<uint64_t>(o_kb), w.at<uint32_t>(o_va), w.at<uint32_t>(o_vb), w.at<uint32_t>(o_hist),
                w.at<uint8_t>(o_scan)};
    const Words ws{{w.at<uint64_t>(o_K0), w.at<uint64_t>(o_K1)}, {0, 1}, 2};
    const int rc = sort_words(n, ws, mm, 0, sb, st);
    if (rc != POLYHIP_OK)
        return rc;
    PH_HIP(hipMemcpyAsync(order, sb.va, n * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    return POLYHIP_OK;
}

} // extern "C"
