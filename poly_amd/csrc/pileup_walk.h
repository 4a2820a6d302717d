// pileup_walk.h -- what polyhip_pileup, polyhip_pileup_qual (pileup.hip), polyhip_pileup_rows (pileup_rows.hip) and
// polyhip_call_variants (variants.hip) share about their entries, each piece once:
//   Entries        the entry arrays as a kernel sees them (and, on the host, as the caller gave them)
//   ColumnWalk     one step of the walk: 64 columns of an entry, one per lane, their classes as 64-bit masks
//   walk_entries   the walk that judges the entries (err) and the one that adds the used ones to the count planes, compiled
//                  once, in pileup_walk.hip: the library is built without relocatable device code, so a kernel is launched
//                  from the unit that defines it
//   check_*, EntryStage   the argument checks the entry points share, in pieces (each entry point has its own checks between
//                  them and keeps its order), and the entry arrays' way to the device
#pragma once
#include "device_prims.h"
#include "pileup_call.h"

namespace polyhip {

enum : int { QINFO_FILTERED = INFO_WORDS, QINFO_WORDS };
constexpr uint32_t MAX_Q = 93;

struct Entries {
    uint64_t n;
    uint32_t min_mapq;
    const uint32_t *flags;
    const uint8_t *mapq; // may be null
    const uint32_t *ref_start, *ref_end, *read_start;
    const uint8_t *alnA, *alnB;
    const uint64_t *alnOff;
    const uint8_t *qual; // null: no qualities
    const uint64_t *qualOff;
    uint32_t *err;
    const uint32_t *order; // null: entry order
};

__device__ __forceinline__ bool entry_used(const Entries &E, uint64_t i)
{
    const uint32_t f = E.flags[i];
    return (f & 1u) && !(E.min_mapq > 0 && E.mapq[i] < E.min_mapq) && E.err[i] == 0;
}

__device__ __forceinline__ uint32_t fold(uint32_t c) { return c >= 'a' && c <= 'z' ? c - 32u : c; }

// The walk is the one of aln_records.hip: a step loads one byte of alnA and one of alnB per lane and turns the classes into
// 64-bit masks with __ballot.  A lane's text position is the entry's running base plus the popcount of the b != '-' mask
// below the lane, its index in the oriented read the same with the a != '-' mask; the anchor of a run that starts at the
// lane is its position minus one, whichever step the column before it sat in, so the only other carry is the class of the
// step's last column.  What a kernel does not read of this (abase and x without qualities, carry without runs) is not computed.
struct ColumnWalk {
    uint64_t tbase; // text position of the next column with b != '-'
    uint64_t abase; // index in the oriented read of the next column with a != '-'
    uint32_t carry; // the column before this step: bit 0 it was I, bit 1 it was D
    // the step: the lane's column, and the wave's columns by class
    bool v, ga, gb;
    uint32_t ca, cb;
    uint64_t mV, mD, mI, mT, mA;
    uint64_t p; // a column with b != '-' sits at p; a run that starts at this lane is anchored at p - 1

    __device__ __forceinline__ ColumnWalk(uint64_t ref_start, uint64_t read_start) : tbase(ref_start), abase(read_start), carry(0) {}

    __device__ __forceinline__ void load(const uint8_t *a, const uint8_t *b, uint32_t base, uint32_t ncols, int lane)
    {
        const uint32_t c = base + lane;
        v = c < ncols;
        ca = v ? a[c] : 0u, cb = v ? b[c] : 0u;
        ga = ca == '-', gb = cb == '-';
        mV = __ballot(v), mD = __ballot(v && ga), mI = __ballot(v && gb), mT = mV & ~mI, mA = mV & ~mD;
        p = tbase + (uint64_t)__popcll(mT & lanes_below(lane));
    }
    __device__ __forceinline__ uint64_t x(int lane) const { return abase + (uint64_t)__popcll(mA & lanes_below(lane)); }
    // the lanes at which an I run, a D run starts
    __device__ __forceinline__ uint64_t sI() const { return mI & ~(mI << 1 | (carry & 1u)); }
    __device__ __forceinline__ uint64_t sD() const { return mD & ~(mD << 1 | (carry >> 1 & 1u)); }
    __device__ __forceinline__ void advance()
    {
        const int nv = __popcll(mV);
        carry = (uint32_t)(mI >> (nv - 1) & 1ull) | (uint32_t)(mD >> (nv - 1) & 1ull) << 1;
        tbase += (uint64_t)__popcll(mT);
        abase += (uint64_t)__popcll(mA);
    }
};

// what a walk takes besides the entries; counts and qsum may be null where nothing adds, min_q and qbase count with qualities
struct WalkArgs {
    uint64_t lo, L, ref_len;
    const uint8_t *ref;
    uint32_t min_q, qbase;
    uint32_t *counts, *qsum;
    unsigned long long *info;
};

// add == false: err[i] is written, info[USED, SKIPPED, BAD, COLUMNS] are added to, counts and qsum are not touched.
// add == true: err[i] is read, the used entries add to counts (and qsum), info[EDGE] (and [FILTERED]) are added to.
// with_qual is the caller's word, not E.qual's: a batch whose quality strings are all empty is still judged with them.
// One wave per entry on grid_for(n, PU_WAVES, PU_MAX_BLOCKS); nothing is launched for n == 0.
hipError_t walk_entries(const Entries &E, const WalkArgs &W, bool add, bool with_qual, hipStream_t st);

// ---- host side: the shared checks, in the order every entry point has them, and the staging ------------------------------
inline int check_region(const char *who, uint64_t lo, uint64_t hi, uint64_t ref_len)
{
    PH_REQUIRE(lo <= hi, "%s: region_lo = %llu is above region_hi = %llu", who, (unsigned long long)lo, (unsigned long long)hi);
    PH_REQUIRE(hi <= ref_len, "%s: region_hi = %llu is above ref_len = %llu", who, (unsigned long long)hi, (unsigned long long)ref_len);
    return POLYHIP_OK;
}

inline int check_qual_offset(const char *who, uint32_t qual_offset)
{
    PH_REQUIRE(qual_offset <= 255u - MAX_Q, "%s: qual_offset = %u, it is 0 to %u", who, qual_offset, 255u - MAX_Q);
    return POLYHIP_OK;
}

inline int check_qual_params(const char *who, uint32_t min_base_qual, uint32_t qual_offset)
{
    PH_REQUIRE(min_base_qual <= MAX_Q, "%s: min_base_qual = %u, it is 0 to %u", who, min_base_qual, MAX_Q);
    return check_qual_offset(who, qual_offset);
}

// H: the caller's host arrays
inline int check_entries(const char *who, const Entries &H, bool with_q)
{
    const uint64_t n = H.n;
    PH_REQUIRE(n == 0 || (H.flags && H.ref_start && H.ref_end && H.alnOff && H.err &&
                          (!with_q || (H.read_start && H.qualOff && (H.qual || H.qualOff[n] == H.qualOff[0]))) &&
                          ((H.alnA && H.alnB) || H.alnOff[n] == H.alnOff[0])),
               "%s: null argument", who);
    for (uint64_t i = 0; i < n; ++i)
        PH_REQUIRE(H.alnOff[i + 1] >= H.alnOff[i] && (!with_q || H.qualOff[i + 1] >= H.qualOff[i]), "%s: offsets are not ascending", who);
    return POLYHIP_OK;
}

// The entry arrays H (the caller's, which outlive the stage), ref and err in the caller's arena: the constructor reserves,
// upload() (after the arena's allocation) issues the copies and gives the device view.  mapq travels only with need_mapq;
// qual, qualOff and read_start only with with_q.  The device copies of the strings start at the first entry's bytes.
struct EntryStage {
    const Entries &H;
    size_t o_flags, o_mapq, o_rs, o_re, o_qs, o_a, o_b, o_off, o_q, o_qoff, o_ref, o_err;
    uint64_t nbytes, qbytes, ref_len;
    bool need_mapq, with_q;

    EntryStage(Arena &w, const Entries &H_, uint64_t ref_len_, bool need_mapq_, bool with_q_)
        : H(H_), ref_len(ref_len_), need_mapq(need_mapq_), with_q(with_q_)
    {
        const uint64_t n = H.n;
        nbytes = n ? H.alnOff[n] - H.alnOff[0] : 0;
        qbytes = with_q && n ? H.qualOff[n] - H.qualOff[0] : 0;
        o_flags = w.reserve(n * 4), o_mapq = w.reserve(need_mapq ? n : 0), o_rs = w.reserve(n * 4), o_re = w.reserve(n * 4);
        o_qs = w.reserve(with_q ? n * 4 : 0), o_a = w.reserve(nbytes), o_b = w.reserve(nbytes), o_off = w.reserve((n + 1) * 8);
        o_q = w.reserve(qbytes), o_qoff = w.reserve(with_q ? (n + 1) * 8 : 0), o_ref = w.reserve(ref_len), o_err = w.reserve(n * 4);
    }
    const uint8_t *ref(const Arena &w) const { return w.at<uint8_t>(o_ref); }
    hipError_t upload(const Arena &w, const uint8_t *host_ref, hipStream_t st, Entries &D) const
    {
        const uint64_t n = H.n;
        const struct {
            size_t at;
            const void *src;
            size_t bytes;
        } in[] = {{o_flags, H.flags, n * 4}, {o_mapq, H.mapq, need_mapq ? n : 0}, {o_rs, H.ref_start, n * 4}, {o_re, H.ref_end, n * 4},
                  {o_qs, H.read_start, with_q ? n * 4 : 0}, {o_a, nbytes ? H.alnA + H.alnOff[0] : nullptr, nbytes},
                  {o_b, nbytes ? H.alnB + H.alnOff[0] : nullptr, nbytes}, {o_off, H.alnOff, n ? (n + 1) * 8 : 0},
                  {o_q, qbytes ? H.qual + H.qualOff[0] : nullptr, qbytes}, {o_qoff, H.qualOff, with_q && n ? (n + 1) * 8 : 0},
                  {o_ref, host_ref, ref_len}};
        for (const auto &x : in)
            if (x.bytes)
                if (hipError_t e = hipMemcpyAsync(w.at<uint8_t>(x.at), x.src, x.bytes, hipMemcpyHostToDevice, st))
                    return e;
        D = Entries{n,
                    H.min_mapq,
                    w.at<uint32_t>(o_flags),
                    need_mapq ? w.at<uint8_t>(o_mapq) : nullptr,
                    w.at<uint32_t>(o_rs),
                    w.at<uint32_t>(o_re),
                    w.at<uint32_t>(o_qs),
                    w.at<uint8_t>(o_a),
                    w.at<uint8_t>(o_b),
                    w.at<uint64_t>(o_off),
                    with_q ? w.at<uint8_t>(o_q) : nullptr,
                    w.at<uint64_t>(o_qoff),
                    w.at<uint32_t>(o_err),
                    nullptr};
        return hipSuccess;
    }
};

} // namespace polyhip
