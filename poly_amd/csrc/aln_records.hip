// aln_records.hip -- polyhip_aln_records: the mapper's aligned strings as CIGAR, NM, MD, MAPQ and SAM FLAG.  The definition is
// the comment above polyhip_aln_records in include/polyhip.h; tests/aln_records_oracle.py restates it in plain Python.
//
//   records_kernel<false>  one wave per entry, 64 columns per step: err, nm, CIGAR entries and MD bytes of the entry
//   scan_excl x 2          cigar_off, md_off (uint64, in place); the totals come back to the host with the per-entry arrays
//   finish_kernel          one lane per entry: mapq, sam_flag (the mate's err is known by now), the info counters
//   records_kernel<true>   the same walk, writing the CIGAR entries and the MD bytes at the scanned offsets
//
// The walk: a step loads one byte of alnA and one of alnB per lane (coalesced) and turns the column classes into 64-bit
// masks with __ballot.  A run starts where a class mask has a bit its own left shift lacks (the last class of the step
// before is carried into bit 0), so the runs of a step, their lengths and their output slots are popcounts and leading-zero
// counts of wave-uniform masks; only the MD bytes, whose decimal widths differ per lane, take a wave scan.  No LDS.
#include "device_prims.h"
#include "host_pipeline.h"

namespace polyhip {
namespace {

constexpr int AR_WAVES = BT / 64; // entries a block walks at a time
enum : uint32_t { OP_M = 0, OP_I = 1, OP_D = 2, OP_S = 4, OP_EQ = 7, OP_X = 8 };

__device__ __forceinline__ uint32_t dec_width(uint32_t k)
{
    return 1u + (k >= 10u) + (k >= 100u) + (k >= 1000u) + (k >= 10000u) + (k >= 100000u) + (k >= 1000000u) + (k >= 10000000u) +
           (k >= 100000000u);
}

__device__ __forceinline__ void put_dec(uint8_t *p, uint32_t k, uint32_t w)
{
    for (uint32_t j = w; j-- > 0;) {
        p[j] = (uint8_t)('0' + k % 10u);
        k /= 10u;
    }
}

__device__ __forceinline__ uint32_t wave_total(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)dpp_incl_scan(v), 63); }

// EMIT == false: ncig / nmd (uint64, n + 1 slots for the scans), nm and err are written, cigar / md are not touched.
// EMIT == true: err, ncig (now cigar_off) and nmd (now md_off) are read, the live entries' CIGAR and MD are written.
template <bool EMIT>
__global__ __launch_bounds__(BT) void records_kernel(uint64_t n, uint32_t eqx, const uint32_t *__restrict__ flags,
                                                     const uint32_t *__restrict__ read_start, const uint32_t *__restrict__ read_end,
                                                     const uint32_t *__restrict__ read_len, const uint8_t *__restrict__ alnA,
                                                     const uint8_t *__restrict__ alnB, const uint64_t *__restrict__ alnOff, uint64_t *ncig,
                                                     uint64_t *nmd, uint32_t *nm, uint32_t *err, uint32_t *__restrict__ cigar,
                                                     uint8_t *__restrict__ md)
{
    const int lane = threadIdx.x & 63;
    const uint64_t off0 = alnOff[0]; // the device copy of the strings starts at the first entry's columns
    for (uint64_t i = (uint64_t)blockIdx.x * AR_WAVES + (threadIdx.x >> 6); i < n; i += (uint64_t)gridDim.x * AR_WAVES) {
        const bool mapped = flags[i] & 1u;
        const uint64_t ncol = alnOff[i + 1] - alnOff[i];
        if (!EMIT && (!mapped || ncol > POLYHIP_ALN_MAX_COLUMNS)) {
            if (lane == 0) {
                ncig[i] = 0;
                nmd[i] = 0;
                nm[i] = 0;
                err[i] = mapped ? 4u : 0u;
            }
            continue;
        }
        if (EMIT && (!mapped || err[i] != 0))
            continue;
        const uint32_t L = (uint32_t)ncol, rs = read_start[i], re = read_end[i], rl = read_len[i];
        const uint8_t *a = alnA + (alnOff[i] - off0), *b = alnB + (alnOff[i] - off0);
        const uint32_t slot0 = rs > 0 ? 1u : 0u;
        uint32_t *cg = EMIT ? cigar + ncig[i] : nullptr;
        uint8_t *mp = EMIT ? md + nmd[i] : nullptr;
        if (EMIT && lane == 0 && rs > 0)
            cg[0] = rs << 4 | OP_S;
        uint32_t carry = 0;                           // one-hot class (M or '=', X, I, D) of the column before this step
        uint32_t runs = 0, open_len = 0, open_op = 0; // CIGAR: runs started so far; the last of them up to this step
        uint32_t k = 0;                               // MD: '=' columns since the last X or deletion start
        uint32_t nongap = 0, edits = 0, bytes = 0;    // bytes: per lane when sizing, the entry's running offset when emitting
        bool invalid = false;
        for (uint32_t base = 0; base < L; base += 64) {
            const uint32_t c = base + lane;
            const bool v = c < L;
            const uint32_t ca = v ? a[c] : 0u, cb = v ? b[c] : 0u;
            const bool ga = ca == '-', gb = cb == '-';
            const uint64_t mV = __ballot(v), mBad = __ballot(v && ga && gb);
            if (mBad) {
                invalid = true;
                break;
            }
            const uint64_t mD = __ballot(v && ga), mI = __ballot(v && gb), mE = __ballot(v && !ga && !gb && ca == cb);
            const uint64_t mX = mV & ~(mD | mI | mE);
            const uint64_t m0 = eqx ? mE : mE | mX, m1 = eqx ? mX : 0ull;
            const uint64_t sD = mD & ~(mD << 1 | (carry >> 3 & 1u));
            const uint64_t S = (m0 & ~(m0 << 1 | (carry & 1u))) | (m1 & ~(m1 << 1 | (carry >> 1 & 1u))) |
                               (mI & ~(mI << 1 | (carry >> 2 & 1u))) | sD;
            auto op_at = [&](int p) -> uint32_t {
                return (m0 >> p & 1ull) ? (eqx ? OP_EQ : OP_M) : (m1 >> p & 1ull) ? OP_X : (mI >> p & 1ull) ? OP_I : OP_D;
            };
            const int nv = __popcll(mV);
            // ---- CIGAR: the lane where a run starts writes the run that ends before it
            if (EMIT && (S >> lane & 1ull)) {
                const uint64_t below = S & lanes_below(lane);
                const uint32_t len = below ? (uint32_t)(lane - top_bit(below)) : open_len + (uint32_t)lane;
                const uint32_t op = below ? op_at(top_bit(below)) : open_op;
                if (len)
                    cg[slot0 + runs + __popcll(below) - 1] = len << 4 | op;
            }
            if (S) {
                open_op = op_at(top_bit(S));
                open_len = (uint32_t)(nv - top_bit(S));
            } else {
                open_len += (uint32_t)nv;
            }
            runs += __popcll(S);
            carry = (uint32_t)(m0 >> (nv - 1) & 1ull) | (uint32_t)(m1 >> (nv - 1) & 1ull) << 1 | (uint32_t)(mI >> (nv - 1) & 1ull) << 2 |
                    (uint32_t)(mD >> (nv - 1) & 1ull) << 3;
            // ---- MD: X columns and deletion starts write the counter; its value is the '=' columns since the one before
            const uint64_t K = mX | sD;
            const bool writes_k = K >> lane & 1ull, starts_d = sD >> lane & 1ull, is_d = mD >> lane & 1ull;
            uint32_t kk = 0, nb = is_d ? 1u : 0u;
            if (writes_k) {
                const uint64_t below = K & lanes_below(lane), eq = mE & lanes_below(lane);
                kk = below ? (uint32_t)__popcll(eq >> top_bit(below) >> 1) : k + (uint32_t)__popcll(eq);
                nb = dec_width(kk) + 1u + (starts_d ? 1u : 0u);
            }
            if (EMIT) {
                const uint32_t incl = dpp_incl_scan(nb);
                uint8_t *p = mp + bytes + (incl - nb);
                if (writes_k) {
                    const uint32_t w = dec_width(kk);
                    put_dec(p, kk, w);
                    p += w;
                    if (starts_d)
                        *p++ = '^';
                    *p = (uint8_t)cb;
                } else if (is_d) {
                    *p = (uint8_t)cb;
                }
                bytes += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            } else {
                bytes += nb;
            }
            k = K ? (uint32_t)__popcll(mE >> top_bit(K) >> 1) : k + (uint32_t)__popcll(mE);
            nongap += (uint32_t)__popcll(mV & ~mD);
            edits += (uint32_t)__popcll(mX | mI | mD);
        }
        if (EMIT) {
            if (lane == 0) {
                if (open_len)
                    cg[slot0 + runs - 1] = open_len << 4 | open_op;
                if (rl > re)
                    cg[slot0 + runs] = (rl - re) << 4 | OP_S;
                put_dec(mp + bytes, k, dec_width(k));
            }
        } else {
            const uint32_t e = invalid ? 1u : (rs > re || re > rl || nongap != re - rs) ? 2u : L == 0 ? 3u : 0u;
            const uint32_t total = wave_total(bytes) + dec_width(k);
            if (lane == 0) {
                ncig[i] = e ? 0u : slot0 + runs + (rl > re ? 1u : 0u);
                nmd[i] = e ? 0u : total;
                nm[i] = e ? 0u : edits;
                err[i] = e;
            }
        }
    }
}

// one lane per entry, once every err is known: mapq, sam_flag, and info[0..2] += live entries, their columns, entries with err
__global__ __launch_bounds__(BT) void finish_kernel(uint64_t n, uint32_t paired, const uint32_t *__restrict__ flags,
                                                    const int64_t *__restrict__ score, const int64_t *__restrict__ second,
                                                    const uint64_t *__restrict__ alnOff, const uint32_t *__restrict__ err,
                                                    uint8_t *__restrict__ mapq, uint32_t *__restrict__ sam_flag,
                                                    unsigned long long *__restrict__ info)
{
    const int lane = threadIdx.x & 63;
    uint64_t nlive = 0, cols = 0, nbad = 0; // this lane's share; the grid is small, so a wave adds to info once
    for (uint64_t i = (uint64_t)blockIdx.x * BT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BT) {
        const uint32_t f = flags[i], e = err[i];
        const bool live = (f & 1u) && e == 0;
        {
            uint32_t q = 0, sf = live ? (f & 2u ? 0x10u : 0u) : 0x4u;
            if (live) {
                const int64_t s = score[i], t = second[i] > 0 ? second[i] : 0;
                if (t < s) {
                    const int64_t r = 60 * (s - t) / s;
                    q = r < 60 ? (uint32_t)r : 60u;
                }
            }
            if (paired) {
                const uint64_t m = i ^ 1ull; // n is even
                const uint32_t fm = flags[m];
                const bool mlive = (fm & 1u) && err[m] == 0;
                sf |= 0x1u | (i & 1ull ? 0x80u : 0x40u);
                if ((f & 4u) && live && mlive)
                    sf |= 0x2u;
                if (!mlive)
                    sf |= 0x8u;
                else if (fm & 2u)
                    sf |= 0x20u;
            }
            mapq[i] = (uint8_t)q;
            sam_flag[i] = sf;
        }
        nlive += live ? 1u : 0u;
        cols += live ? alnOff[i + 1] - alnOff[i] : (uint64_t)0;
        nbad += e != 0 ? 1u : 0u;
    }
    nlive = wave_incl_scan(nlive);
    cols = wave_incl_scan(cols);
    nbad = wave_incl_scan(nbad);
    if (lane == 63) {
        if (nlive) {
            atomicAdd(&info[0], (unsigned long long)nlive);
            atomicAdd(&info[1], (unsigned long long)cols);
        }
        if (nbad)
            atomicAdd(&info[2], (unsigned long long)nbad);
    }
}

thread_local polyhip_aln_records_info t_info{};

} // namespace
} // namespace polyhip

using namespace polyhip;

extern "C" {

int polyhip_aln_records(const polyhip_aln_records_params *params, uint64_t n, const uint32_t *flags, const int64_t *score,
                        const int64_t *second, const uint32_t *read_start, const uint32_t *read_end, const uint32_t *read_len,
                        const uint8_t *alnA, const uint8_t *alnB, const uint64_t *alnOff, uint64_t *cigar_off, uint32_t *cigar,
                        uint64_t cigar_capacity, uint64_t *md_off, uint8_t *md, uint64_t md_capacity, uint32_t *nm, uint8_t *mapq,
                        uint32_t *sam_flag, uint32_t *err)
{
    const char *who = "polyhip_aln_records";
    PH_REQUIRE(params, "%s: null params", who);
    PH_REQUIRE(params->eqx <= 1, "%s: eqx = %u, it is 0 or 1", who, params->eqx);
    PH_REQUIRE(params->paired <= 1, "%s: paired = %u, it is 0 or 1", who, params->paired);
    PH_REQUIRE(!params->paired || n % 2 == 0, "%s: paired with %llu entries, mates come in twos", who, (unsigned long long)n);
    t_info = polyhip_aln_records_info{};
    if (n == 0) {
        if (cigar_off)
            cigar_off[0] = 0;
        if (md_off)
            md_off[0] = 0;
        return POLYHIP_OK;
    }
    PH_REQUIRE(flags && score && second && read_start && read_end && read_len && alnOff && cigar_off && md_off && nm && mapq &&
                   sam_flag && err && ((alnA && alnB) || alnOff[n] == alnOff[0]),
               "%s: null argument", who);
    PH_REQUIRE((cigar || cigar_capacity == 0) && (md || md_capacity == 0), "%s: null output with a capacity", who);
    for (uint64_t i = 0; i < n; ++i)
        PH_REQUIRE(alnOff[i + 1] >= alnOff[i], "%s: offsets are not ascending", who);
    const uint64_t nbytes = alnOff[n] - alnOff[0];

    HostStreams &hs = host_streams();
    PH_HIP(hs.init());
    hipStream_t st = hs.s[0];
    Arena w;
    const size_t o_flags = w.reserve(n * 4), o_score = w.reserve(n * 8), o_second = w.reserve(n * 8), o_rs = w.reserve(n * 4),
                 o_re = w.reserve(n * 4), o_rl = w.reserve(n * 4), o_a = w.reserve(nbytes), o_b = w.reserve(nbytes),
                 o_off = w.reserve((n + 1) * 8), o_coff = w.reserve((n + 1) * 8), o_moff = w.reserve((n + 1) * 8),
                 o_nm = w.reserve(n * 4), o_err = w.reserve(n * 4), o_sf = w.reserve(n * 4), o_mapq = w.reserve(n),
                 o_info = w.reserve(3 * sizeof(unsigned long long)), o_scan = w.reserve(scan_scratch_bytes<uint64_t>(n));
    PH_HIP(w.buf.alloc(w.used));
    SyncOnExit sync(st);
    const struct {
        size_t at;
        const void *src;
        size_t bytes;
    } in[] = {{o_flags, flags, n * 4}, {o_score, score, n * 8},   {o_second, second, n * 8}, {o_rs, read_start, n * 4}, {o_re, read_end, n * 4},
              {o_rl, read_len, n * 4}, {o_a, alnA + (nbytes ? alnOff[0] : 0), nbytes}, {o_b, alnB + (nbytes ? alnOff[0] : 0), nbytes},
              {o_off, alnOff, (n + 1) * 8}};
    for (const auto &x : in)
        if (x.bytes)
            PH_HIP(hipMemcpyAsync(w.at<uint8_t>(x.at), x.src, x.bytes, hipMemcpyHostToDevice, st));
    PH_HIP(hipMemsetAsync(w.at<uint8_t>(o_info), 0, 3 * sizeof(unsigned long long), st));

    const unsigned wgrid = grid_for(n, AR_WAVES, 1u << 20);
    hipLaunchKernelGGL(records_kernel<false>, dim3(wgrid), dim3(BT), 0, st, n, params->eqx, w.at<uint32_t>(o_flags), w.at<uint32_t>(o_rs),
                       w.at<uint32_t>(o_re), w.at<uint32_t>(o_rl), w.at<uint8_t>(o_a), w.at<uint8_t>(o_b), w.at<uint64_t>(o_off),
                       w.at<uint64_t>(o_coff), w.at<uint64_t>(o_moff), w.at<uint32_t>(o_nm), w.at<uint32_t>(o_err), (uint32_t *)nullptr,
                       (uint8_t *)nullptr);
    PH_HIP(hipGetLastError());
    PH_HIP(scan_excl<uint64_t>(w.at<uint64_t>(o_coff), w.at<uint64_t>(o_coff), n, w.at<uint8_t>(o_scan), st));
    PH_HIP(scan_excl<uint64_t>(w.at<uint64_t>(o_moff), w.at<uint64_t>(o_moff), n, w.at<uint8_t>(o_scan), st));
    hipLaunchKernelGGL(finish_kernel, dim3(grid_for(n, BT, 1024)), dim3(BT), 0, st, n, params->paired, w.at<uint32_t>(o_flags),
                       w.at<int64_t>(o_score), w.at<int64_t>(o_second), w.at<uint64_t>(o_off), w.at<uint32_t>(o_err), w.at<uint8_t>(o_mapq),
                       w.at<uint32_t>(o_sf), w.at<unsigned long long>(o_info));
    PH_HIP(hipGetLastError());
    unsigned long long info[3];
    PH_HIP(hipMemcpyAsync(cigar_off, w.at<uint8_t>(o_coff), (n + 1) * 8, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(md_off, w.at<uint8_t>(o_moff), (n + 1) * 8, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(nm, w.at<uint8_t>(o_nm), n * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(err, w.at<uint8_t>(o_err), n * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(sam_flag, w.at<uint8_t>(o_sf), n * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(mapq, w.at<uint8_t>(o_mapq), n, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(info, w.at<uint8_t>(o_info), sizeof info, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    const uint64_t nc = cigar_off[n], nb = md_off[n];
    t_info = polyhip_aln_records_info{n, info[0], info[1], nc, nb, info[2]};
    if (nc > cigar_capacity || nb > md_capacity)
        return set_error(POLYHIP_ERR_INVALID, "%s: the records need %llu CIGAR entries and %llu MD bytes, the buffers hold %llu and %llu",
                         who, (unsigned long long)nc, (unsigned long long)nb, (unsigned long long)cigar_capacity,
                         (unsigned long long)md_capacity);
    if (nc == 0 && nb == 0)
        return POLYHIP_OK;
    // only now, bounded by the caller's capacities: the records themselves
    DevBuf dcig, dmd;
    PH_HIP(dcig.alloc(nc * sizeof(uint32_t)));
    PH_HIP(dmd.alloc(nb));
    hipLaunchKernelGGL(records_kernel<true>, dim3(wgrid), dim3(BT), 0, st, n, params->eqx, w.at<uint32_t>(o_flags), w.at<uint32_t>(o_rs),
                       w.at<uint32_t>(o_re), w.at<uint32_t>(o_rl), w.at<uint8_t>(o_a), w.at<uint8_t>(o_b), w.at<uint64_t>(o_off),
                       w.at<uint64_t>(o_coff), w.at<uint64_t>(o_moff), w.at<uint32_t>(o_nm), w.at<uint32_t>(o_err), dcig.as<uint32_t>(),
                       dmd.as<uint8_t>());
    PH_HIP(hipGetLastError());
    if (nc)
        PH_HIP(hipMemcpyAsync(cigar, dcig.p, nc * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (nb)
        PH_HIP(hipMemcpyAsync(md, dmd.p, nb, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    return POLYHIP_OK;
}

int polyhip_aln_records_last_info(polyhip_aln_records_info *info)
{
    PH_REQUIRE(info, "polyhip_aln_records_last_info: null argument");
    *info = t_info;
    return POLYHIP_OK;
}

} // extern "C"
