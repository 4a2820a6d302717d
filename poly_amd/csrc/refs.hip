// refs.hip -- a reference of several contigs: one FM-index over their concatenation C, and the contigs' starts in C.
//
// The packed batch that comes in (bytes + k + 1 offsets) is C already: contig c is C[start_c, start_{c+1}) with start_c =
// off[c] - off[0].  The index is polyhip_bwt_create's, on the device current at creation; the set owns it and lends it out
// (polyhip_refs_index).  start[] lives on that device for the mapper's refs kernels (map_reads.hip) and for
//   resolve_kernel   one lane per entry: binary search of a position of C over start[], the contig and the local position
#include <cstring>
#include <vector>

#include "bwt_index.h"
#include "device_prims.h"

namespace polyhip {
namespace {

constexpr uint64_t REFS_MAX_CONTIGS = 1ull << 24;

__global__ __launch_bounds__(BT) void resolve_kernel(const uint32_t *__restrict__ start, uint32_t k, const uint32_t *__restrict__ pos,
                                                     const uint32_t *__restrict__ len, uint64_t n, uint32_t *__restrict__ rid,
                                                     uint32_t *__restrict__ local, uint32_t *__restrict__ err)
{
    const uint32_t total = start[k];
    for (uint64_t i = blockIdx.x * (uint64_t)BT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BT) {
        const uint32_t p = pos[i];
        const uint64_t l = len ? len[i] : 1u;
        uint32_t c = 0, at = 0, e = 1;
        if (p < total) {
            uint32_t lo = 0, hi = k; // start[lo] <= p < start[hi]
            while (hi - lo > 1) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (start[mid] <= p)
                    lo = mid;
                else
                    hi = mid;
            }
            c = lo;
            at = p - start[lo];
            e = (uint64_t)p + l > start[lo + 1] ? 2u : 0u;
        }
        rid[i] = c;
        local[i] = at;
        err[i] = e;
    }
}

RefsHandle *as_mut(polyhip_refs *h) { return reinterpret_cast<RefsHandle *>(h); }

void refs_free(RefsHandle *r)
{
    if (r->index) {
        DeviceScope ds;
        if (ds.enter(as_h(r->index)->dev) == hipSuccess && r->d_start)
            (void)hipFree(r->d_start);
        (void)polyhip_bwt_destroy(r->index);
    }
    delete[] r->starts;
    delete r;
}

} // namespace
} // namespace polyhip

using namespace polyhip;

extern "C" {

int polyhip_refs_create(const uint8_t *seqs, const uint64_t *off, uint64_t ncontigs, polyhip_refs **out)
{
    PH_REQUIRE(out, "polyhip_refs_create: null output handle");
    *out = nullptr;
    PH_REQUIRE(seqs && off, "polyhip_refs_create: null argument");
    PH_REQUIRE(ncontigs > 0, "polyhip_refs_create: a reference set needs at least one contig");
    if (ncontigs > REFS_MAX_CONTIGS)
        return set_error(POLYHIP_ERR_UNSUPPORTED, "polyhip_refs_create: %llu contigs exceed 2^24", (unsigned long long)ncontigs);
    for (uint64_t c = 0; c < ncontigs; ++c) {
        PH_REQUIRE(off[c] <= off[c + 1], "polyhip_refs_create: offsets are not ascending at %llu", (unsigned long long)c);
        PH_REQUIRE(off[c] < off[c + 1], "polyhip_refs_create: contig %llu is empty", (unsigned long long)c);
    }
    const uint64_t n = off[ncontigs] - off[0];
    PH_REQUIRE(n < 0xFFFFFFFFull, "polyhip_refs_create: contigs of %llu bytes in all are too long (suffix array entries are uint32: "
                                  "at most 2^32 - 2 bytes)", (unsigned long long)n);
    const uint8_t *text = seqs + off[0];
    if (memchr(text, NULL_CHAR, n))
        return set_error(POLYHIP_ERR_INVALID, "Provided sequence contains the nullChar $. BWT cannot be constructed");
    auto *r = new RefsHandle();
    r->k = (uint32_t)ncontigs;
    r->starts = new uint64_t[ncontigs + 1];
    std::vector<uint32_t> s32(ncontigs + 1);
    for (uint64_t c = 0; c <= ncontigs; ++c) {
        r->starts[c] = off[c] - off[0];
        s32[c] = (uint32_t)r->starts[c];
        if (c)
            r->nmax = std::max(r->nmax, s32[c] - s32[c - 1]);
    }
    auto fail = [&](int rc) {
        refs_free(r);
        return rc;
    };
    if (int rc = polyhip_bwt_create(text, n, &r->index))
        return fail(rc);
    const BwtHandle *h = as_h(r->index);
    DeviceScope ds;
    if (ds.enter(h->dev) != hipSuccess || hipMalloc((void **)&r->d_start, (ncontigs + 1) * sizeof(uint32_t)) != hipSuccess) {
        r->d_start = nullptr;
        return fail(set_error(POLYHIP_ERR_HIP, "polyhip_refs_create: allocation of %llu starts failed", (unsigned long long)ncontigs + 1));
    }
    if (hipMemcpyAsync(r->d_start, s32.data(), (ncontigs + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
        return fail(set_error(POLYHIP_ERR_HIP, "polyhip_refs_create: upload of the starts failed"));
    *out = reinterpret_cast<polyhip_refs *>(r);
    return POLYHIP_OK;
}

int polyhip_refs_destroy(polyhip_refs *h)
{
    if (h)
        refs_free(as_mut(h));
    return POLYHIP_OK;
}

int64_t polyhip_refs_count(const polyhip_refs *h)
{
    if (!h)
        return set_error(POLYHIP_ERR_INVALID, "polyhip_refs_count: null handle");
    return (int64_t)as_refs(h)->k;
}

int polyhip_refs_starts(const polyhip_refs *h, uint64_t *out)
{
    PH_REQUIRE(h && out, "polyhip_refs_starts: null argument");
    memcpy(out, as_refs(h)->starts, ((size_t)as_refs(h)->k + 1) * sizeof(uint64_t));
    return POLYHIP_OK;
}

const polyhip_bwt *polyhip_refs_index(const polyhip_refs *h)
{
    if (!h) {
        (void)set_error(POLYHIP_ERR_INVALID, "polyhip_refs_index: null handle");
        return nullptr;
    }
    return as_refs(h)->index;
}

int polyhip_refs_resolve(const polyhip_refs *hp, const uint32_t *pos, const uint32_t *len, uint64_t n, uint32_t *rid, uint32_t *local,
                         uint32_t *err)
{
    PH_REQUIRE(hp, "polyhip_refs_resolve: null handle");
    if (n == 0)
        return POLYHIP_OK;
    PH_REQUIRE(pos && rid && local && err, "polyhip_refs_resolve: null argument");
    const RefsHandle *r = as_refs(hp);
    const BwtHandle *h = as_h(r->index);
    DeviceScope ds;
    PH_HIP(ds.enter(h->dev));
    hipStream_t st = h->stream;
    // pos and len in, rid, local and err out: five arrays of n in one block
    DevBuf buf;
    PH_HIP(buf.alloc(5 * n * sizeof(uint32_t)));
    uint32_t *d = buf.as<uint32_t>();
    SyncOnExit sync(st);
    PH_HIP(hipMemcpyAsync(d, pos, n * 4, hipMemcpyHostToDevice, st));
    if (len)
        PH_HIP(hipMemcpyAsync(d + n, len, n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(resolve_kernel, dim3(grid_for(n)), dim3(BT), 0, st, r->d_start, r->k, d, len ? d + n : (const uint32_t *)nullptr, n,
                       d + 2 * n, d + 3 * n, d + 4 * n);
    PH_HIP(hipGetLastError());
    PH_HIP(hipMemcpyAsync(rid, d + 2 * n, n * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(local, d + 3 * n, n * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(err, d + 4 * n, n * 4, hipMemcpyDeviceToHost, st));
    PH_HIP(hipStreamSynchronize(st));
    return POLYHIP_OK;
}

} // extern "C"
