// pileup_call.h -- the pileup family's channels, info words and base classes (pileup_walk.hip fills the count planes with
// them; pileup_rows.hip and variants.hip read them), and the pass that turns the 16 count planes into the consensus and the
// sites for polyhip_pileup and polyhip_pileup_qual (pileup.hip, which alone instantiates it; internal linkage).
#pragma once
#include "device_prims.h"

namespace polyhip {
namespace {

constexpr int PU_WAVES = BT / 64;       // entries a block walks at a time
constexpr unsigned PU_MAX_BLOCKS = 4096; // the walk is a grid-stride loop: a wave adds to the info counters once
enum : int { INFO_USED = 0, INFO_SKIPPED, INFO_BAD, INFO_COLUMNS, INFO_EDGE, INFO_WORDS };
enum : uint32_t { CH_OTHER = 4, CH_DEL = 5, CH_INS_EVENT = 6, CH_DEL_EVENT = 7, CH_STRAND = 8 };

// A/a, C/c, G/g, T/t -> 0..3, every other byte 4 (c | 0x20 is 'a' for 'A' and 'a' only, and so on)
__device__ __forceinline__ uint32_t base_class(uint32_t c)
{
    c |= 0x20u;
    return c == 'a' ? 0u : c == 'c' ? 1u : c == 'g' ? 2u : c == 't' ? 3u : CH_OTHER;
}

// One lane per position of the region.  EMIT == false: consensus[j] and nsite[j] (L + 1 slots for the scan) are written.
// EMIT == true: nsite (now the offsets) is read and the position's sites are written.
template <bool EMIT>
__global__ __launch_bounds__(BT) void call_kernel(uint64_t lo, uint64_t L, uint32_t min_depth, uint32_t min_count, uint32_t permille,
                                                  const uint32_t *__restrict__ counts, const uint8_t *__restrict__ ref,
                                                  uint8_t *__restrict__ consensus, uint64_t *nsite, polyhip_pileup_site *__restrict__ sites)
{
    for (uint64_t j = (uint64_t)blockIdx.x * BT + threadIdx.x; j < L; j += (uint64_t)gridDim.x * BT) {
        uint32_t fwd[8], two[8]; // an entry adds at most one to a cell and n < 2^32: no sum below overflows
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            fwd[k] = counts[k * L + j];
            two[k] = fwd[k] + counts[(CH_STRAND + k) * L + j];
        }
        uint32_t depth = 0, best = 0, most = two[0];
#pragma unroll
        for (uint32_t k = 0; k < 6; ++k) {
            depth += two[k];
            if (two[k] > most) { // ties stay with the lowest k
                most = two[k];
                best = k;
            }
        }
        const bool deep = depth >= min_depth;
        if (!EMIT)
            consensus[j] = deep ? (uint8_t)"ACGTN*"[best] : (uint8_t)'N';
        const uint32_t rb = ref[lo + j], rc = base_class(rb);
        uint64_t at = EMIT ? nsite[j] : 0;
#pragma unroll
        for (uint32_t s = 0; s < 6; ++s) { // SNV to A, C, G, T, then the insertion and the deletion events
            const uint32_t k = s < 4 ? s : s + 2;
            const bool is = deep && (s >= 4 || k != rc) && two[k] >= min_count && (uint64_t)two[k] * 1000u >= (uint64_t)permille * depth;
            if (!is)
                continue;
            if (EMIT) {
                polyhip_pileup_site x;
                x.pos = (uint32_t)(lo + j);
                x.depth = depth;
                x.count = two[k];
                x.count_fwd = fwd[k];
                x.kind = (uint8_t)(s < 4 ? 1u : s - 2);
                x.ref = (uint8_t)rb;
                x.alt = s < 4 ? (uint8_t)"ACGT"[s] : (uint8_t)0;
                x.pad = 0;
                sites[at] = x;
            }
            ++at;
        }
        if (!EMIT)
            nsite[j] = at;
    }
}

} // namespace
} // namespace polyhip
