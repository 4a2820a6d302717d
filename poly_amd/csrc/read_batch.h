// read_batch.h -- what the units that take a packed batch of reads with optional qualities from host pointers share (trim.hip,
// demux.hip): the batch as the caller hands it over and as the kernels see it, the letter test of the mask searches and the
// block-level info counters.
#pragma once
#include "device_prims.h"

namespace polyhip {

// one batch of reads on the device; the copies of the bytes start at the first read's (off[0], qual_off[0])
struct DevBatch {
    const uint8_t *reads, *qual; // qual == nullptr: no qualities
    const uint64_t *off, *qual_off;
};

// one batch as the caller hands it over
struct HostBatch {
    const uint8_t *reads;
    const uint64_t *off;
    const uint8_t *qual;
    const uint64_t *qual_off;
    uint8_t *out_reads, *out_qual;
    uint64_t *out_off;
};

// the upper-case letter of one of ACGTacgt, 0 for every other byte
__device__ __forceinline__ uint32_t base_code(uint32_t c)
{
    const uint32_t u = c & ~0x20u;
    return (u == 'A' || u == 'C' || u == 'G' || u == 'T') ? u : 0u;
}

// a wave's count into the block's counter in LDS
__device__ __forceinline__ void add_info(uint32_t *s_info, int which, uint32_t mine)
{
    const uint32_t all = (uint32_t)__builtin_amdgcn_readlane((int)dpp_incl_scan(mine), 63);
    if ((threadIdx.x & 63) == 0 && all)
        atomicAdd(&s_info[which], all);
}

} // namespace polyhip
