// k1_tauq.h -- the K1 slab pass's survivor threshold, shared by the kernel (mash_sketch.hip) and a host test
// (tests/test_k1_tauq_cpu.py compiles this header alone with the host compiler).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PH_TAUQ_HD __host__ __device__
#else
#define PH_TAUQ_HD
#endif

namespace polyhip {
namespace k1 {

// The slab pass's threshold: a hash survives iff it is <= ((target << 32) / nwin) | 0xFFFF, the value a uniform hash
// would need for `target` survivors, rounded up to 16 bits.  The quotient's low 16 bits are ORed away, and
// floor(floor(x / d) / 2^16) = floor(x / (2^16 d)), so floor((target << 16) / nwin) is all it takes: a 32-bit division
// (a float reciprocal and integer corrections, ~20 instructions) instead of the 64-bit one (over 100 scalar
// instructions and spilled SGPRs, per read).  For nwin >= 2^32 > target << 16 that quotient is 0.  Needs
// target < 2^16, i.e. s below ~65,000; the slab pass's LDS caps s near 8,000, and launch() checks it.  Bit-identical to
// the 64-bit formula: tests/test_k1_tauq_cpu.py compiles this function for the host and compares.
PH_TAUQ_HD inline uint32_t slab_tauq(uint32_t target, int64_t nwin)
{
    if ((int64_t)target >= nwin)
        return 0xFFFFFFFFu;
    if (nwin >= ((int64_t)1 << 32))
        return 0xFFFFu;
    return (((target << 16) / (uint32_t)nwin) << 16) | 0xFFFFu;
}

} // namespace k1
} // namespace polyhip
