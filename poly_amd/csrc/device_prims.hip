// device_prims.hip -- the kernels of the exclusive scan and the LSD radix sort, and the host functions that launch them
// (declared in device_prims.h).  One copy for every unit that scans or sorts.
#include "device_prims.h"

namespace polyhip {
namespace {

template <class T> __global__ __launch_bounds__(BT) void scan_reduce_kernel(const T *__restrict__ in, uint64_t m, T *__restrict__ sums)
{
    const uint64_t base = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * ITEMS;
    T s = 0;
#pragma unroll
    for (int q = 0; q < ITEMS; ++q)
        if (base + q < m)
            s += in[base + q];
    T total;
    (void)block_excl_scan<T>(s, total);
    if (threadIdx.x == 0)
        sums[blockIdx.x] = total;
}

// offs == nullptr: a single block, offset 0
template <class T>
__global__ __launch_bounds__(BT) void scan_apply_kernel(const T *in, T *out, uint64_t m, const T *__restrict__ offs)
{
    const uint64_t base = (uint64_t)blockIdx.x * TILE + (uint64_t)threadIdx.x * ITEMS;
    T v[ITEMS];
    T s = 0;
#pragma unroll
    for (int q = 0; q < ITEMS; ++q) {
        v[q] = base + q < m ? in[base + q] : T(0);
        s += v[q];
    }
    T total;
    T run = block_excl_scan<T>(s, total) + (offs ? offs[blockIdx.x] : T(0));
#pragma unroll
    for (int q = 0; q < ITEMS; ++q)
        if (base + q < m) {
            out[base + q] = run;
            run += v[q];
        }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == BT - 1)
        out[m] = run;
}

// hist[d * nblocks + block] = items of the block's tile with digit d
__global__ __launch_bounds__(BT) void radix_hist_kernel(const uint64_t *__restrict__ keys, uint64_t n, int shift,
                                                        uint32_t *__restrict__ hist, uint32_t nblocks)
{
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t tile0 = (uint64_t)blockIdx.x * TILE;
    for (int it = 0; it < ITEMS; ++it) {
        const uint64_t i = tile0 + (uint64_t)it * BT + threadIdx.x;
        const bool valid = i < n;
        const uint32_t d = valid ? (uint32_t)(keys[i] >> shift) & 255u : 0u;
        const uint64_t m = same_digit_lanes(d, valid);
        if (valid && (m & ((1ull << lane) - 1)) == 0)
            atomicAdd(&cnt[d], (uint32_t)__popcll(m));
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * nblocks + blockIdx.x] = cnt[threadIdx.x];
}

// base = the exclusive scan of hist: every item goes to base[digit][block] + (items of that digit before it in the tile)
__global__ __launch_bounds__(BT) void radix_scatter_kernel(const uint64_t *__restrict__ kin, const uint32_t *__restrict__ vin,
                                                           uint64_t *__restrict__ kout, uint32_t *__restrict__ vout, uint64_t n,
                                                           int shift, const uint32_t *__restrict__ base, uint32_t nblocks)
{
    __shared__ uint32_t run[256];
    __shared__ uint32_t wcnt[BT / 64][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    run[threadIdx.x] = base[(uint64_t)threadIdx.x * nblocks + blockIdx.x];
#pragma unroll
    for (int q = 0; q < BT / 64; ++q)
        wcnt[q][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t tile0 = (uint64_t)blockIdx.x * TILE;
    for (int it = 0; it < ITEMS; ++it) {
        const uint64_t i = tile0 + (uint64_t)it * BT + threadIdx.x;
        const bool valid = i < n;
        const uint64_t k = valid ? kin[i] : 0;
        const uint32_t d = (uint32_t)(k >> shift) & 255u;
        const uint64_t m = same_digit_lanes(d, valid);
        const uint64_t below = m & ((1ull << lane) - 1);
        if (valid && below == 0)
            wcnt[w][d] = (uint32_t)__popcll(m);
        __syncthreads();
        if (valid) {
            uint32_t pos = run[d] + (uint32_t)__popcll(below);
            for (int q = 0; q < w; ++q)
                pos += wcnt[q][d];
            kout[pos] = k;
            vout[pos] = vin[i];
        }
        __syncthreads();
        uint32_t add = 0;
#pragma unroll
        for (int q = 0; q < BT / 64; ++q) {
            add += wcnt[q][threadIdx.x];
            wcnt[q][threadIdx.x] = 0;
        }
        run[threadIdx.x] += add;
        __syncthreads();
    }
}

} // namespace

template <class T> hipError_t scan_excl(const T *in, T *out, uint64_t m, uint8_t *scratch, hipStream_t st)
{
    if (m == 0)
        return hipMemsetAsync(out, 0, sizeof(T), st);
    const uint64_t nb = (m + TILE - 1) / TILE;
    if (nb == 1) {
        hipLaunchKernelGGL(scan_apply_kernel<T>, dim3(1), dim3(BT), 0, st, in, out, m, (const T *)nullptr);
        return hipGetLastError();
    }
    T *sums = reinterpret_cast<T *>(scratch);
    hipLaunchKernelGGL(scan_reduce_kernel<T>, dim3((unsigned)nb), dim3(BT), 0, st, in, m, sums);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = scan_excl<T>(sums, sums, nb, scratch + align256((nb + 1) * sizeof(T)), st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(scan_apply_kernel<T>, dim3((unsigned)nb), dim3(BT), 0, st, in, out, m, (const T *)sums);
    return hipGetLastError();
}

template hipError_t scan_excl<uint32_t>(const uint32_t *, uint32_t *, uint64_t, uint8_t *, hipStream_t);
template hipError_t scan_excl<uint64_t>(const uint64_t *, uint64_t *, uint64_t, uint8_t *, hipStream_t);

int radix_sort(uint64_t *&ka, uint32_t *&va, uint64_t *&kb, uint32_t *&vb, uint64_t N, int bits, uint32_t *hist, uint8_t *scratch,
               hipStream_t st)
{
    const uint64_t nb = radix_blocks(N);
    for (int shift = 0; shift < bits; shift += 8) {
        hipLaunchKernelGGL(radix_hist_kernel, dim3((unsigned)nb), dim3(BT), 0, st, ka, N, shift, hist, (uint32_t)nb);
        PH_HIP(hipGetLastError());
        PH_HIP(scan_excl<uint32_t>(hist, hist, 256 * nb, scratch, st));
        hipLaunchKernelGGL(radix_scatter_kernel, dim3((unsigned)nb), dim3(BT), 0, st, ka, va, kb, vb, N, shift, hist, (uint32_t)nb);
        PH_HIP(hipGetLastError());
        std::swap(ka, kb);
        std::swap(va, vb);
    }
    return POLYHIP_OK;
}

} // namespace polyhip
