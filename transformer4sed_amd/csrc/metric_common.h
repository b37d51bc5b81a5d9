// Shared by the metric kernels (metrics.hip, psds.hip, event_f1.hip): the order-preserving score key, the LDS sort over such keys and
// the integer wave reductions (common.h has the float ones).
#pragma once
#include "common.h"

// float -> uint32 whose unsigned order is the float order; -0.0 and +0.0 are one value (one tie, one operating point).
__device__ __forceinline__ uint32_t score_key(float f) {
    uint32_t u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Ascending bitonic sort of a[0, n) in LDS by the whole workgroup.  Every comparator puts the smaller key at the lower index (the first
// step of each merge stage compares mirrored positions), so slots past n behave as +inf that never move: comparators reaching them are
// skipped, and a non-power-of-two length needs no padding slots.
template <typename K> __device__ void lds_sort(K* a, int n) {
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    const int half = np2 >> 1;
    for (int k = 2; k <= np2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = threadIdx.x; q < half; q += blockDim.x) {
                int i, p;
                if (j == (k >> 1)) {
                    const int blk = q / j, t = q - blk * j;
                    i = blk * k + t;
                    p = blk * k + k - 1 - t;
                } else {
                    i = (q / j) * 2 * j + (q % j);
                    p = i + j;
                }
                if (p < n) {
                    const K x = a[i], y = a[p];
                    if (x > y) { a[i] = y; a[p] = x; }
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned long long wave_or_u64(unsigned long long v) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo |= (unsigned)__shfl_xor((int)lo, o, 64);
        hi |= (unsigned)__shfl_xor((int)hi, o, 64);
    }
    return ((unsigned long long)hi << 32) | lo;
}
