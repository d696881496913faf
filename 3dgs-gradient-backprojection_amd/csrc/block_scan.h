// block_scan.h -- the exclusive scan of one integer per row that densify.hip and mcmc.hip share: a workgroup of 256 scans its rows
// (wave scan by shuffles, the four wave totals through LDS) and leaves its total in sums[block]; ONE workgroup then walks sums in
// chunks of 256 in ascending order with a running carry, so that sums becomes its own exclusive scan; a last pass adds sums[block] to
// every row.  Integer sums in a fixed order, no atomics and no waits between workgroups.  Each translation unit gets its own copy of
// the kernel (the unnamed namespace).
#pragma once
#include "gwbp_dev.h"

namespace gwbp {

namespace {

constexpr int kScanRows = GWBP_DENSIFY_BLOCK;
static_assert(kScanRows == 256, "the scans below are written for four waves of 64");

// exclusive scan of one value per thread over the workgroup; *total: the workgroup's sum, the same in every thread
template <typename T> __device__ __forceinline__ T block_exclusive(T v, T *wave_tot, T *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(incl, o, 64);
        if (lane >= o)
            incl += up;
    }
    if (lane == 63)
        wave_tot[wave] = incl;
    __syncthreads();
    const T t0 = wave_tot[0], t1 = wave_tot[1], t2 = wave_tot[2], t3 = wave_tot[3];
    *total = ((t0 + t1) + t2) + t3;
    const T before = wave == 0 ? (T)0 : wave == 1 ? t0 : wave == 2 ? t0 + t1 : (t0 + t1) + t2;
    return before + (incl - v);
}

__global__ __launch_bounds__(256) void k_scan_block_sums(int64_t n_blocks, int64_t *__restrict__ sums, int64_t *__restrict__ grand)
{
    __shared__ long long wave_tot[4];
    long long carry = 0;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += kScanRows) {
        const int64_t b = b0 + threadIdx.x;
        const long long v = b < n_blocks ? (long long)sums[b] : 0;
        long long total;
        const long long before = block_exclusive<long long>(v, wave_tot, &total);
        if (b < n_blocks)
            sums[b] = carry + before;
        carry += total;
        __syncthreads(); // the wave totals are read; the next chunk may write them
    }
    if (threadIdx.x == 0)
        *grand = carry;
}

} // namespace

} // namespace gwbp
