// Pieces shared by the device planners: anchor sampling (sampling.hip) and the memory-bank enqueue (queue.hip). Both restate a host
// loop that issues torch.randperm calls in a fixed order as one block prefix sum over the calls plus one thread per call.
#pragma once
#include "cseg_common.h"

namespace {

constexpr int SP_THREADS = 256;

// exclusive prefix sum over the block of one value per thread (thread order); *sum = the block's total
__device__ __forceinline__ int block_excl_scan(int v, int* red, int tid, int* sum) {
    const int lane = tid & 63, wave = tid >> 6;
    const int inc = wave_incl_scan_i(v, lane);
    __syncthreads();
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SP_THREADS / 64; ++w) {
        if (w < wave) base += red[w];
        all += red[w];
    }
    *sum = all;
    return base + inc - v;
}

// torch.randperm(n) on the CPU generator draws max(n - 1, 0) words (csrc_host/rng_draws.cpp)
__device__ __forceinline__ int draws_of(int n) { return n > 0 ? n - 1 : 0; }

}  // namespace
