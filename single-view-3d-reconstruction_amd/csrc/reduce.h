// Block reductions of 256-thread workgroups, defined once.  block_sum_f64 IS the project's definition of a reproducible
// sum: every thread adds its strided share in ascending order (the caller's loop), then the tree below folds the 256
// partials in a fixed order -- the same bits on every run and on every launch geometry that keeps 256 threads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// red: 256 doubles of LDS; the block's sum is in red[0] afterwards (behind a barrier: every thread may read it; one more
// barrier before `red` is written again).  Every thread of the block must call it.
__device__ __forceinline__ void block_sum_f64(double v, double *red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
}

// The same tree for a maximum (exact in any order); red: 256 values of LDS, the maximum is in red[0] afterwards
__device__ __forceinline__ float red_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ int red_max(int a, int b) { return max(a, b); }
template <class T>
__device__ __forceinline__ void block_max(T v, T *red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = red_max(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
}

// Two integer totals of a block of NT threads added to totals[0], totals[1] (the meshers' vertex / triangle counts): wave
// shuffles, then the NT / 64 waves through LDS, then one atomic per non-zero total.  Integer sums: exact in any order.
// part: 2 x NT / 64 values of LDS.
template <int NT>
__device__ __forceinline__ void block_add_totals_u64(uint64_t v, uint64_t t, uint64_t (*part)[NT / 64], unsigned long long *totals) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    v += __shfl_xor(v, o);
    t += __shfl_xor(t, o);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[0][w] = v;
    part[1][w] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t sv = 0, st = 0;
#pragma unroll
    for (int q = 0; q < NT / 64; ++q) {
      sv += part[0][q];
      st += part[1][q];
    }
    if (sv) atomicAdd(&totals[0], (unsigned long long)sv);
    if (st) atomicAdd(&totals[1], (unsigned long long)st);
  }
}

}  // namespace
