// Shared host-side helpers for libsvr_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include "error.h"  // set_error, SVR_CHECK, svr_hip.h
#include "workspace.h"  // WsCursor: one layout function per multi-piece workspace

namespace svr {
inline int launch_status(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return (int)e;
  }
  return SVR_OK;
}
__host__ __device__ inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// XCD-aware workgroup order: blocks are dealt round-robin over the 8 XCDs (each with its own 4 MB L2), so tiles
// that share an operand panel should have equal `block id % 8`.  1-D grids are padded to a multiple of 8 and the
// linear block id is mapped to a logical index that is contiguous per XCD; indices >= the real count exit.
constexpr int kXcds = 8;
inline unsigned xcd_grid(int64_t total) { return (unsigned)(kXcds * cdiv(total, kXcds)); }
__device__ __forceinline__ int64_t xcd_logical(int64_t bid, int64_t grid) { return (bid % kXcds) * (grid / kXcds) + bid / kXcds; }
// 256-byte aligned start of a caller's workspace (every *_workspace size includes the slack) ...
template <class T = char>
inline T *align256(const void *p) { return (T *)(((uintptr_t)p + 255) & ~(uintptr_t)255); }
inline int64_t align256(int64_t bytes) { return (bytes + 255) / 256 * 256; }   // ... and the size of a piece of it
// The weight-plane workspaces of the split GEMMs and convs (PREPARE fills them, RUN reads them).  bf16 split: `n` planes of
// `elems` uint16 back to back, on a cursor with base alignment 16.  Scaled f16 split: the |max| word of W on a 256-byte line of
// its own, then the two planes.
inline uint16_t *planes_layout(WsCursor &c, int64_t elems, int n) { return c.take<uint16_t>(n * elems, 2); }
struct ScaledPlanesWs { uint32_t *amax; uint16_t *planes; };
inline ScaledPlanesWs scaled_planes_layout(WsCursor &c, int64_t elems) { return {c.take<uint32_t>(64), c.take<uint16_t>(2 * elems, 2)}; }

// ---- functions shared between translation units, each declared once here ----
// gemm.hip: out[n] = sum_m Y[m][n] (part: colsum_workspace_floats(M, N) floats), and the ordered f64 sum of partials it ends
// in, out[n] = sum_p part[p][n] -- one workgroup per column
void colsum_launch(const float *Y, int64_t ldy, float *out, float *part, int64_t M, int64_t N, hipStream_t s);
int64_t colsum_workspace_floats(int64_t M, int64_t N);
void col_parts_sum_launch(const float *part, float *out, int64_t N, int parts, hipStream_t s);
// gemm_f16x3.hip: amax[0] = bit pattern of max |W[n * ldw + k]| over N x K (memset + one launch); the input of w_scale (f16x3.h).
// grid = 0: min(cdiv(N K, 1024), 1024) workgroups
void w_amax_launch(const float *W, int64_t ldw, int64_t N, int64_t K, uint32_t *amax, hipStream_t s, unsigned grid = 0);
// bn_pool.hip: mean / biased variance from per-block partial sums [blocks][2C] (f64); ... + svr_bn_finalize(training = 1) in
// one launch (stats may be null); out[c] = ordered f64 sum of part[b][c]
void bn_stats_final_launch(const double *part, double *stats, int64_t rows, int C, int blocks, hipStream_t s);
void bn_stats_finalize_launch(const double *part, double *stats, int64_t rows, int C, int blocks, const float *gamma,
                              const float *beta, float *rmean, float *rvar, float *ss, float *mean_f32, float eps, float momentum,
                              hipStream_t s);
void bn_sum_parts_launch(const double *part, double *out, int cols, int blocks, hipStream_t s);
// conv3d.hip: dWp = ordered f64 sum of `parts` slabs [part][tap][tile][32][32] (+ db from dbpart [dbparts][Co] in the same
// launch); conv_in's dWp[tap][co] / db[co] from per-workgroup slabs [part][32 taps][32] / [part][Co]
void conv3d_bwd_weight_reduce_launch(const float *slab, float *dWp, int Ci, int Co, int cit, int cot, int parts,
                                     hipStream_t s, int param_layout, const float *dbpart, float *db, int dbparts);
void conv3d_c1_wgrad_reduce_launch(const float *slab, float *dWp, int Co, int parts, int param_layout, const float *dbpart,
                                   float *db, hipStream_t s);
// conv3d.hip / conv3d_bwdw_bf16.hip: which kernel (SVR_WGRAD_*) a 3x3x3 weight-gradient entry point runs for a shape, with how
// many workgroups per channel-tile pair (parts) and how many bricks the busiest of them walks (per_part).  Host arithmetic only;
// each launcher asks its own function, svr_conv3d_k3_bwd_weight_variant exports both.  Returns SVR_OK or the entry point's refusal.
struct WgradVariant { int kernel, parts; int64_t per_part; };
int conv3d_bwd_weight_f32_variant(int B, int D, int H, int W, int Ci, int Co, WgradVariant *v);
int conv3d_bwd_weight_x3_variant(int B, int D, int H, int W, int Ci, int Co, WgradVariant *v);
// sort.hip: stable 32-bit key / value radix sort (rocPRIM)
size_t sort_pairs_u32_temp_bytes(int64_t n, int bits);
hipError_t sort_pairs_u32(void *tmp, size_t tmp_bytes, const uint32_t *kin, uint32_t *kout, const int32_t *vin, int32_t *vout,
                          int64_t n, int bits, hipStream_t s);
size_t scan_max_i32_temp_bytes(int64_t n);
hipError_t scan_max_i32(void *tmp, size_t tmp_bytes, const int32_t *in, int32_t *out, int64_t n, hipStream_t s);
// gemm_bf16x3.hip: dX = dY W on the scaled f16 split through the k-step-32 kernel (planes [K][N]); see svr_linear_bwd_data_f16x3
int linear_bwd_data_f16_nn(const float *dY, int64_t lddy, const float *W, int64_t ldw, float *dX, int64_t lddx, int64_t M, int64_t N,
                           int64_t K, int epilogue, const float *mask, int64_t ldmask, const uint32_t *amax_dy, uint32_t *amax_dx,
                           void *workspace, hipStream_t s);
size_t scan_sum_excl_i32_temp_bytes(int64_t n);
hipError_t scan_sum_excl_i32(void *tmp, size_t tmp_bytes, const int32_t *in, int32_t *out, int64_t n, hipStream_t s);
size_t scan_sum_excl_u64_temp_bytes(int64_t n);
hipError_t scan_sum_excl_u64(void *tmp, size_t tmp_bytes, const uint64_t *in, uint64_t *out, int64_t n, hipStream_t s);
}  // namespace svr

#ifdef __HIPCC__
// Publish a wave's |max| into an amax word (bit pattern of a non-negative float; unsigned order = float order).  Tens of
// thousands of waves hit ONE address: an atomic per wave cost 0.25 ms on a 0.26 ms BatchNorm pass -- so the wave first reads the
// word (a stale, smaller value only costs an atomic that changes nothing) and issues the atomic only if it would raise it.
__device__ __forceinline__ void svr_amax_publish(uint32_t *amax, float vmax) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
  if ((threadIdx.x & 63) == 0) {
    const uint32_t bits = __float_as_uint(vmax);
    if (bits > *reinterpret_cast<volatile uint32_t *>(amax)) atomicMax(amax, bits);
  }
}
#endif
