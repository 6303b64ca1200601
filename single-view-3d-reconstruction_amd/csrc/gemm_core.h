// LDS-tiled exact-f32 MFMA GEMM core for gfx950 (v_mfma_f32_32x32x2_f32, 64-lane waves).
//
// C[BM x BN] += A[BM x K] * B[K x BN], 256 threads = 4 waves arranged WR x WC, every wave
// owning TM x TN tiles of 32x32.  K is consumed in steps of BK = 16 through a double
// buffered LDS image  As[buf][k][m], Bs[buf][k][n]  (k-major, so the MFMA fragment read
// "lane l -> A[i = l&31][k = l>>5]" is 32 consecutive floats per half wave: conflict free).
// Global loads for step t+1 are issued before the MFMAs of step t and written to the other
// LDS buffer afterwards: one barrier per step.
//
// Loaders are small structs: load(kt) pulls this thread's slice of k-step kt into
// registers, store(tile) writes it into one LDS tile.  Two shapes cover every operand on the
// path:  RowK (a row-major [rows][K] operand, K contiguous: activations X, weights W[N][K],
// the conv input gathered per output voxel) and KRow ([K][cols], cols contiguous: packed
// conv weights, the two operands of a weight-gradient product).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

// ---- launch plans of the point-MLP GEMMs (host side) -------------------------------------------------------------------------
// Which kernel, epilogue form, reduction split and bias-sum form a linear entry point of gemm.hip / gemm_f16x3.hip /
// gemm_bf16x3.hip / gemm_bf16x6.hip takes for a shape, its leading dimensions and the low address bits of its operands, and
// the refusal it answers with otherwise.  The launchers call lin_plan() and act on the result; svr_linear_variant (gemm.hip)
// exports the same call, so the answer cannot drift from what runs.  Nothing here touches the device.
// (gemm_f16x3.hip / gemm_bf16x3.hip have loaders of their own under the names used below: they define SVR_GEMM_PLAN_ONLY.)
namespace svr {

struct LinQuery {
  int op;                        // SVR_LIN_*
  int64_t M, N, K;               // x (M,K), w (N,K), dy (M,N)
  int64_t lda, ldb, ldo, ldm;    // leading dimensions: first operand (X / dY), second (W; X of backward-weight), output, mask
  unsigned a_lo, b_lo, o_lo, m_lo;   // low four address bits of the same
  int epilogue;                  // SVR_EPI_*
  int want_bias;                 // backward-weight: db asked for
  int run;                       // 0: a PREPARE call (weights only) -- the shape checks alone
};
struct LinPlan {
  int kernel, coalesced, splits, bias;   // SVR_LIN_K_*, float4 epilogue, reduction splits, SVR_LIN_BIAS_*
  int64_t rows_per_split;
};

inline unsigned lo4(const void *p) { return (unsigned)((uintptr_t)p & 15); }

// the float4 epilogue of linear_nt_h3_kernel (gemm_f16x3.hip); N / ldy / Y are the kernel's (backward: N = dX's columns)
__host__ __device__ inline bool nt_h3_coalesced(int TN, bool bwd, int64_t N, int64_t ldy, uintptr_t Y, bool mask, int64_t ldm,
                                                uintptr_t maskp) {
  return TN == 128 && N % 4 == 0 && ldy % 4 == 0 && (Y & 15) == 0 && (!bwd || !mask || (ldm % 4 == 0 && (maskp & 15) == 0));
}
// colsum_launch (gemm.hip): the float4 kernel needs N / 4 column quads that divide the workgroup
inline bool colsum_vec(int64_t N, int64_t ldy, uintptr_t Y) {
  return N % 4 == 0 && N / 4 <= 256 && 256 % (N / 4) == 0 && ldy % 4 == 0 && (Y & 15) == 0;
}
// exact-f32 dW: splits of whole 16-row k-steps, ~2048 workgroups
inline int tn_splits_f32(int64_t M, int64_t N, int64_t K, int *steps_per_split) {
  int64_t tiles = cdiv(N, 128) * cdiv(K, 128);
  int64_t steps = cdiv(M, 16);
  int64_t want = cdiv(2048, tiles);
  int64_t splits = want < 1 ? 1 : want;
  if (splits > steps) splits = steps > 0 ? steps : 1;
  int64_t sps = cdiv(steps, splits);
  splits = steps > 0 ? cdiv(steps, sps) : 1;
  *steps_per_split = (int)sps;
  return (int)splits;
}
// split-precision dW (k-step 32): three 4-wave workgroups per CU, two rounds
inline int tn_splits_x3(int64_t M, int64_t N, int64_t K, int64_t *rows_per_split) {
  int64_t tiles = cdiv(N, 128) * cdiv(K, 128);
  int64_t want = cdiv(1536, tiles);
  if (want < 1) want = 1;
  int64_t rps = cdiv(cdiv(M, want), 32) * 32;  // multiple of the k-step
  if (rps < 32) rps = 32;
  *rows_per_split = rps;
  return (int)cdiv(M, rps);
}

inline int lin_plan(const LinQuery &q, LinPlan &p) {
  const int64_t M = q.M, N = q.N, K = q.K;
  const bool a16 = q.lda % 4 == 0 && q.a_lo == 0, b16 = q.ldb % 4 == 0 && q.b_lo == 0, o16 = q.ldo % 4 == 0 && q.o_lo == 0;
  const bool masked = q.epilogue == SVR_EPI_MASK, m16 = q.ldm % 4 == 0 && q.m_lo == 0;
  const bool fwd_epi = q.epilogue == SVR_EPI_NONE || q.epilogue == SVR_EPI_BIAS || q.epilogue == SVR_EPI_BIAS_RELU;
  p = LinPlan{-1, 0, 1, SVR_LIN_BIAS_NONE, M};
  switch (q.op) {
    case SVR_LIN_FWD_F32:
      p.kernel = SVR_LIN_K_NT;
      if (M == 0) return SVR_OK;  // empty point set
      SVR_CHECK(M >= 0 && N > 0 && K > 0 && K % 16 == 0, SVR_E_BADSHAPE, "linear_fwd: M=%ld N=%ld K=%ld (K %% 16)", (long)M, (long)N, (long)K);
      SVR_CHECK(a16 && b16, SVR_E_ALIGN, "linear_fwd: operands must be 16-byte aligned");
      SVR_CHECK(q.epilogue >= SVR_EPI_NONE && q.epilogue <= SVR_EPI_MASK, SVR_E_BADARG, "bad epilogue %d", q.epilogue);
      return SVR_OK;
    case SVR_LIN_BWD_DATA_F32:
      p.kernel = SVR_LIN_K_NN;
      if (M == 0) return SVR_OK;
      SVR_CHECK(M >= 0 && N > 0 && K > 0 && N % 16 == 0 && K % 4 == 0, SVR_E_BADSHAPE, "linear_bwd_data: M=%ld N=%ld K=%ld", (long)M, (long)N, (long)K);
      SVR_CHECK(a16 && b16, SVR_E_ALIGN, "linear_bwd_data: operands must be 16-byte aligned");
      SVR_CHECK(q.epilogue == SVR_EPI_NONE || masked, SVR_E_BADARG, "linear_bwd_data: epilogue %d", q.epilogue);
      return SVR_OK;
    case SVR_LIN_BWD_WEIGHT_F32: {
      p.kernel = SVR_LIN_K_TN;
      SVR_CHECK(M > 0 && N > 0 && K > 0 && N % 4 == 0 && K % 4 == 0, SVR_E_BADSHAPE, "linear_bwd_weight: M=%ld N=%ld K=%ld", (long)M, (long)N, (long)K);
      SVR_CHECK(a16 && b16, SVR_E_ALIGN, "linear_bwd_weight: operands must be 16-byte aligned");
      int sps;
      p.splits = tn_splits_f32(M, N, K, &sps);
      p.rows_per_split = (int64_t)sps * 16;
      if (q.want_bias) p.bias = colsum_vec(N, q.lda, q.a_lo) ? SVR_LIN_BIAS_COLSUM_VEC : SVR_LIN_BIAS_COLSUM_SLOW;
      return SVR_OK;
    }
    case SVR_LIN_FWD_F16X3:
      p.kernel = N <= 64 ? SVR_LIN_K_NT64 : SVR_LIN_K_NT128;   // narrow outputs: 128 x 64 tiles, two waves, half the wasted columns
      if (M == 0 && q.run) return SVR_OK;
      SVR_CHECK(M >= 0 && N > 0 && K > 0 && K % 16 == 0, SVR_E_BADSHAPE, "linear_fwd_f16x3: M=%ld N=%ld K=%ld (K %% 16)", (long)M, (long)N, (long)K);
      if (!q.run) return SVR_OK;
      SVR_CHECK(a16, SVR_E_ALIGN, "linear_fwd_f16x3: X must be 16-byte aligned");
      SVR_CHECK(fwd_epi, SVR_E_BADARG, "linear_fwd_f16x3: epilogue %d", q.epilogue);
      p.coalesced = nt_h3_coalesced(N <= 64 ? 64 : 128, false, N, q.ldo, q.o_lo, false, 0, 0);
      return SVR_OK;
    case SVR_LIN_FWD_BF16X6:
      p.kernel = SVR_LIN_K_NT_X6;
      if (M == 0) return SVR_OK;
      SVR_CHECK(M >= 0 && N > 0 && K > 0 && K % 16 == 0, SVR_E_BADSHAPE, "linear_fwd_bf16x6: M=%ld N=%ld K=%ld (K %% 16)", (long)M, (long)N, (long)K);
      SVR_CHECK(a16, SVR_E_ALIGN, "linear_fwd_bf16x6: X must be 16-byte aligned");
      SVR_CHECK(fwd_epi, SVR_E_BADARG, "linear_fwd_bf16x6: epilogue %d", q.epilogue);
      return SVR_OK;
    case SVR_LIN_BWD_DATA_F16X3S: {
      // the k-step-32 kernel of gemm_bf16x3.hip where the shape allows it, else the forward kernel with transposed planes (k-step 16)
      // (a function of the SHAPE only: PREPARE and RUN calls must agree on the plane layout)
      const bool nn = N % 32 == 0 && K % 4 == 0;
      p.kernel = nn ? SVR_LIN_K_NN_X3 : SVR_LIN_K_NT128_BWD;
      if (M == 0 && q.run) return SVR_OK;
      SVR_CHECK(M >= 0 && N > 0 && K > 0 && N % 16 == 0, SVR_E_BADSHAPE, "linear_bwd_data_f16x3: M=%ld N=%ld K=%ld (N %% 16)", (long)M, (long)N, (long)K);
      if (!q.run) return SVR_OK;
      SVR_CHECK(a16, SVR_E_ALIGN, "linear_bwd_data_f16x3: dY must be 16-byte aligned");
      SVR_CHECK(q.epilogue == SVR_EPI_NONE || masked, SVR_E_BADARG, "linear_bwd_data_f16x3: epilogue %d", q.epilogue);
      if (nn) {
        SVR_CHECK(o16 && (!masked || m16), SVR_E_ALIGN,
                  "linear_bwd_data_f16x3: dX and the mask must be 16-byte aligned with leading dimensions that are multiples of 4");
        p.coalesced = 1;
      } else {
        p.coalesced = nt_h3_coalesced(128, true, K, q.ldo, q.o_lo, masked, q.ldm, q.m_lo);
      }
      return SVR_OK;
    }
    case SVR_LIN_BWD_DATA_BF16X3:
      p.kernel = SVR_LIN_K_NN_X3;
      p.coalesced = 1;
      if (M == 0 && q.run) return SVR_OK;
      SVR_CHECK(M >= 0 && N > 0 && K > 0 && N % 32 == 0 && K % 4 == 0, SVR_E_BADSHAPE,
                "linear_bwd_data_bf16x3: M=%ld N=%ld K=%ld (need N %% 32 == 0, K %% 4 == 0)", (long)M, (long)N, (long)K);
      if (!q.run) return SVR_OK;
      SVR_CHECK(q.ldo % 4 == 0 && q.ldm % 4 == 0, SVR_E_BADSHAPE, "linear_bwd_data_bf16x3: leading dimensions must be multiples of 4");
      SVR_CHECK(a16, SVR_E_ALIGN, "linear_bwd_data_bf16x3: dY must be 16-byte aligned");
      SVR_CHECK(q.epilogue == SVR_EPI_NONE || masked, SVR_E_BADARG, "linear_bwd_data_bf16x3: epilogue %d", q.epilogue);
      // linear_nn_x3_kernel moves both as float4
      SVR_CHECK(q.o_lo == 0 && (!masked || q.m_lo == 0), SVR_E_ALIGN, "linear_bwd_data_bf16x3: dX and the mask must be 16-byte aligned");
      return SVR_OK;
    case SVR_LIN_BWD_WEIGHT_BF16X3:
      SVR_CHECK(M > 0 && N > 0 && K > 0 && N % 4 == 0, SVR_E_BADSHAPE, "linear_bwd_weight_bf16x3: M=%ld N=%ld K=%ld (N %% 4)", (long)M, (long)N, (long)K);
      SVR_CHECK(a16, SVR_E_ALIGN, "linear_bwd_weight_bf16x3: dY must be 16-byte aligned");
      // both operands row-major through the transposing LDS reads, or (X not float4-able) the dY pre-pass + transposing loader
      p.kernel = (K % 4 == 0 && b16 && N >= 4 && K >= 4) ? SVR_LIN_K_TN_TR : SVR_LIN_K_TN_PREPASS;
      p.splits = tn_splits_x3(M, N, K, &p.rows_per_split);
      if (q.want_bias) p.bias = SVR_LIN_BIAS_KERNEL;
      return SVR_OK;
    case SVR_LIN_BWD_WEIGHT_F16X3S:
      p.kernel = SVR_LIN_K_TN_TR;
      SVR_CHECK(M > 0 && N >= 4 && K >= 4 && N % 4 == 0 && K % 4 == 0, SVR_E_BADSHAPE, "linear_bwd_weight_f16x3: M=%ld N=%ld K=%ld (N, K %% 4)", (long)M, (long)N, (long)K);
      SVR_CHECK(a16 && b16, SVR_E_ALIGN, "linear_bwd_weight_f16x3: dY and X must be 16-byte aligned with leading dimensions that are multiples of 4");
      p.splits = tn_splits_x3(M, N, K, &p.rows_per_split);
      if (q.want_bias) p.bias = SVR_LIN_BIAS_KERNEL;
      return SVR_OK;
  }
  SVR_CHECK(false, SVR_E_BADARG, "linear plan: op %d", q.op);
}

}  // namespace svr

#ifndef SVR_GEMM_PLAN_ONLY

namespace svr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int BK = 16;

template <int WR_, int WC_, int TM_, int TN_>
struct TileCfg {
  static constexpr int WR = WR_, WC = WC_, TM = TM_, TN = TN_;
  static constexpr int BM = WR * TM * 32, BN = WC * TN * 32;
  static_assert(WR * WC == 4, "4 waves per workgroup");
};

// ---- RowK: tile rows x 16 k, source rows are k-contiguous ------------------------------------
// LD must satisfy LD % 8 == 2 so the 4 scalar LDS writes of a float4 are conflict free
// (lane -> (row = lane/4, quad = lane%4): bank = (quad*4+e)*LD + row).
template <int ROWS, class PtrFn>
struct RowKLoader {
  static constexpr int R = (ROWS + 63) / 64;  // float4 per thread
  static constexpr int LD = ROWS + 2;
  PtrFn fn;  // const float* fn(int row_in_tile, int kt)  -> pointer to 16 contiguous floats or nullptr
  float4 v[R];
  __device__ __forceinline__ void load(int kt) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      int row = (t >> 2) + 64 * i;
      const float *p = (ROWS % 64 == 0 || row < ROWS) ? fn(row, kt) : nullptr;
      v[i] = p ? *reinterpret_cast<const float4 *>(p + (t & 3) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __device__ __forceinline__ void store(float *tile) const {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      int row = (t >> 2) + 64 * i;
      if (ROWS % 64 == 0 || row < ROWS) {
        float *d = tile + ((t & 3) * 4) * LD + row;
        d[0] = v[i].x;
        d[LD] = v[i].y;
        d[2 * LD] = v[i].z;
        d[3 * LD] = v[i].w;
      }
    }
  }
};

// ---- KRow: 16 k x COLS, source is [k][col] with col contiguous ------------------------------
template <int COLS, class PtrFn>
struct KRowLoader {
  static constexpr int Q = COLS / 4;                 // float4 per k-row
  static constexpr int R = (16 * Q + 255) / 256;     // float4 per thread
  static constexpr int LD = COLS + 4;
  PtrFn fn;  // const float* fn(int k_in_step, int col4, int kt) -> pointer to 4 floats or nullptr
  float4 v[R];
  __device__ __forceinline__ void load(int kt) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      int idx = t + 256 * i;
      const float *p = (idx < 16 * Q) ? fn(idx / Q, (idx % Q) * 4, kt) : nullptr;
      v[i] = p ? *reinterpret_cast<const float4 *>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __device__ __forceinline__ void store(float *tile) const {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < R; ++i) {
      int idx = t + 256 * i;
      if (idx < 16 * Q) *reinterpret_cast<float4 *>(tile + (idx / Q) * LD + (idx % Q) * 4) = v[i];
    }
  }
};

template <class Cfg, class AL, class BL>
struct GemmSmem {
  float a[2][BK * AL::LD];
  float b[2][BK * BL::LD];
};

// Runs the k loop [kt0, kt1) and leaves the block tile in acc[TM][TN] (MFMA C layout:
// reg r of lane l = C[32*tile_m + (r&3) + 8*(r>>2) + 4*(l>>5)][32*tile_n + (l&31)]).
template <class Cfg, class AL, class BL>
__device__ __forceinline__ void gemm_mainloop(AL &al, BL &bl, GemmSmem<Cfg, AL, BL> &sm, int kt0, int kt1,
                                              f32x16 (&acc)[Cfg::TM][Cfg::TN]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave / Cfg::WC, wc = wave % Cfg::WC;
  const int l31 = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  if (kt0 >= kt1) return;
  al.load(kt0);
  bl.load(kt0);
  al.store(sm.a[0]);
  bl.store(sm.b[0]);
  __syncthreads();
  int buf = 0;
  for (int kt = kt0; kt < kt1; ++kt) {
    const bool more = kt + 1 < kt1;
    if (more) {
      al.load(kt + 1);
      bl.load(kt + 1);
    }
    const float *as = sm.a[buf] + wr * (Cfg::TM * 32) + l31;
    const float *bs = sm.b[buf] + wc * (Cfg::TN * 32) + l31;
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      float af[Cfg::TM], bf[Cfg::TN];
#pragma unroll
      for (int i = 0; i < Cfg::TM; ++i) af[i] = as[(kk * 2 + lh) * AL::LD + i * 32];
#pragma unroll
      for (int j = 0; j < Cfg::TN; ++j) bf[j] = bs[(kk * 2 + lh) * BL::LD + j * 32];
#pragma unroll
      for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
        for (int j = 0; j < Cfg::TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      al.store(sm.a[buf ^ 1]);
      bl.store(sm.b[buf ^ 1]);
    }
    __syncthreads();
    buf ^= 1;
  }
}

// Visit every accumulator element of this thread: f(row_in_block, col_in_block, value).
template <class Cfg, class F>
__device__ __forceinline__ void gemm_foreach(f32x16 (&acc)[Cfg::TM][Cfg::TN], F f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave / Cfg::WC, wc = wave % Cfg::WC;
#pragma unroll
  for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j) {
      const int col = wc * (Cfg::TN * 32) + j * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wr * (Cfg::TM * 32) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        f(row, col, acc[i][j][r]);
      }
    }
}

}  // namespace svr
#endif  // SVR_GEMM_PLAN_ONLY
