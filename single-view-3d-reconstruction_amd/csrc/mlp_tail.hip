// Fused tail of the point MLP for gfx950: fc_1 + ReLU, fc_2 + ReLU and fc_out in ONE kernel, bit for bit what
// svr_linear_fwd_f16x3 (twice) and svr_fc_out_fwd return.
//
// The three separate kernels read h0, write h1, read h1, write h2, read h2: 2.05 GB at 400 000 rows, of which the two
// read-backs (0.82 GB) serve nothing -- the backward needs h1 and h2 WRITTEN, not read.  Here a workgroup owns TTM = 64 rows
// and all 256 columns (eight waves of 64 x 32 outputs; two workgroups per CU = four waves per SIMD.  Four waves of 64 x 64, the
// shape of gather_fc0.hip's consumers, were 5 % slower: 176 VGPRs, two waves per SIMD):
//   * the h0 tile is read once (one 1 KB row per wave and load), split (split_x) into f16 hi / lo planes in LDS -- all 16
//     k-steps of it: 64 KB, the whole reduction of fc_1;
//   * fc_1: every wave multiplies the planes with W1's pre-split planes, which it reads straight from L2 in MFMA fragment
//     layout (no LDS staging, nothing shared between the waves), three k-steps ahead in a ring of four register sets;
//   * behind a barrier the epilogue values (acc 2^-s + b1, ReLU) go to h1 with streaming stores AND, split again, into the
//     same LDS planes: h1 is the A operand of fc_2 without ever being read back;
//   * fc_2 the same way on W2's planes (whose first k-steps were requested in front of fc_1's epilogue); its epilogue values
//     go to LDS as an f32 tile (the planes are dead by then), from where h2 is stored in float4 pieces and fc_out's dot
//     product is taken in svr_fc_out_fwd's order: 16 lanes per row, four strided float4 terms each, the xor tree 8, 4, 2, 1.
//
// Why the bits cannot move: an output element of linear_nt_h3_kernel (gemm_f16x3.hip) is ONE fixed sequence -- k-steps of
// 16 ascending; per 32 x 32 x 16 block v_mfma_f32_32x32x16_f16 three times, lo(x) hi(w) 2^-11, hi(x) lo(w), hi(x) hi(w); the
// operands of split_x and of split_w on W 2^s (w_scale of the same amax word); then acc 2^-s + bias, ReLU -- and none of it
// depends on the tile shape.  This kernel issues that sequence on those operands.  No atomics, no host synchronisation.
#include "common.h"
#include "f16x3.h"
#include "mlp_tail_layout.h"

using namespace svr;

namespace {

constexpr int TH = (int)kMlpTailHidden;   // hidden width: reduction length and output columns of fc_1 / fc_2
constexpr int TTM = 64;                   // rows per workgroup
constexpr int TNW = 8;                    // waves per workgroup, each TTM rows x TH / TNW columns
constexpr int TJT = TH / (32 * TNW);      // 32-column MFMA tiles per wave
constexpr int TNT = 64 * TNW;             // threads per workgroup
constexpr int TRW = TTM / TNW;            // rows of the h0 tile a wave loads
constexpr int TLW = 8;                    // dwords per LDS row of one k-step: 16 halves = two 16-byte slots (slot_dw)
constexpr int TNK = TH / 16;              // k-steps per layer
constexpr int TPLANE = TTM * TLW;         // dwords per plane and k-step
constexpr int TKSTEP = 2 * TPLANE + 8;    // hi + lo; + 8 dwords: the 16 k-steps one wave's store covers land on different banks
constexpr int T_LDS_BYTES = TNK * TKSTEP * 4;
constexpr int WKSTEP = 2 * (TH / 32) * 512;   // halves per k-step of the W planes (hi and lo: 8 row tiles x 64 lanes x 8 halves each)
static_assert((TNW == 4 || TNW == 8) && TH == 256 && T_LDS_BYTES >= TTM * TH * 4 && 2 * T_LDS_BYTES <= 160 * 1024, "the f32 h2 tile fits; two workgroups per CU");

// Fragment-major W planes, gather_fc0.hip's layout: the 16 halves x 32 rows of one MFMA B fragment are 1 KB contiguous (lane l
// reads 16 bytes at l * 16), k-step major: [k-step][hi / lo][row tile of 32][lane 64][8 halves].
__device__ __forceinline__ int wfrag_index(int kk, int plane, int n) {
  return ((((kk >> 4) * 2 + plane) * (TH / 32) + (n >> 5)) * 64 + ((kk >> 3) & 1) * 32 + (n & 31)) * 8 + (kk & 7);
}

// W[n][k] f32 (row stride ldw) -> the planes hi(W 2^s), lo(W 2^s): the words split_w_kernel makes, in fragment order
__global__ __launch_bounds__(64) void mlp_tail_split_w_kernel(const float *__restrict__ W, int64_t ldw, const uint32_t *__restrict__ amax,
                                                              uint16_t *__restrict__ p0) {
  const int kk = blockIdx.x * 64 + threadIdx.x, n = blockIdx.y;   // grid (TH / 64, TH)
  const float w = W[(int64_t)n * ldw + kk] * w_scale(amax[0], false);
  _Float16 h, l;
  split_w(w, h, l);
  p0[wfrag_index(kk, 0, n)] = __builtin_bit_cast(uint16_t, h);
  p0[wfrag_index(kk, 1, n)] = __builtin_bit_cast(uint16_t, l);
}

__device__ __forceinline__ float lane_xor1(float v) {   // the value of lane ^ 1 (quad_perm [1, 0, 3, 2])
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xf, 0xf, true));
}

// two workgroups per CU: TNW / 2 waves per SIMD
__global__ __launch_bounds__(TNT, TNW / 2) void mlp_tail_kernel(const float *__restrict__ H0, int64_t ldh0, const uint16_t *__restrict__ P1,
                                                          const uint32_t *__restrict__ amax1, const float *__restrict__ b1,
                                                          const uint16_t *__restrict__ P2, const uint32_t *__restrict__ amax2,
                                                          const float *__restrict__ b2, const float *__restrict__ wo,
                                                          const float *__restrict__ bo, float *__restrict__ H1, int64_t ldh1,
                                                          float *__restrict__ H2, int64_t ldh2, float *__restrict__ logits,
                                                          const int32_t *__restrict__ row_map, int64_t M) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int t = threadIdx.x, lane = t & 63, wc = t >> 6;   // wave wc -> columns [32 TJT wc, 32 TJT (wc + 1))
  const int l31 = lane & 31, lh = lane >> 5;
  const int64_t m0 = (int64_t)blockIdx.x * TTM;   // (the grid is cdiv(M, TTM): m0 < M)

  // W fragments: a ring of four register sets over the 32 k-steps of both layers, three k-steps in flight
  uint4 w[4][TJT][2];   // [set][column tile][hi / lo]
  const int woff = ((TJT * wc) * 64 + lane) * 8;
  auto loadb = [&](uint4 (&r)[TJT][2], int g) {   // g: k-step of fc_1 (0 .. 15) or of fc_2 (16 .. 31)
    const uint16_t *q = (g < TNK ? P1 + g * WKSTEP : P2 + (g - TNK) * WKSTEP) + woff;
#pragma unroll
    for (int jt = 0; jt < TJT; ++jt) {
      r[jt][0] = *reinterpret_cast<const uint4 *>(q + jt * 512);
      r[jt][1] = *reinterpret_cast<const uint4 *>(q + (TH / 32) * 512 + jt * 512);
    }
  };
#pragma unroll
  for (int g = 0; g < 3; ++g) loadb(w[g], g);

  // the h0 tile: wave wc reads rows [TRW wc, TRW (wc + 1)), one 1 KB row per load (rows past M: the last row again -- they only
  // feed outputs that are never stored), all TRW loads in flight, then split into the planes
  {
    float4 x[TRW];
#pragma unroll
    for (int i = 0; i < TRW; ++i) {
      int64_t m = m0 + wc * TRW + i;
      m = m < M ? m : M - 1;
      x[i] = *reinterpret_cast<const float4 *>(H0 + m * ldh0 + lane * 4);
    }
#pragma unroll
    for (int i = 0; i < TRW; ++i) {
      uint32_t h0, l0, h1, l1;
      split_x(x[i].x, x[i].y, h0, l0);
      split_x(x[i].z, x[i].w, h1, l1);
      const int off = (lane >> 2) * TKSTEP + slot_dw(wc * TRW + i, (lane & 3) >> 1) + (lane & 1) * 2;   // 4 halves = half a slot
      *reinterpret_cast<uint2 *>(lds + off) = make_uint2(h0, h1);
      *reinterpret_cast<uint2 *>(lds + TPLANE + off) = make_uint2(l0, l1);
    }
  }
  __syncthreads();

  f32x16 acc[2][TJT];
  // one layer's 16 k-steps on the planes in LDS; k-step g + 3 of the two-layer W stream is requested in front of step g
  auto layer = [&](int g0) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jt = 0; jt < TJT; ++jt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][jt][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < TNK; ++ks) {
      const int g = g0 + ks;
      if (g + 3 < 2 * TNK) loadb(w[(g + 3) & 3], g + 3);
      const uint4(&cur)[TJT][2] = w[g & 3];
      f16x8 b[3][TJT];
#pragma unroll
      for (int jt = 0; jt < TJT; ++jt) {
        union { uint4 q; f16x8 v; } u0, u1;
        u0.q = cur[jt][0];
        u1.q = cur[jt][1];
        b[0][jt] = u0.v;
        b[1][jt] = u1.v;
        b[2][jt] = scale_2m11(u0.v);
      }
      const uint32_t *pa = lds + ks * TKSTEP;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f16x8 ah = frag_f16(pa + slot_dw(i * 32 + l31, lh)), al = frag_f16(pa + TPLANE + slot_dw(i * 32 + l31, lh));
#pragma unroll
        for (int jt = 0; jt < TJT; ++jt) {
          acc[i][jt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, b[2][jt], acc[i][jt], 0, 0, 0);  // lo(x) hi(w)
          acc[i][jt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b[1][jt], acc[i][jt], 0, 0, 0);  // hi(x) lo(w)
          acc[i][jt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b[0][jt], acc[i][jt], 0, 0, 0);  // hi(x) hi(w)
        }
      }
    }
  };

  // ---- fc_1 ----
  layer(0);
  __syncthreads();   // every wave is done with the h0 planes
  {
    // accumulator register r of lane (lh, l31): row i 32 + (r & 3) + 8 (r >> 2) + 4 lh, column 32 TJT wc + 32 jt + l31.  Registers 2p and
    // 2p + 1 are two consecutive rows of ONE column; the planes want two consecutive columns of one row in a dword, so lane pairs
    // trade: the even lane keeps row 2p of columns (n, n + 1), the odd lane row 2p + 1 of columns (n - 1, n).
    const float inv = w_scale(amax1[0], true);
    const int odd = l31 & 1;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jt = 0; jt < TJT; ++jt) {
        const int n = 32 * TJT * wc + jt * 32 + l31, c = n & ~1;
        const float bv = b1[n];
        const int koff = (c >> 4) * TKSTEP + ((c & 7) >> 1), sub = (c & 15) >> 3;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
          const int row = i * 32 + ((2 * p) & 3) + 8 * ((2 * p) >> 2) + 4 * lh;
          const float v0 = fmaxf(acc[i][jt][2 * p] * inv + bv, 0.f), v1 = fmaxf(acc[i][jt][2 * p + 1] * inv + bv, 0.f);
          // streaming stores: h1 is read once, by the backward
          if (m0 + row < M) __builtin_nontemporal_store(v0, H1 + (m0 + row) * ldh1 + n);
          if (m0 + row + 1 < M) __builtin_nontemporal_store(v1, H1 + (m0 + row + 1) * ldh1 + n);
          const float got = lane_xor1(odd ? v0 : v1);
          uint32_t hi, lo;
          split_x(odd ? got : v0, odd ? v1 : got, hi, lo);
          const int off = koff + slot_dw(row + odd, sub);
          lds[off] = hi;
          lds[TPLANE + off] = lo;
        }
      }
  }
  __syncthreads();   // the h1 planes are complete

  // ---- fc_2 ----
  layer(TNK);
  __syncthreads();   // every wave is done with the h1 planes: the region becomes the f32 tile of h2
  float *ct = reinterpret_cast<float *>(lds);
  {
    const float inv = w_scale(amax2[0], true);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jt = 0; jt < TJT; ++jt) {
        const int n = 32 * TJT * wc + jt * 32 + l31;
        const float bv = b2[n];
#pragma unroll
        for (int r = 0; r < 16; ++r)
          ct[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * TH + n] = fmaxf(acc[i][jt][r] * inv + bv, 0.f);
      }
  }
  __syncthreads();

  // ---- h2 out, fc_out: fc_out_fwd_kernel's sum (gemm.hip), term for term ----
  const int sub = t & 15;
  float4 c4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) c4[j] = *reinterpret_cast<const float4 *>(wo + sub * 4 + 64 * j);
#pragma unroll
  for (int pass = 0; pass < TTM * 16 / TNT; ++pass) {
    // fc_out_fwd_kernel as built rounds every product and every sum (v_pk_mul_f32, v_add_f32: nothing contracted); stated here
    // so that this unit's flags cannot decide otherwise
#pragma clang fp contract(off)
    const int row = (t >> 4) + (TNT / 16) * pass;
    const int64_t m = m0 + row;
    float s = 0.f;
    if (m < M) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 a = *reinterpret_cast<const float4 *>(ct + row * TH + sub * 4 + 64 * j);
        const float4 c = c4[j];
        __builtin_nontemporal_store(f32x4{a.x, a.y, a.z, a.w}, reinterpret_cast<f32x4 *>(H2 + m * ldh2 + sub * 4 + 64 * j));
        s += a.x * c.x + a.y * c.y + a.z * c.z + a.w * c.w;
      }
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (m < M && sub == 0) logits[row_map ? (int64_t)row_map[m] : m] = s + bo[0];
  }
}

bool al16(const void *p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0 && ld >= TH; }

}  // namespace

extern "C" int64_t svr_mlp_tail_fwd_workspace(int64_t hidden) {
  if (hidden != kMlpTailHidden) return SVR_E_UNSUPPORTED;
  return ws_measure(mlp_tail_layout, hidden);
}

extern "C" int svr_mlp_tail_fwd(const float *h0, int64_t ldh0, const float *W1, const float *b1, const float *W2, const float *b2,
                                const float *w_out, const float *b_out, float *h1, int64_t ldh1, float *h2, int64_t ldh2,
                                float *logits, const int32_t *row_map, int64_t M, int64_t hidden, void *workspace, void *stream) {
  // h0 == NULL: PREPARE only (W1, W2 -> scale + split planes in the workspace);  W1 == NULL: RUN on a workspace prepared earlier
  SVR_CHECK(hidden == kMlpTailHidden, SVR_E_UNSUPPORTED, "mlp_tail_fwd: hidden %ld (the kernel is built for %ld)", (long)hidden,
            (long)kMlpTailHidden);
  SVR_CHECK((h0 || W1) && (!W1 == !W2) && workspace, SVR_E_BADARG, "mlp_tail_fwd: null pointer");
  if (h0 && M > 0) {   // the operand checks of a RUN, in front of anything that is enqueued
    SVR_CHECK(b1 && b2 && w_out && b_out && h1 && h2 && logits, SVR_E_BADARG, "mlp_tail_fwd: null pointer");
    SVR_CHECK(al16(h0, ldh0) && al16(h1, ldh1) && al16(h2, ldh2) && ((uintptr_t)w_out & 15) == 0, SVR_E_UNSUPPORTED,
              "mlp_tail_fwd: rows must be 16-byte aligned, leading dimensions multiples of 4 (ldh0=%ld ldh1=%ld ldh2=%ld)", (long)ldh0,
              (long)ldh1, (long)ldh2);
  }
  hipStream_t s = (hipStream_t)stream;
  WsCursor c(workspace);
  const MlpTailWs ws = mlp_tail_layout(c, hidden);
  if (W1) {
    const float *W[2] = {W1, W2};
    for (int l = 0; l < 2; ++l) {
      w_amax_launch(W[l], hidden, hidden, hidden, ws.amax[l], s);
      hipLaunchKernelGGL(mlp_tail_split_w_kernel, dim3(TH / 64, TH), dim3(64), 0, s, W[l], hidden, ws.amax[l], ws.planes[l]);
    }
  }
  if (!h0) return launch_status("mlp_tail_fwd (prepare)");
  if (M <= 0) return launch_status("mlp_tail_fwd");   // empty point set
  static const hipError_t lds_attr =   // once per process (an immutable kernel attribute)
      hipFuncSetAttribute((const void *)mlp_tail_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, T_LDS_BYTES);
  SVR_CHECK(lds_attr == hipSuccess, (int)lds_attr, "mlp_tail_fwd: cannot reserve %d bytes of LDS: %s", T_LDS_BYTES,
            hipGetErrorString(lds_attr));
  hipLaunchKernelGGL(mlp_tail_kernel, dim3((unsigned)cdiv(M, TTM)), dim3(TNT), T_LDS_BYTES, s, h0, ldh0, ws.planes[0], ws.amax[0], b1,
                     ws.planes[1], ws.amax[1], b2, w_out, b_out, h1, ldh1, h2, ldh2, logits, row_map, M);
  return launch_status("mlp_tail_fwd");
}
