// 3x3x3 convolution on the bf16 matrix cores, gfx950: backward-data with the 3-term split ("bf16x3") and
// forward with the 6-product split ("bf16x6", f32-equivalent accuracy: x = hi + mid + lo, see gemm_bf16x6.hip).
//
// Same brick structure as conv3d_brick_kernel (conv3d.hip): one workgroup = one 4x4x8 output brick, wave w =
// z-slice w (32 voxels = one MFMA row tile); per 32-channel chunk the input halo tile (6x6x10 voxels) is staged
// in LDS once -- here split on the way in into hi/mid bf16 planes [voxel][ci] -- and serves all 27 taps; the
// tap's weight slice [co][ci] (pre-split planes, packed once per step) is double buffered in LDS.
//   x = hi + mid, products hi*hi + hi*mid + mid*hi, f32 accumulation in v_mfma_f32_32x32x16_bf16:
//   ~1.5e-5 relative per product (see gemm_bf16x3.hip for why that is harmless in the BACKWARD pass), at a
//   fraction of the exact-f32 MFMA cycles (6 x 32 cycles per 32x32x32 block instead of 16 x 64).
// bf16x3 is used only for dIn = conv^T(dOut).  The production forward is the f16 split (F16 = true: f16x3.h /
// gemm_f16x3.hip, f32-level accuracy for |x| < 65504 at three products); bf16x6 (three planes, six products, any
// f32 range) stays selectable.  Both forwards are held to the exact-f32 kernel's gate.
#include "common.h"
#include <cstdlib>
#include "f16x3.h"

using namespace svr;

namespace {

struct ConvShape {
  int B, D, H, W, Ci, Co;
};

constexpr int BRZ = 4, BRY = 4, BRX = 8;
constexpr int HLZ = BRZ + 2, HLY = BRY + 2, HLX = BRX + 2, HLV = HLZ * HLY * HLX;

// LDS layout of the operand tiles (round 3): rows of SL = CK/8 16-byte slots, slot_dw<SL> / frag_f16 / frag_bf16 of f16x3.h
// (one ds_read_b128 per fragment, conflict free when the 16 lanes of a group hit 16 different slots mod 16):
//   weight tile: row = output column = lane & 31 -> the rows of a group pair up at distances 8 and 24;
//   halo tile:   x pitch HP = 12 voxels and the lane -> voxel map of tile_vy / tile_vx below: a group holds two complete
//                x-rows of 8 voxels, y and y + 2, i.e. rows r .. r+7 and r+24 .. r+31 for EVERY tap shift (the shift adds a
//                constant to all rows; an odd multiple of 8 flips bit 3 whatever the constant is).
constexpr int HP = 12;
// voxel (y, x) of the 4 x 8 tile held by MFMA row m (= lane & 31 of the A operand, = the accumulator's row index)
__device__ __forceinline__ int tile_vy(int m) { return (0x32230110u >> ((m >> 2) * 4)) & 3; }
__device__ __forceinline__ int tile_vx(int m) { return ((m >> 3) & 1) * 4 + (m & 3); }

// W (Co,Ci,3,3,3) f32 -> weight planes [plane][27][R][K] of 16-bit values (ps = 27 R K per plane), one thread per pair along K:
//   forward (BWD = false):  [27][Co][Ci], row = output channel, k = input channel;
//   backward-data (BWD):    [27][Ci][Co], row = ORIGINAL input channel (the output channel of the transposed conv), k = original
//                           output channel, taps flipped.
// F16: the scaled f16 split, hi(W 2^s), lo(W 2^s) (f16x3.h / gemm_f16x3.hip; "f16x3" forward, "f16x3s" backward-data);
// else bf16: hi, mid (backward-data, "bf16x3") or hi, mid, lo (forward, "bf16x6").
template <bool F16, bool BWD>
__global__ void pack_planes_kernel(const float *__restrict__ W, const uint32_t *__restrict__ amax, uint16_t *__restrict__ p0,
                                   int64_t ps, int Ci, int Co) {
  const int R = BWD ? Ci : Co, K = BWD ? Co : Ci;
  int idx = blockIdx.x * blockDim.x + threadIdx.x;  // over (tap, r, k/2)
  if (idx >= 27 * R * (K / 2)) return;
  const int k = (idx % (K / 2)) * 2;
  const int r = (idx / (K / 2)) % R;
  const int tap = idx / ((K / 2) * R);
  const size_t src = BWD ? ((size_t)k * Ci + r) * 27 + (26 - tap) : ((size_t)r * Ci + k) * 27 + tap;
  const float w0 = W[src], w1 = W[src + (BWD ? (size_t)Ci * 27 : 27)];   // (co, ci) and its neighbour along k
  const size_t o = ((size_t)tap * R + r) * K + k;
  uint32_t a, b, c = 0;
  if constexpr (F16) {
    const float sc = w_scale(amax[0], false);
    split_w(w0 * sc, w1 * sc, a, b);
  } else if constexpr (BWD) {
    split2(w0, w1, a, b);
  } else {
    split3(w0, w1, a, b, c);
    *reinterpret_cast<uint32_t *>(p0 + 2 * ps + o) = c;
  }
  *reinterpret_cast<uint32_t *>(p0 + o) = a;
  *reinterpret_cast<uint32_t *>(p0 + ps + o) = b;
}

// out(B,D,H,W,NOUT) = epi( sum_{tap,k} in[voxel+tap][k] * P[tap][n][k] ), K = s.Ci input channels of THIS call,
// NOUT = s.Co.  planes: hi then mid, each [27][NOUT][K] bf16.
// NP = 2: products mid*hi + hi*mid + hi*hi (bf16x3);  NP = 3: the six products of bf16x6;
// F16 (NP = 2): the f16 split of gemm_f16x3.hip -- planes hi / lo*2^11 of the input, hi / lo of the normalised
// weights, products lo'(x) wq + hi(x) lo(w) + hi(x) hi(w) with wq = hi(w) 2^-11 made in registers, epilogue * 2^-s.
// VT = z-slices (32-voxel row tiles) per wave: with VT = 2 the brick is 8x4x8 and every weight fragment read from LDS
// feeds two MFMA tiles (these kernels are LDS-bandwidth bound: 1.33 -> 1.0 KB of fragment reads per MFMA at Co = 32).
template <int CK, int TNB, int NP, bool F16 = false, int VT = 1>
__global__ __launch_bounds__(256) void conv3d_brick_x3_kernel(const float *__restrict__ in,
                                                              const uint16_t *__restrict__ P0,
                                                              int64_t plane_stride, const float *__restrict__ bias,
                                                              float *__restrict__ out, const float *__restrict__ mask,
                                                              ConvShape s, int nbz, int nby, int nbx, int mode,
                                                              const uint32_t *__restrict__ amax = nullptr,
                                                              double *__restrict__ spart = nullptr,
                                                              const uint32_t *__restrict__ amax_in = nullptr,
                                                              uint32_t *__restrict__ amax_out = nullptr) {
  // amax_in (F16 only; the backward-data product of the scaled f16 split, "f16x3s"): |max| of the input (a gradient): it is
  // multiplied by the exact power of two that brings that into [2^13, 2^14) on the way into the split, the epilogue divides
  // again; amax_out: |max| of what this launch stored (the next layer's scale without a pass over the tensor)
  float sin = 1.f;
  if constexpr (F16) sin = amax_in ? w_scale(amax_in[0], false) : 1.f;
  float vmax = 0.f;
  constexpr int BZ = BRZ * VT, HV = (BZ + 2) * HLY * HLX;  // brick depth and halo voxels of this instantiation
  constexpr int SL = CK / 8, XW = SL * 4;    // 16-byte slots / dwords per LDS row (CK 16-bit values, no padding: slot_dw)
  constexpr int HR = (BZ + 2) * HLY * HP;    // halo rows in LDS (x pitch HP)
  constexpr int NC = TNB * 32;               // output columns of this workgroup
  constexpr int TG = TNB == 1 ? 3 : 1;       // taps per barrier
  constexpr int KS = CK / 16;                // MFMA k sub-steps per chunk
  constexpr int PIECES = TG * NP * NC * (CK / 8);  // 16-byte pieces per weight group
  constexpr int WPT = (PIECES + 255) / 256;
  __shared__ __attribute__((aligned(16))) uint32_t sh[NP][HR * XW];        // halo tile, hi / mid (/ lo) planes: [voxel row][k]
  __shared__ __attribute__((aligned(16))) uint32_t sw[2][TG][NP][NC * XW]; // weight slices: [buffer][tap][plane][n][k]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  int64_t q = blockIdx.x;
  const int bx = (int)(q % nbx); q /= nbx;
  const int by = (int)(q % nby); q /= nby;
  const int bz = (int)(q % nbz);
  const int64_t b = q / nbz;
  const int z0 = bz * BZ, y0 = by * BRY, x0 = bx * BRX;
  const int n0 = blockIdx.y * NC;
  const float *inb = in + b * (int64_t)s.D * s.H * s.W * s.Ci;
  const int hrow = ((wave + 1) * HLY + tile_vy(l31) + 1) * HP + tile_vx(l31) + 1;  // this lane's voxel (row) in the halo tile
  f32x16 acc[VT][TNB];  // tile v of this wave = z-slice wave + 4 v
#pragma unroll
  for (int v = 0; v < VT; ++v)
#pragma unroll
    for (int j = 0; j < TNB; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[v][j][r] = 0.f;

  // weight slices travel global -> registers -> LDS two steps ahead of their use (two register sets, two LDS
  // buffers): one step of MFMAs (0.2-0.3 us at Co = 32) is shorter than an L2 round trip
  uint2 wregA[WPT][2], wregB[WPT][2];
  auto wload = [&](uint2 (&wreg)[WPT][2], int k0, int tap0) {
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int idx = t + 256 * i;
      const int part = idx % (CK / 8), row = (idx / (CK / 8)) % NC, pl = (idx / (CK / 8 * NC)) % NP, tg = idx / (CK / 8 * NC * NP);
      const bool ok = idx < PIECES && n0 + row < s.Co;
      const uint16_t *base = P0 + (ok ? pl : 0) * plane_stride;
      const uint2 *p = reinterpret_cast<const uint2 *>(base + ((size_t)(tap0 + (ok ? tg : 0)) * s.Co + (ok ? n0 + row : 0)) * s.Ci + k0 + part * 8);
      wreg[i][0] = p[0];  // unconditional (clamped to piece 0 when out of range: those columns are never stored)
      wreg[i][1] = p[1];
    }
  };
  auto wstore = [&](const uint2 (&wreg)[WPT][2], int buf) {
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int idx = t + 256 * i;
      if (idx < PIECES) {
        const int part = idx % (CK / 8), row = (idx / (CK / 8)) % NC, pl = (idx / (CK / 8 * NC)) % NP, tg = idx / (CK / 8 * NC * NP);
        *reinterpret_cast<uint4 *>(&sw[buf][tg][pl][slot_dw<SL>(row, part)]) = make_uint4(wreg[i][0].x, wreg[i][0].y, wreg[i][1].x, wreg[i][1].y);
      }
    }
  };

  constexpr int STEPS = 27 / TG;
  for (int k0 = 0; k0 < s.Ci; k0 += CK) {
    wload(wregA, k0, 0);
    wload(wregB, k0, TG);
    if (k0 > 0) __syncthreads();  // previous chunk's tiles are no longer read
    // Halo tile: all loads of the chunk are issued first, unconditionally and from clamped coordinates (a load inside
    // a branch is waited for at the end of the branch, one full memory latency per iteration), zeroed afterwards.
    constexpr int HIT = (HV * (CK / 4) + 255) / 256;
    float4 hreg[HIT];
    uint64_t hok = 0;
#pragma unroll
    for (int i = 0; i < HIT; ++i) {
      const int idx = min(t + 256 * i, HV * (CK / 4) - 1);
      const int hv = idx / (CK / 4), c4 = (idx % (CK / 4)) * 4;
      const int hx = hv % HLX, hy = (hv / HLX) % HLY, hz = hv / (HLX * HLY);
      const int gz = z0 + hz - 1, gy = y0 + hy - 1, gx = x0 + hx - 1;
      if (gz >= 0 && gz < s.D && gy >= 0 && gy < s.H && gx >= 0 && gx < s.W) hok |= 1ull << i;
      const int cz = min(max(gz, 0), s.D - 1), cy = min(max(gy, 0), s.H - 1), cx = min(max(gx, 0), s.W - 1);
      hreg[i] = *reinterpret_cast<const float4 *>(inb + (((int64_t)cz * s.H + cy) * s.W + cx) * s.Ci + k0 + c4);
    }
#pragma unroll
    for (int i = 0; i < HIT; ++i) {
      const int idx = t + 256 * i;
      if (idx >= HV * (CK / 4)) break;
      const int hv = idx / (CK / 4), c4 = (idx % (CK / 4)) * 4;
      const int hd = slot_dw<SL>((hv / HLX) * HP + hv % HLX, c4 / 8) + (c4 % 8) / 2;   // (hz*HLY + hy)*HP + hx; half a slot
      const bool ok = (hok >> i) & 1ull;
      const float4 v = make_float4(ok ? hreg[i].x : 0.f, ok ? hreg[i].y : 0.f, ok ? hreg[i].z : 0.f, ok ? hreg[i].w : 0.f);
      uint32_t h0, m0, l0 = 0, h1, m1, l1 = 0;
      if constexpr (NP == 3) {
        split3(v.x, v.y, h0, m0, l0);
        split3(v.z, v.w, h1, m1, l1);
        *reinterpret_cast<uint2 *>(&sh[NP - 1][hd]) = make_uint2(l0, l1);
      } else if constexpr (F16) {
        split_x(v.x * sin, v.y * sin, h0, m0);
        split_x(v.z * sin, v.w * sin, h1, m1);
      } else {
        split2(v.x, v.y, h0, m0);
        split2(v.z, v.w, h1, m1);
      }
      *reinterpret_cast<uint2 *>(&sh[0][hd]) = make_uint2(h0, h1);
      *reinterpret_cast<uint2 *>(&sh[1][hd]) = make_uint2(m0, m1);
    }
    wstore(wregA, 0);
    __syncthreads();
    // step st: MFMAs on LDS buffer st & 1; `nxt` holds step st+1 (in flight since step st-1), `fre` is refilled with st+2
    auto step = [&](int st, uint2 (&nxt)[WPT][2], uint2 (&fre)[WPT][2]) {
      const int buf = st & 1, tap0 = st * TG;
      if (st + 2 < STEPS) wload(fre, k0, tap0 + 2 * TG);
#pragma unroll
      for (int tg = 0; tg < TG; ++tg) {
        const int tap = tap0 + tg;
        const int arow = hrow + ((tap / 9 - 1) * HLY + ((tap / 3) % 3 - 1)) * HP + (tap % 3 - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int sub = ks * 2 + lh;
          int aoff[VT], woff[TNB];
#pragma unroll
          for (int v = 0; v < VT; ++v) aoff[v] = slot_dw<SL>(arow + v * BRZ * HLY * HP, sub);
#pragma unroll
          for (int j = 0; j < TNB; ++j) woff[j] = slot_dw<SL>(j * 32 + l31, sub);
          if constexpr (F16) {
            f16x8 xh[VT], xl[VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) {
              xh[v] = frag_f16(&sh[0][aoff[v]]);
              xl[v] = frag_f16(&sh[1][aoff[v]]);
            }
#pragma unroll
            for (int j = 0; j < TNB; ++j) {
              const f16x8 wh = frag_f16(&sw[buf][tg][0][woff[j]]);
              const f16x8 wl = frag_f16(&sw[buf][tg][1][woff[j]]);
              const f16x8 wq = scale_2m11(wh);
#pragma unroll
              for (int v = 0; v < VT; ++v) {
                acc[v][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl[v], wq, acc[v][j], 0, 0, 0);
                acc[v][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh[v], wl, acc[v][j], 0, 0, 0);
                acc[v][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh[v], wh, acc[v][j], 0, 0, 0);
              }
            }
            continue;
          }
          bf16x8 ah[VT], am[VT];
#pragma unroll
          for (int v = 0; v < VT; ++v) {
            ah[v] = frag_bf16(&sh[0][aoff[v]]);
            am[v] = frag_bf16(&sh[1][aoff[v]]);
          }
#pragma unroll
          for (int j = 0; j < TNB; ++j) {
            const bf16x8 bh = frag_bf16(&sw[buf][tg][0][woff[j]]);
            const bf16x8 bm = frag_bf16(&sw[buf][tg][1][woff[j]]);
#pragma unroll
            for (int v = 0; v < VT; ++v) {
              if constexpr (NP == 3) {
                const bf16x8 al = frag_bf16(&sh[NP - 1][aoff[v]]);
                const bf16x8 bl = frag_bf16(&sw[buf][tg][NP - 1][woff[j]]);
                acc[v][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[v][j], 0, 0, 0);
                acc[v][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[v], bl, acc[v][j], 0, 0, 0);
                acc[v][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[v], bm, acc[v][j], 0, 0, 0);
              }
              acc[v][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[v], bh, acc[v][j], 0, 0, 0);
              acc[v][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[v], bm, acc[v][j], 0, 0, 0);
              acc[v][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[v], bh, acc[v][j], 0, 0, 0);
            }
          }
        }
      }
      if (st + 1 < STEPS) wstore(nxt, buf ^ 1);
      __syncthreads();
    };
    for (int st = 0; st < STEPS; st += 2) {
      step(st, wregB, wregA);
      if (st + 1 < STEPS) step(st + 1, wregA, wregB);
    }
  }
  // BatchNorm statistics of what this workgroup stores (spart: per-workgroup partial sums [brick][2][Co] in f64): the
  // stage's last convolution delivers them and the separate statistics pass over its output disappears
  float ssum[TNB], ssq[TNB];
#pragma unroll
  for (int j = 0; j < TNB; ++j) ssum[j] = ssq[j] = 0.f;
#pragma unroll
  for (int v = 0; v < VT; ++v)
#pragma unroll
  for (int j = 0; j < TNB; ++j) {
    const int n = n0 + j * 32 + l31;
    const int nc = min(n, s.Co - 1);
    const float bv = (mode == SVR_EPI_BIAS || mode == SVR_EPI_BIAS_RELU) ? bias[nc] : 0.f;
    const float inv = F16 ? w_scale(amax[0], true) * (amax_in ? w_scale(amax_in[0], true) : 1.f) : 1.f;
    const int gz = z0 + wave + BRZ * v;
    // the ReLU mask of the whole tile is fetched up front from clamped coordinates: loads inside the bounds
    // branch would be waited for one at a time
    float mk[16];
    if (mode == SVR_EPI_MASK) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const int cy = min(y0 + tile_vy(i), s.H - 1), cx = min(x0 + tile_vx(i), s.W - 1), cz = min(gz, s.D - 1);
        mk[r] = mask[((((int64_t)b * s.D + cz) * s.H + cy) * s.W + cx) * s.Co + nc];
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = (r & 3) + 8 * (r >> 2) + 4 * lh;
      const int gy = y0 + tile_vy(i), gx = x0 + tile_vx(i);
      if (n < s.Co && gz < s.D && gy < s.H && gx < s.W) {
        const int64_t o = ((((int64_t)b * s.D + gz) * s.H + gy) * s.W + gx) * s.Co + n;
        float val = (F16 ? acc[v][j][r] * inv : acc[v][j][r]) + bv;
        if (mode == SVR_EPI_BIAS_RELU) val = fmaxf(val, 0.f);
        if (mode == SVR_EPI_MASK) val = mk[r] > 0.f ? val : 0.f;
        // streaming store: the layer's output (268 MB at 64^3 x 32) should not push the halo voxels its neighbours re-read out of
        // L2 (conv forward 1.39 -> 1.37, backward-data 1.54 -> 1.52 ms per step)
        __builtin_nontemporal_store(val, out + o);
        ssum[j] += val;
        ssq[j] = fmaf(val, val, ssq[j]);
        vmax = fmaxf(vmax, fabsf(val));
      }
    }
  }
  if (amax_out) {  // (uniform)
svr_amax_publish(amax_out, vmax);
  }
  if (spart) {  // (uniform) lanes l31 / l31 + 32 of the four waves hold the same channel: fixed-order f64 sum of the 8 partials
    float *red = reinterpret_cast<float *>(&sw[0][0][0][0]);   // the weight buffers are free now: [thread][TNB][2] floats
    static_assert(sizeof(sw) >= 256 * TNB * 2 * sizeof(float), "weight buffer too small for the statistics reduction");
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TNB; ++j) {
      red[(t * TNB + j) * 2] = ssum[j];
      red[(t * TNB + j) * 2 + 1] = ssq[j];
    }
    __syncthreads();
    if (t < 2 * NC) {
      const int which = t / NC, col = t % NC, j = col / 32, c31 = col % 32;
      double acc = 0.0;
#pragma unroll
      for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int h = 0; h < 2; ++h) acc += (double)red[(((w * 64 + h * 32 + c31) * TNB) + j) * 2 + which];
      if (n0 + col < s.Co) spart[((int64_t)blockIdx.x * 2 + which) * s.Co + n0 + col] = acc;
    }
  }
}


// ---------------------------------------------------------------------------------------------------------------------
// PERSISTENT form of the brick kernel for 32 output columns (TNB = 1), round 3.  Measurement builds of the kernel above
// (no MFMAs / no halo loads / halo loads not waited for: profiles/r03_conv_variants.txt; no longer in
// the tree) showed that at 64^3 the matrix instructions are completely hidden
// (no MFMAs: same time), that the halo tile's global loads cost 19-23 % and that half of that is the WAIT for them: a
// workgroup that stages a chunk computes nothing, and with two workgroups per CU the other one then has each SIMD to itself,
// one wave that stalls on every LDS fragment read.  Here a workgroup walks bricks (grid = the resident workgroups) and the
// NEXT work item's halo tile -- the next 16 / 32-channel chunk of the brick or the first chunk of the next brick -- is
// fetched into registers before the current item's MFMA steps and split into LDS behind them; the weight pipeline (two
// register sets, two steps ahead) runs straight through the item boundaries: an item is TEN barrier steps (taps 3 3 3 3 3 3
// 3 2 2 2), an even number, so the two register sets keep their roles from one item to the next.
// ---------------------------------------------------------------------------------------------------------------------
template <int CK, bool F16, int VT>
__global__ __launch_bounds__(256, 2) void conv3d_brick_p_kernel(const float *__restrict__ in, const uint16_t *__restrict__ P0,
                                                             int64_t plane_stride, const float *__restrict__ bias,
                                                             float *__restrict__ out, const float *__restrict__ mask,
                                                             ConvShape s, int nbz, int nby, int nbx, int nbricks, int mode,
                                                             const uint32_t *__restrict__ amax, double *__restrict__ spart,
                                                             const uint32_t *__restrict__ amax_in, uint32_t *__restrict__ amax_out) {
  float sin = 1.f;   // (see conv3d_brick_x3_kernel)
  if constexpr (F16) sin = amax_in ? w_scale(amax_in[0], false) : 1.f;
  float vmax = 0.f;
  constexpr int NP = 2, NC = 32, TG = 3, STEPS = 10;
  constexpr int BZ = BRZ * VT, HV = (BZ + 2) * HLY * HLX;
  constexpr int SL = CK / 8, XW = SL * 4, HR = (BZ + 2) * HLY * HP, KS = CK / 16;
  constexpr int PIECES = TG * NP * NC * (CK / 8), WPT = (PIECES + 255) / 256;
  constexpr int HIT = (HV * (CK / 4) + 255) / 256;
  static_assert(CK == 16, "the piece -> (tap, plane, row, part) split below is written out for 16-channel chunks");
  __shared__ __attribute__((aligned(16))) uint32_t sh[NP][HR * XW];
  __shared__ __attribute__((aligned(16))) uint32_t sw[2][TG][NP][NC * XW];
  static_assert(sizeof(sh) >= 256 * 2 * sizeof(float), "halo buffer too small for the statistics reduction");
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int n0 = blockIdx.y * NC;
  const int hrow = ((wave + 1) * HLY + tile_vy(l31) + 1) * HP + tile_vx(l31) + 1;
  const int nch = s.Ci / CK;
  const int nmy = (nbricks - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;   // bricks of this workgroup (>= 1: grid <= bricks)
  const int nitems = nmy * nch;

  // ADDRESS ARITHMETIC (round 3, SQ counters: this kernel issued 1 520 vector-ALU instructions per item and wave next to 162
  // MFMAs -- 44 % + 38 % of the SIMDs' time, and the two add up; a fifth of them were 32 / 64-bit integer multiplies of the
  // flat index arithmetic).  Everything below is 32-bit: wave-uniform bases (SGPRs) + per-lane offsets inside ONE sample
  // (host: D H W <= 2^24 voxels and D H W max(Ci, Co) < 2^30 elements, so v_mad_u32_u24 is exact and byte offsets fit),
  // and what only depends on the thread is computed once, in front of the item loop.
  const uint32_t HW = (uint32_t)(s.H * s.W);

  f32x16 acc[VT];
#pragma unroll
  for (int v = 0; v < VT; ++v)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[v][r] = 0.f;

  struct Item { int b, z0, y0, x0, k0, brick; };
  auto decode = [&](int it) {   // (wave-uniform: scalar unit)
    Item I;
    const int bi = it / nch;
    I.k0 = (it - bi * nch) * CK;
    I.brick = (int)blockIdx.x + bi * (int)gridDim.x;
    int q = I.brick;
    I.x0 = (q % nbx) * BRX; q /= nbx;
    I.y0 = (q % nby) * BRY; q /= nby;
    I.z0 = (q % nbz) * BZ;
    I.b = q / nbz;
    return I;
  };

  // ---- weights: piece 0 of a thread = (tap tg0 of the step, plane, row, 8-channel part), piece 1 (threads < 128) = the
  // step's third tap; step st of an item covers taps tap0(st) .. + 2 (the last three steps: + 1, no piece 1)
  const int p0part = t & 1, p0row = (t >> 1) & 31, p0pl = (t >> 6) & 1, p0tg = t >> 7;
  const bool rowok = n0 + p0row < s.Co;
  const uint32_t wtap = (uint32_t)(s.Co * s.Ci) * 2u;                             // bytes per tap of one plane
  const uint32_t wrow = (uint32_t)((rowok ? n0 + p0row : 0) * s.Ci + p0part * 8) * 2u;
  const uint32_t wof0 = (uint32_t)p0pl * (uint32_t)plane_stride * 2u + (uint32_t)p0tg * wtap + wrow;   // + (tap0 Co Ci + k0) * 2
  const uint32_t wof1 = (uint32_t)((t >> 6) & 1) * (uint32_t)plane_stride * 2u + 2u * wtap + wrow;      // piece 1: tg = 2, plane = (t >> 6) & 1
  const int wst0 = (int)(&sw[0][p0tg][p0pl][slot_dw<SL>(p0row, p0part)] - &sw[0][0][0][0]);
  const int wst1 = (int)(&sw[0][2][(t >> 6) & 1][slot_dw<SL>(p0row, p0part)] - &sw[0][0][0][0]);
  constexpr int WBUF = TG * NP * NC * XW;   // dwords per weight buffer
  static_assert(PIECES == 384 && WPT == 2, "pieces 0 (256 threads) and 1 (128 threads)");
  // (scalars, not arrays: a two-element array with a conditionally written element was demoted to LDS by the compiler)
  struct WReg { uint4 p0, p1; };
  WReg wregA, wregB;
  wregA.p1 = wregB.p1 = make_uint4(0u, 0u, 0u, 0u);
  const char *Pb = reinterpret_cast<const char *>(P0);
  auto wload = [&](WReg &wreg, int k0, int st) {
    const int tap0 = st < 7 ? 3 * st : 21 + 2 * (st - 7);
    const uint32_t sb = (uint32_t)tap0 * wtap + (uint32_t)k0 * 2u;   // (uniform)
    wreg.p0 = *reinterpret_cast<const uint4 *>(Pb + (wof0 + sb));
    if (st < 7) wreg.p1 = *reinterpret_cast<const uint4 *>(Pb + (wof1 + sb));   // (compile time: the two-tap steps have no third tap)
  };
  auto wstore = [&](const WReg &wreg, int buf, int st_of_data) {
    uint32_t *base = &sw[0][0][0][0] + buf * WBUF;
    *reinterpret_cast<uint4 *>(base + wst0) = wreg.p0;
    if (st_of_data < 7 && t < 128) *reinterpret_cast<uint4 *>(base + wst1) = wreg.p1;
  };

  // ---- halo tile of an item: global -> registers (unconditional, clamped coordinates), later registers -> split -> LDS.
  // Per piece the thread's halo voxel (hz, hy, hx) and its LDS offset are constants: packed once (8 + 8 + 8 + 8 bits would
  // not hold the LDS offset: two packed registers per piece would cost 20 VGPRs; the LDS offset is recomputed, 6 VALU)
  constexpr int C4 = CK / 4;
  const int c4 = (t % C4) * 4;   // (256 % C4 == 0: the same channel quad in every piece)
  float4 hreg[HIT];
  uint32_t hok = 0;
  auto halo_vox = [&](int i, int &hz, int &hy, int &hx) {   // compile-time i: constants folded per piece, t-dependent part small
    const int idx = min(t + 256 * i, HV * C4 - 1);
    const int hv = idx / C4;
    hx = hv % HLX;
    const int q = hv / HLX;
    hy = q % HLY;
    hz = q / HLY;
  };
  // (hz, hy, hx) of every piece, packed: 5 + 3 + 4 bits
  int hpk[HIT];
#pragma unroll
  for (int i = 0; i < HIT; ++i) {
    int hz, hy, hx;
    halo_vox(i, hz, hy, hx);
    hpk[i] = hz | (hy << 5) | (hx << 8);
  }
  auto halo_load = [&](const Item &I, int i0, int i1) {
    const char *inb = reinterpret_cast<const char *>(in + (int64_t)I.b * s.D * s.H * s.W * s.Ci);   // (uniform)
    if (i0 == 0) hok = 0;
#pragma unroll
    for (int i = i0; i < i1; ++i) {
      const int gz = I.z0 - 1 + (hpk[i] & 31), gy = I.y0 - 1 + ((hpk[i] >> 5) & 7), gx = I.x0 - 1 + (hpk[i] >> 8);
      if ((unsigned)gz < (unsigned)s.D && (unsigned)gy < (unsigned)s.H && (unsigned)gx < (unsigned)s.W) hok |= 1u << i;
      const uint32_t cz = (uint32_t)min(max(gz, 0), s.D - 1), cy = (uint32_t)min(max(gy, 0), s.H - 1), cx = (uint32_t)min(max(gx, 0), s.W - 1);
      const uint32_t vox = __umul24(__umul24(cz, (uint32_t)s.H) + cy, (uint32_t)s.W) + cx;
      const uint32_t off = (__umul24(vox, (uint32_t)s.Ci) + (uint32_t)(I.k0 + c4)) * 4u;
      hreg[i] = *reinterpret_cast<const float4 *>(inb + off);
    }
  };
  auto halo_store = [&]() {
#pragma unroll
    for (int i = 0; i < HIT; ++i) {
      if (t + 256 * i >= HV * C4) break;
      const int row = ((hpk[i] & 31) * HLY + ((hpk[i] >> 5) & 7)) * HP + (hpk[i] >> 8);
      const int hd = slot_dw<SL>(row, c4 / 8) + (c4 % 8) / 2;
      const bool ok = (hok >> i) & 1u;
      const float4 v = make_float4(ok ? hreg[i].x : 0.f, ok ? hreg[i].y : 0.f, ok ? hreg[i].z : 0.f, ok ? hreg[i].w : 0.f);
      uint32_t h0, m0, h1, m1;
      if constexpr (F16) {
        split_x(v.x * sin, v.y * sin, h0, m0);
        split_x(v.z * sin, v.w * sin, h1, m1);
      } else {
        split2(v.x, v.y, h0, m0);
        split2(v.z, v.w, h1, m1);
      }
      *reinterpret_cast<uint2 *>(&sh[0][hd]) = make_uint2(h0, h1);
      *reinterpret_cast<uint2 *>(&sh[1][hd]) = make_uint2(m0, m1);
    }
  };

  // ---- epilogue of a finished brick (the kernel above's, for TNB = 1); the accumulators start the next brick at zero.
  // Element offset of result r = (uniform voxel base + lane part) * Co + n: the lane part (vy W + vx) of the 16 results is
  // one of two compile-time tables (lh), the voxel base is scalar
  auto epilogue = [&](const Item &I) {
    float ssum = 0.f, ssq = 0.f;
    const int n = n0 + l31, nc = min(n, s.Co - 1);
    const float bv = (mode == SVR_EPI_BIAS || mode == SVR_EPI_BIAS_RELU) ? bias[nc] : 0.f;
    const float inv = F16 ? w_scale(amax[0], true) * (amax_in ? w_scale(amax_in[0], true) : 1.f) : 1.f;
    const bool interior = I.z0 + BZ <= s.D && I.y0 + BRY <= s.H && I.x0 + BRX <= s.W && n0 + NC <= s.Co;   // (uniform)
    char *outb = reinterpret_cast<char *>(out + (int64_t)I.b * s.D * s.H * s.W * s.Co);
    const char *maskb = reinterpret_cast<const char *>(mask + (mode == SVR_EPI_MASK ? (int64_t)I.b * s.D * s.H * s.W * s.Co : 0));
#pragma unroll
    for (int v = 0; v < VT; ++v) {
      const int gz = I.z0 + wave + BRZ * v;
      const uint32_t vbase = __umul24((uint32_t)min(gz, s.D - 1), HW) + __umul24((uint32_t)I.y0, (uint32_t)s.W) + (uint32_t)I.x0;   // (uniform)
      uint32_t off[16];
      bool okr[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i0 = (r & 3) + 8 * (r >> 2);                 // MFMA row of lanes 0 .. 31; lanes 32 .. 63: + 4
        const int vy = lh ? tile_vy(i0 + 4) : tile_vy(i0), vx = lh ? tile_vx(i0 + 4) : tile_vx(i0);   // two constants, one select each
        const int gy = I.y0 + vy, gx = I.x0 + vx;
        okr[r] = interior || (n < s.Co && gz < s.D && gy < s.H && gx < s.W);
        // (a voxel outside the volume gets the offset of a clamped one: never stored, its mask value never used)
        const uint32_t lv = __umul24((uint32_t)min(vy, s.H - 1 - I.y0), (uint32_t)s.W) + (uint32_t)min(vx, s.W - 1 - I.x0);
        off[r] = (__umul24(vbase + lv, (uint32_t)s.Co) + (uint32_t)nc) * 4u;
      }
      float mk[16];
      if (mode == SVR_EPI_MASK) {
#pragma unroll
        for (int r = 0; r < 16; ++r) mk[r] = *reinterpret_cast<const float *>(maskb + off[r]);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (okr[r]) {
          float val = (F16 ? acc[v][r] * inv : acc[v][r]) + bv;
          if (mode == SVR_EPI_BIAS_RELU) val = fmaxf(val, 0.f);
          if (mode == SVR_EPI_MASK) val = mk[r] > 0.f ? val : 0.f;
          __builtin_nontemporal_store(val, reinterpret_cast<float *>(outb + off[r]));
          ssum += val;
          ssq = fmaf(val, val, ssq);
          vmax = fmaxf(vmax, fabsf(val));
        }
        acc[v][r] = 0.f;
      }
    }
    if (spart) {  // (uniform) per-brick partial sums, row = brick id: the same rows as the one-brick-per-workgroup kernel writes
      float *red = reinterpret_cast<float *>(&sh[0][0]);   // the halo tile is free between an item's last step and the next store
      red[t * 2] = ssum;
      red[t * 2 + 1] = ssq;
      __syncthreads();
      if (t < 2 * NC) {
        const int which = t / NC, c31 = t % NC;
        double a2 = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
          for (int h = 0; h < 2; ++h) a2 += (double)red[(w * 64 + h * 32 + c31) * 2 + which];
        if (n0 + c31 < s.Co) spart[((int64_t)I.brick * 2 + which) * s.Co + n0 + c31] = a2;
      }
      __syncthreads();
    }
  };

  // W fragment offset of this lane inside a tap's plane (rows = output columns)
  int woff[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) woff[ks] = slot_dw<SL>(l31, ks * 2 + lh);

  Item cur = decode(0);
  halo_load(cur, 0, HIT);
  wload(wregA, cur.k0, 0);
  wload(wregB, cur.k0, 1);
  halo_store();
  wstore(wregA, 0, 0);
  __syncthreads();
  for (int it = 0; it < nitems; ++it) {
    const Item nxt = decode(it + 1 < nitems ? it + 1 : it);   // (clamped: the last item fetches itself again, never stored)
    // the 27 swizzled fragment addresses are loop invariant; hoisted out of the item loop they cost 27 VGPRs and the kernel
    // its second workgroup per CU.  Opaque per item, each is computed where it is used (4 VALU) and dies there; the second
    // z-slice of the wave sits BRZ HLY HP = 288 rows further -- a multiple of 16, so the swizzle bit is the same and its
    // address is an immediate offset
    int hrow_i = hrow;
    asm volatile("" : "+v"(hrow_i));
    // step st: MFMAs on LDS buffer st & 1; `nx` holds step st + 1 (in flight since st - 1), `fr` is refilled with st + 2
    auto step = [&](int st, WReg &nx, WReg &fr) {
      const int buf = st & 1, tap0 = st < 7 ? 3 * st : 21 + 2 * (st - 7), nt = st < 7 ? 3 : 2;
      if (st + 2 < STEPS) wload(fr, cur.k0, st + 2);
      else wload(fr, nxt.k0, st + 2 - STEPS);
      halo_load(nxt, (st * HIT) / STEPS, ((st + 1) * HIT) / STEPS);   // this step's share of the next item's halo tile
#pragma unroll
      for (int tg = 0; tg < TG; ++tg) {
        if (tg >= nt) break;
        const int tap = tap0 + tg;
        const int arow = hrow_i + ((tap / 9 - 1) * HLY + ((tap / 3) % 3 - 1)) * HP + (tap % 3 - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int sub = ks * 2 + lh;
          const int aoff = slot_dw<SL>(arow, sub);
          static_assert((BRZ * HLY * HP) % 16 == 0, "second z-slice: same swizzle");
          constexpr int VSTEP = BRZ * HLY * HP * XW;   // dwords between the wave's z-slices
          if constexpr (F16) {
            f16x8 xh[VT], xl[VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) {
              xh[v] = frag_f16(&sh[0][aoff + v * VSTEP]);
              xl[v] = frag_f16(&sh[1][aoff + v * VSTEP]);
            }
            const f16x8 wh = frag_f16(&sw[buf][tg][0][woff[ks]]);
            const f16x8 wl = frag_f16(&sw[buf][tg][1][woff[ks]]);
            const f16x8 wq = scale_2m11(wh);
#pragma unroll
            for (int v = 0; v < VT; ++v) {
              acc[v] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl[v], wq, acc[v], 0, 0, 0);
              acc[v] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh[v], wl, acc[v], 0, 0, 0);
              acc[v] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh[v], wh, acc[v], 0, 0, 0);
            }
          } else {
            bf16x8 ah[VT], am[VT];
#pragma unroll
            for (int v = 0; v < VT; ++v) {
              ah[v] = frag_bf16(&sh[0][aoff + v * VSTEP]);
              am[v] = frag_bf16(&sh[1][aoff + v * VSTEP]);
            }
            const bf16x8 bh = frag_bf16(&sw[buf][tg][0][woff[ks]]);
            const bf16x8 bm = frag_bf16(&sw[buf][tg][1][woff[ks]]);
#pragma unroll
            for (int v = 0; v < VT; ++v) {
              acc[v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[v], bh, acc[v], 0, 0, 0);
              acc[v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[v], bm, acc[v], 0, 0, 0);
              acc[v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[v], bh, acc[v], 0, 0, 0);
            }
          }
        }
      }
      wstore(nx, buf ^ 1, (st + 1) % STEPS);
      __syncthreads();
    };
#pragma unroll
    for (int st = 0; st < STEPS; st += 2) {
      step(st, wregB, wregA);
      step(st + 1, wregA, wregB);
    }
    if (cur.k0 + CK >= s.Ci) epilogue(cur);   // (uniform) the brick's last chunk
    halo_store();                              // the next item's tile, fetched during this item's steps
    __syncthreads();
    cur = nxt;
  }
  if (amax_out) {  // (uniform) |max| of everything this workgroup stored
svr_amax_publish(amax_out, vmax);
  }
}

// SVR_CONV_PERSISTENT=0: the one-brick-per-workgroup kernel everywhere (A/B switch, read once)
bool persistent_bricks(const ConvShape &sh) {
  static const bool on = !(getenv("SVR_CONV_PERSISTENT") && getenv("SVR_CONV_PERSISTENT")[0] == '0');
  // the kernel's 24-bit voxel index multiplies and 32-bit byte offsets inside one sample
  const int64_t vox = (int64_t)sh.D * sh.H * sh.W, cmax = sh.Ci > sh.Co ? sh.Ci : sh.Co;
  return on && vox <= (1LL << 24) && vox * cmax < (1LL << 30);
}
// resident workgroups of an instantiation (CUs x occupancy; cached per kernel: immutable after the first call)
template <int CK, bool F16, int VT>
int brick_p_resident() {
  static int resident = 0;
  if (resident == 0) {
    int dev = 0, cus = 256, per_cu = 2;
    if (hipGetDevice(&dev) == hipSuccess) hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, conv3d_brick_p_kernel<CK, F16, VT>, 256, 0) != hipSuccess || per_cu < 1) per_cu = 2;
    (void)hipGetLastError();
    resident = cus * per_cu;
  }
  return resident;
}
template <int CK, bool F16, int VT>
void launch_brick_p(const float *in, const uint16_t *P0, int64_t plane_stride, const float *bias, float *out, const float *mask,
                    ConvShape sh, int nbz, int nby, int nbx, int ycols, int mode, const uint32_t *amax, double *spart, hipStream_t s,
                    const uint32_t *amax_in = nullptr, uint32_t *amax_out = nullptr) {
  const int64_t bricks = (int64_t)sh.B * nbz * nby * nbx;
  int gx = brick_p_resident<CK, F16, VT>() / ycols;
  if (gx < 1) gx = 1;
  if (gx > bricks) gx = (int)bricks;
  hipLaunchKernelGGL((conv3d_brick_p_kernel<CK, F16, VT>), dim3((unsigned)gx, (unsigned)ycols), dim3(256), 0, s, in, P0, plane_stride, bias, out,
                     mask, sh, nbz, nby, nbx, (int)bricks, mode, amax, spart, amax_in, amax_out);
}

// The tile choice of the 3x3x3 launchers below, from the shape alone (svr_conv3d_k3_variant exports it).  cols = the output
// columns (Co forward, Ci backward-data), k = the reduction side.
//   tn: 32-column tiles per workgroup, as wide as the layer allows (fragment reuse) but narrower on the small volumes so
//       that the grid still has >= 512 workgroups (the 8^3 / 16^3 layers ran 32 / 256 workgroups of 108 barrier steps);
//   vt == 2: two z-slices per wave (8x4x8 bricks, 16-channel chunks, 32 columns), persistent where persistent_bricks() allows;
//   rows: grid.x of the one-brick-per-workgroup kernels = bricks of the persistent one = partial-sum rows of the stats epilogue.
struct ConvVariant {
  int ck, tn, vt, nbz, nby, nbx, ycols;
  bool persistent;
  int64_t rows;
};
ConvVariant conv_variant(int op, int B, int D, int H, int Wd, int k, int cols) {
  ConvVariant v;
  v.nbz = (int)cdiv(D, BRZ), v.nby = (int)cdiv(H, BRY), v.nbx = (int)cdiv(Wd, BRX);
  v.vt = 1, v.persistent = false;
  v.rows = (int64_t)B * v.nbz * v.nby * v.nbx;
  v.tn = cols <= 32 ? 1 : (cols <= 64 ? 2 : 4);
  if (op == SVR_CONV_FWD_BF16X6) {
    v.ck = 16;
  } else {
    while (v.tn > 1 && v.rows * cdiv(cols, v.tn * 32) < 512) v.tn /= 2;
    const int nbz2 = (int)cdiv(D, 2 * BRZ);
    const int64_t rows2 = (int64_t)B * nbz2 * v.nby * v.nbx;
    if (v.tn == 1 && rows2 * cdiv(cols, 32) >= 512) {
      v.ck = 16, v.vt = 2, v.nbz = nbz2, v.rows = rows2;
      v.persistent = persistent_bricks(ConvShape{B, D, H, Wd, k, cols});
    } else {
      v.ck = k % 32 == 0 ? 32 : 16;
    }
  }
  v.ycols = (int)cdiv(cols, v.tn * 32);
  return v;
}

}  // namespace

extern "C" int64_t svr_conv3d_bwd_data_bf16x3_workspace(int32_t Ci, int32_t Co) { return ws_measure(planes_layout, (int64_t)27 * Ci * Co, 2); }

// dIn(B,D,H,W,Ci) = epi( conv^T(dOut(B,D,H,W,Co), W(Co,Ci,3,3,3)) ), epilogue NONE or MASK (mask shaped like dIn).
extern "C" int svr_conv3d_k3_bwd_data_bf16x3(const float *dout, const float *W, float *din, int32_t B, int32_t D, int32_t H,
                                             int32_t Wd, int32_t Ci, int32_t Co, int epilogue, const float *mask,
                                             void *workspace, void *stream) {
  // dout == NULL: PREPARE only (W -> split planes in the workspace);  W == NULL: RUN on a workspace prepared earlier
  SVR_CHECK((dout || W) && (!dout || din) && workspace, SVR_E_BADARG, "conv3d_bwd_data_bf16x3: null pointer");
  SVR_CHECK(Co % 16 == 0 && Ci % 2 == 0 && Ci >= 2, SVR_E_UNSUPPORTED, "conv3d_bwd_data_bf16x3: need Co %% 16 == 0, Ci even (Ci=%d Co=%d)", Ci, Co);
  hipStream_t s = (hipStream_t)stream;
  const int64_t ps = (int64_t)27 * Ci * Co;
  WsCursor c(workspace, 16);
  uint16_t *hi = planes_layout(c, ps, 2);
  // the transposed conv reads dOut (Co channels = its K) and writes Ci channels: planes [27][Ci][Co]
  if (W) hipLaunchKernelGGL((pack_planes_kernel<false, true>), dim3(cdiv(27 * Ci * (Co / 2), 256)), dim3(256), 0, s, W, (const uint32_t *)nullptr, hi, ps, Ci, Co);
  if (!dout) return launch_status("conv3d_bwd_data_bf16x3 (prepare)");
  SVR_CHECK(B > 0 && D > 0 && H > 0 && Wd > 0, SVR_E_BADSHAPE, "conv3d_bwd_data_bf16x3: empty volume");
  SVR_CHECK(epilogue == SVR_EPI_NONE || (epilogue == SVR_EPI_MASK && mask), SVR_E_BADARG, "conv3d_bwd_data_bf16x3: epilogue %d", epilogue);
  ConvShape sh{B, D, H, Wd, /*K=*/Co, /*NOUT=*/Ci};
  const ConvVariant v = conv_variant(SVR_CONV_BWD_DATA_BF16X3, B, D, H, Wd, Co, Ci);
#define LAUNCH_X3(CKV, TNV)                                                                                               \
  hipLaunchKernelGGL((conv3d_brick_x3_kernel<CKV, TNV, 2>), dim3((unsigned)v.rows, (unsigned)v.ycols), dim3(256), 0, s, dout, \
                     hi, ps, (const float *)nullptr, din, mask, sh, v.nbz, v.nby, v.nbx, epilogue)
  if (v.persistent) {
    launch_brick_p<16, false, 2>(dout, hi, ps, nullptr, din, mask, sh, v.nbz, v.nby, v.nbx, v.ycols, epilogue, nullptr, nullptr, s);
  } else if (v.vt == 2) {
    hipLaunchKernelGGL((conv3d_brick_x3_kernel<16, 1, 2, false, 2>), dim3((unsigned)v.rows, (unsigned)v.ycols), dim3(256), 0, s, dout, hi,
                       ps, (const float *)nullptr, din, mask, sh, v.nbz, v.nby, v.nbx, epilogue);
  } else if (v.ck == 32) {
    if (v.tn == 1) LAUNCH_X3(32, 1); else if (v.tn == 2) LAUNCH_X3(32, 2); else LAUNCH_X3(32, 4);
  } else {
    if (v.tn == 1) LAUNCH_X3(16, 1); else if (v.tn == 2) LAUNCH_X3(16, 2); else LAUNCH_X3(16, 4);
  }
#undef LAUNCH_X3
  return launch_status("conv3d_bwd_data_bf16x3");
}

// ---- backward-data on the scaled f16 split ("f16x3s": f32 level at the bf16x3 cost; see svr_linear_bwd_data_f16x3) -------------
extern "C" int64_t svr_conv3d_bwd_data_f16x3_workspace(int32_t Ci, int32_t Co) { return ws_measure(scaled_planes_layout, (int64_t)27 * Ci * Co); }

extern "C" int svr_conv3d_k3_bwd_data_f16x3(const float *dout, const float *W, float *din, int32_t B, int32_t D, int32_t H,
                                            int32_t Wd, int32_t Ci, int32_t Co, int epilogue, const float *mask,
                                            const uint32_t *amax_dout, uint32_t *amax_din, void *workspace, void *stream) {
  // dout == NULL: PREPARE only (W -> scale + split planes in the workspace);  W == NULL: RUN on a workspace prepared earlier
  SVR_CHECK((dout || W) && (!dout || din) && workspace, SVR_E_BADARG, "conv3d_bwd_data_f16x3: null pointer");
  SVR_CHECK(Co % 16 == 0 && Ci % 2 == 0 && Ci >= 2, SVR_E_UNSUPPORTED, "conv3d_bwd_data_f16x3: need Co %% 16 == 0, Ci even (Ci=%d Co=%d)", Ci, Co);
  hipStream_t s = (hipStream_t)stream;
  const int64_t ps = (int64_t)27 * Ci * Co;
  WsCursor c(workspace);
  const auto [amax, hi] = scaled_planes_layout(c, ps);
  if (W) {
    w_amax_launch(W, ps, 1, ps, amax, s, (unsigned)cdiv(ps, 1024));
    hipLaunchKernelGGL((pack_planes_kernel<true, true>), dim3(cdiv(27 * Ci * (Co / 2), 256)), dim3(256), 0, s, W, (const uint32_t *)amax, hi, ps, Ci, Co);
  }
  if (!dout) return launch_status("conv3d_bwd_data_f16x3 (prepare)");
  SVR_CHECK(B > 0 && D > 0 && H > 0 && Wd > 0, SVR_E_BADSHAPE, "conv3d_bwd_data_f16x3: empty volume");
  SVR_CHECK(epilogue == SVR_EPI_NONE || (epilogue == SVR_EPI_MASK && mask), SVR_E_BADARG, "conv3d_bwd_data_f16x3: epilogue %d", epilogue);
  ConvShape sh{B, D, H, Wd, /*K=*/Co, /*NOUT=*/Ci};
  const ConvVariant v = conv_variant(SVR_CONV_BWD_DATA_F16X3S, B, D, H, Wd, Co, Ci);
#define LAUNCH_B3(CKV, TNV)                                                                                                     \
  hipLaunchKernelGGL((conv3d_brick_x3_kernel<CKV, TNV, 2, true>), dim3((unsigned)v.rows, (unsigned)v.ycols), dim3(256), 0, s, dout, \
                     hi, ps, (const float *)nullptr, din, mask, sh, v.nbz, v.nby, v.nbx, epilogue, amax, (double *)nullptr, amax_dout, amax_din)
  if (v.persistent) {
    launch_brick_p<16, true, 2>(dout, hi, ps, nullptr, din, mask, sh, v.nbz, v.nby, v.nbx, v.ycols, epilogue, amax, nullptr, s, amax_dout, amax_din);
  } else if (v.vt == 2) {
    hipLaunchKernelGGL((conv3d_brick_x3_kernel<16, 1, 2, true, 2>), dim3((unsigned)v.rows, (unsigned)v.ycols), dim3(256), 0, s, dout, hi, ps,
                       (const float *)nullptr, din, mask, sh, v.nbz, v.nby, v.nbx, epilogue, amax, (double *)nullptr, amax_dout, amax_din);
  } else if (v.ck == 32) {
    if (v.tn == 1) LAUNCH_B3(32, 1); else if (v.tn == 2) LAUNCH_B3(32, 2); else LAUNCH_B3(32, 4);
  } else {
    if (v.tn == 1) LAUNCH_B3(16, 1); else if (v.tn == 2) LAUNCH_B3(16, 2); else LAUNCH_B3(16, 4);
  }
#undef LAUNCH_B3
  return launch_status("conv3d_bwd_data_f16x3");
}

extern "C" int64_t svr_conv3d_fwd_bf16x6_workspace(int32_t Ci, int32_t Co) { return ws_measure(planes_layout, (int64_t)27 * Ci * Co, 3); }

// out(B,D,H,W,Co) = epi( conv(in(B,D,H,W,Ci), W(Co,Ci,3,3,3)) ) at f32 accuracy; epilogue NONE / BIAS / BIAS_RELU.
extern "C" int svr_conv3d_k3_fwd_bf16x6(const float *in, const float *W, const float *bias, float *out, int32_t B, int32_t D,
                                        int32_t H, int32_t Wd, int32_t Ci, int32_t Co, int epilogue, void *workspace,
                                        void *stream) {
  SVR_CHECK(in && W && out && workspace, SVR_E_BADARG, "conv3d_fwd_bf16x6: null pointer");
  SVR_CHECK(B > 0 && D > 0 && H > 0 && Wd > 0, SVR_E_BADSHAPE, "conv3d_fwd_bf16x6: empty volume");
  SVR_CHECK(Ci % 16 == 0 && Co >= 1, SVR_E_UNSUPPORTED, "conv3d_fwd_bf16x6: need Ci %% 16 == 0 (Ci=%d Co=%d)", Ci, Co);
  SVR_CHECK(epilogue == SVR_EPI_NONE || ((epilogue == SVR_EPI_BIAS || epilogue == SVR_EPI_BIAS_RELU) && bias), SVR_E_BADARG,
            "conv3d_fwd_bf16x6: epilogue %d", epilogue);
  hipStream_t s = (hipStream_t)stream;
  const int64_t ps = (int64_t)27 * Ci * Co;
  WsCursor c(workspace, 16);
  uint16_t *p0 = planes_layout(c, ps, 3);
  hipLaunchKernelGGL((pack_planes_kernel<false, false>), dim3(cdiv(27 * Co * (Ci / 2), 256)), dim3(256), 0, s, W, (const uint32_t *)nullptr, p0, ps, Ci, Co);
  ConvShape sh{B, D, H, Wd, Ci, Co};
  const ConvVariant v = conv_variant(SVR_CONV_FWD_BF16X6, B, D, H, Wd, Ci, Co);
#define LAUNCH_X6(TNV)                                                                                                    \
  hipLaunchKernelGGL((conv3d_brick_x3_kernel<16, TNV, 3>), dim3((unsigned)v.rows, (unsigned)v.ycols), dim3(256), 0, s, in, p0, \
                     ps, bias, out, (const float *)nullptr, sh, v.nbz, v.nby, v.nbx, epilogue)
  if (v.tn == 1) LAUNCH_X6(1); else if (v.tn == 2) LAUNCH_X6(2); else LAUNCH_X6(4);
#undef LAUNCH_X6
  return launch_status("conv3d_fwd_bf16x6");
}

extern "C" int64_t svr_conv3d_fwd_f16x3_workspace(int32_t Ci, int32_t Co) { return ws_measure(scaled_planes_layout, (int64_t)27 * Ci * Co); }

// out(B,D,H,W,Co) = epi( conv(in(B,D,H,W,Ci), W(Co,Ci,3,3,3)) ) with the 3-product f16 split: f32-level accuracy for
// |in| < 65504 (see gemm_f16x3.hip); epilogue NONE / BIAS / BIAS_RELU.
namespace {
int fwd_f16x3(const float *in, const float *W, const float *bias, float *out, int32_t B, int32_t D, int32_t H, int32_t Wd, int32_t Ci,
              int32_t Co, int epilogue, void *workspace, void *stream, double *spart, int *blocks);
}

extern "C" int svr_conv3d_k3_fwd_f16x3(const float *in, const float *W, const float *bias, float *out, int32_t B, int32_t D,
                                       int32_t H, int32_t Wd, int32_t Ci, int32_t Co, int epilogue, void *workspace,
                                       void *stream) {
  return fwd_f16x3(in, W, bias, out, B, D, H, Wd, Ci, Co, epilogue, workspace, stream, nullptr, nullptr);
}

// The same convolution + the BatchNorm statistics of its output as per-workgroup partial sums: part[blocks][2][Co] float64
// (sum, sum of squares), blocks = svr_conv3d_fwd_f16x3_stats_blocks(...); svr_bn_finalize_parts turns them into the
// BatchNorm's scale / shift / running statistics -- no statistics pass over the output.
extern "C" int32_t svr_conv3d_fwd_f16x3_stats_blocks(int32_t B, int32_t D, int32_t H, int32_t Wd, int32_t Ci, int32_t Co) {
  int blocks = 0;
  (void)fwd_f16x3(nullptr, nullptr, nullptr, nullptr, B, D, H, Wd, Ci, Co, SVR_EPI_NONE, nullptr, nullptr, nullptr, &blocks);
  return blocks;
}
extern "C" int svr_conv3d_k3_fwd_f16x3_stats(const float *in, const float *W, const float *bias, float *out, double *part, int32_t B,
                                             int32_t D, int32_t H, int32_t Wd, int32_t Ci, int32_t Co, int epilogue,
                                             void *workspace, void *stream) {
  SVR_CHECK(in && part, SVR_E_BADARG, "conv3d_fwd_f16x3_stats: null pointer");
  return fwd_f16x3(in, W, bias, out, B, D, H, Wd, Ci, Co, epilogue, workspace, stream, part, nullptr);
}

namespace {
int fwd_f16x3(const float *in, const float *W, const float *bias, float *out, int32_t B, int32_t D, int32_t H, int32_t Wd, int32_t Ci,
              int32_t Co, int epilogue, void *workspace, void *stream, double *spart, int *blocks) {
  if (blocks) {   // query: the number of workgroup rows (= partial-sum rows) of the variant this shape takes
    *blocks = (int)conv_variant(SVR_CONV_FWD_F16X3, B, D, H, Wd, Ci, Co).rows;
    return SVR_OK;
  }
  // in == NULL: PREPARE only (W -> scale + split planes in the workspace);  W == NULL: RUN on a workspace prepared earlier
  SVR_CHECK((in || W) && (!in || out) && workspace, SVR_E_BADARG, "conv3d_fwd_f16x3: null pointer");
  SVR_CHECK(Ci % 16 == 0 && Co >= 1, SVR_E_UNSUPPORTED, "conv3d_fwd_f16x3: need Ci %% 16 == 0 (Ci=%d Co=%d)", Ci, Co);
  hipStream_t s = (hipStream_t)stream;
  const int64_t ps = (int64_t)27 * Ci * Co;
  WsCursor c(workspace);
  const auto [amax, p0] = scaled_planes_layout(c, ps);
  if (W) {
    w_amax_launch(W, ps, 1, ps, amax, s, (unsigned)cdiv(ps, 1024));
    hipLaunchKernelGGL((pack_planes_kernel<true, false>), dim3(cdiv(27 * Co * (Ci / 2), 256)), dim3(256), 0, s, W, (const uint32_t *)amax, p0, ps, Ci, Co);
  }
  if (!in) return launch_status("conv3d_fwd_f16x3 (prepare)");
  SVR_CHECK(B > 0 && D > 0 && H > 0 && Wd > 0, SVR_E_BADSHAPE, "conv3d_fwd_f16x3: empty volume");
  SVR_CHECK(epilogue == SVR_EPI_NONE || ((epilogue == SVR_EPI_BIAS || epilogue == SVR_EPI_BIAS_RELU) && bias), SVR_E_BADARG,
            "conv3d_fwd_f16x3: epilogue %d", epilogue);
  ConvShape sh{B, D, H, Wd, Ci, Co};
  const ConvVariant v = conv_variant(SVR_CONV_FWD_F16X3, B, D, H, Wd, Ci, Co);
#define LAUNCH_H3(CKV, TNV)                                                                                                 \
  hipLaunchKernelGGL((conv3d_brick_x3_kernel<CKV, TNV, 2, true>), dim3((unsigned)v.rows, (unsigned)v.ycols), dim3(256), 0, s, \
                     in, p0, ps, bias, out, (const float *)nullptr, sh, v.nbz, v.nby, v.nbx, epilogue, amax, spart)
  if (v.persistent) {
    launch_brick_p<16, true, 2>(in, p0, ps, bias, out, nullptr, sh, v.nbz, v.nby, v.nbx, v.ycols, epilogue, amax, spart, s);
  } else if (v.vt == 2) {
    hipLaunchKernelGGL((conv3d_brick_x3_kernel<16, 1, 2, true, 2>), dim3((unsigned)v.rows, (unsigned)v.ycols), dim3(256), 0, s, in, p0, ps,
                       bias, out, (const float *)nullptr, sh, v.nbz, v.nby, v.nbx, epilogue, amax, spart);
  } else if (v.ck == 32) {
    if (v.tn == 1) LAUNCH_H3(32, 1); else if (v.tn == 2) LAUNCH_H3(32, 2); else LAUNCH_H3(32, 4);
  } else {
    if (v.tn == 1) LAUNCH_H3(16, 1); else if (v.tn == 2) LAUNCH_H3(16, 2); else LAUNCH_H3(16, 4);
  }
#undef LAUNCH_H3
  return launch_status("conv3d_fwd_f16x3");
}
}  // namespace

// Which kernel instantiation a shape takes (host only, no device memory: callable without a GPU).  The launchers above ask
// the same conv_variant(), so this cannot drift from what runs.
extern "C" int svr_conv3d_k3_variant(int32_t op, int32_t B, int32_t D, int32_t H, int32_t Wd, int32_t Ci, int32_t Co, int32_t *ck,
                                     int32_t *tn, int32_t *vt, int32_t *persistent, int64_t *workgroup_rows) {
  SVR_CHECK(op >= SVR_CONV_FWD_F16X3 && op <= SVR_CONV_FWD_BF16X6, SVR_E_BADARG, "conv3d_k3_variant: op %d", op);
  SVR_CHECK(B > 0 && D > 0 && H > 0 && Wd > 0, SVR_E_BADSHAPE, "conv3d_k3_variant: empty volume");
  const bool fwd = op == SVR_CONV_FWD_F16X3 || op == SVR_CONV_FWD_BF16X6;
  if (fwd)
    SVR_CHECK(Ci % 16 == 0 && Ci >= 16 && Co >= 1, SVR_E_UNSUPPORTED, "conv3d_k3_variant: forward needs Ci %% 16 == 0 (Ci=%d Co=%d)", Ci, Co);
  else
    SVR_CHECK(Co % 16 == 0 && Co >= 16 && Ci % 2 == 0 && Ci >= 2, SVR_E_UNSUPPORTED,
              "conv3d_k3_variant: backward-data needs Co %% 16 == 0, Ci even (Ci=%d Co=%d)", Ci, Co);
  const ConvVariant v = fwd ? conv_variant(op, B, D, H, Wd, Ci, Co) : conv_variant(op, B, D, H, Wd, Co, Ci);
  if (ck) *ck = v.ck;
  if (tn) *tn = v.tn;
  if (vt) *vt = v.vt;
  if (persistent) *persistent = v.persistent ? 1 : 0;
  if (workgroup_rows) *workgroup_rows = v.rows;
  return SVR_OK;
}
