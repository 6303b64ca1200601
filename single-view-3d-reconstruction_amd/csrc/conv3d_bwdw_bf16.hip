// 3x3x3 convolution weight gradient on the bf16 matrix cores with the 3-term split ("bf16x3"), gfx950.
//
//   dW[tap][ci][co] = sum_voxel in[voxel + tap][ci] * dout[voxel][co]
//
// The reduction runs over VOXELS, so both MFMA operands need 8 consecutive voxels of one channel per lane:
// the brick's input halo tile (6x6x10 voxels) and its dout tile (4x4x8) are transposed on the way into LDS,
//   in plane  [ci][halo row (hz,hy)][12 bf16: the 10 voxels of the x-row + pad]      (hi and mid planes)
//   dout plane[co][row (vz,vy)][8 bf16]
// One 24-byte halo row read serves the three dx taps of a (dz,dy) pair: dx = -1 / +1 are dword-aligned
// sub-rows, dx = 0 is a 16-bit funnel shift (v_alignbit).  k of v_mfma_f32_32x32x16_bf16 = 2 x-rows of 8 voxels.
//   x = hi + mid, products mid*hi + hi*mid + hi*hi, f32 accumulation (~1.5e-5 relative per product; the weight
//   gradient sums 10^4..10^6 such products of mixed sign, see gemm_bf16x3.hip for the error argument).
//
// Workgroup = 8 waves, persistent over bricks: wave (g, h) owns the taps 7g .. 7g+6 (g = 3: six taps) for half of the
// brick's voxels (h), its 7 accumulator tiles (32 ci x 32 co) stay in registers over all bricks; the two halves and the
// workgroups land in partial slabs that conv3d.hip's ordered f64 reduce sums (deterministic).  (Until round 3: 6 waves
// = 3 dz x 2 halves with 9 tiles each -- two of the four SIMDs carried two waves, the other two one, and the barrier
// per brick waited for the loaded pair: 6 912 MFMA cycles per brick on the critical SIMD instead of 5 376 now.)
// LDS is double buffered: the next brick's global loads are issued before the MFMA phase and written to the other
// buffer after it, one barrier per brick.  73 KB per buffer -> one workgroup per CU.
#include "common.h"
#include "f16x3.h"

using namespace svr;

namespace {

struct ConvShape {
  int B, D, H, W, Ci, Co;
};

constexpr int BRZ = 4, BRY = 4, BRX = 8;
constexpr int HLY = BRY + 2;
constexpr int HROWS = (BRZ + 2) * (BRY + 2);      // 36 halo x-rows
constexpr int ROWDW = 6;                          // dwords per halo x-row: 10 voxels + 2 pad (bf16)
constexpr int CIS = HROWS * ROWDW + 2;            // 218 dwords per input channel (26 mod 64: b64 reads conflict free)
constexpr int COS = BRZ * BRY * 4 + 4;            // 68 dwords per output channel (b128 reads conflict free)
constexpr int IN_PLANE = 32 * CIS, DO_PLANE = 32 * COS;
constexpr int BUF = 2 * IN_PLANE + 2 * DO_PLANE;  // dwords per stage: 18 304 (73 216 B)
constexpr int NT = 512;
constexpr int IN_ITEMS = HROWS * 5 * 8;           // (halo row, voxel pair, 4-channel group) = 1440
constexpr int DO_ITEMS = BRZ * BRY * 4 * 8;       // (row, voxel pair, 4-channel group)      = 512: one per thread
constexpr int IN_IT = (IN_ITEMS + NT - 1) / NT;   // 3: two travel in the first half of a brick's prefetch, one + the dout item in the second
static_assert(IN_IT == 3 && DO_ITEMS == NT, "prefetch phases below are written for 3 + 1 items per thread");
constexpr int TAPS_PER_WAVE = 7;                  // 27 taps over 4 tap groups: 7 / 7 / 7 / 6

__device__ __forceinline__ bf16x8 frag(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  union { uint4 q; bf16x8 v; } f;
  f.q = make_uint4(a, b, c, d);
  return f.v;
}

// F16 ("f16x3s", svr_conv3d_k3_bwd_weight_f16x3): the scaled f16 split -- dout * 2^s (its |max| brought to [2^13, 2^14)), both
// operands as hi = rn16(v), lo' = rn16((v - hi) 2^11), products lo'(in) (hi(dout) 2^-11) + (hi(in) 2^-11) lo'(dout) + hi hi with
// the 2^-11 applied to the hi fragments in registers, slabs * 2^-s: 22 mantissa bits per operand, the same three instructions.
// MFMA phase of one x-row pair (kq) for tap group G: rows R = (dz, dy) pairs touched by the taps 7G .. 7G+6
template <int G, bool F16>
__device__ __forceinline__ void wgrad_rows(const uint32_t *__restrict__ ibuf, const uint32_t *__restrict__ dbuf, int l31, int r,
                                           f32x16 (&acc)[TAPS_PER_WAVE]) {
  constexpr int T0 = G * TAPS_PER_WAVE, T1 = (T0 + TAPS_PER_WAVE < 27) ? T0 + TAPS_PER_WAVE : 27;
  const int vz = r >> 2, vy = r & 3;
  const uint4 bh = *reinterpret_cast<const uint4 *>(dbuf + l31 * COS + r * 4);
  const uint4 bm = *reinterpret_cast<const uint4 *>(dbuf + DO_PLANE + l31 * COS + r * 4);
  const bf16x8 b_hi = frag(bh.x, bh.y, bh.z, bh.w), b_mid = frag(bm.x, bm.y, bm.z, bm.w);
#pragma unroll
  for (int R = T0 / 3; R <= (T1 - 1) / 3; ++R) {
    const int dzi = R / 3, dyi = R % 3;
    const uint32_t *ph = ibuf + l31 * CIS + ((vz + dzi) * HLY + vy + dyi) * ROWDW;
    const uint2 m01 = *reinterpret_cast<const uint2 *>(ph + IN_PLANE), m23 = *reinterpret_cast<const uint2 *>(ph + IN_PLANE + 2);
    const uint32_t m4 = ph[IN_PLANE + 4];
    const uint2 h01 = *reinterpret_cast<const uint2 *>(ph), h23 = *reinterpret_cast<const uint2 *>(ph + 2);
    const uint32_t h4 = ph[4];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int tap = R * 3 + dx;
      if (tap < T0 || tap >= T1) continue;
      const int i = tap - T0;
      // one 24-byte halo row serves the three dx taps: dx = 0 / 2 are dword-aligned sub-rows, dx = 1 a 16-bit funnel shift
      const bf16x8 am = dx == 0 ? frag(m01.x, m01.y, m23.x, m23.y)
                      : dx == 2 ? frag(m01.y, m23.x, m23.y, m4)
                                : frag(__builtin_amdgcn_alignbit(m01.y, m01.x, 16), __builtin_amdgcn_alignbit(m23.x, m01.y, 16),
                                       __builtin_amdgcn_alignbit(m23.y, m23.x, 16), __builtin_amdgcn_alignbit(m4, m23.y, 16));
      const bf16x8 ah = dx == 0 ? frag(h01.x, h01.y, h23.x, h23.y)
                      : dx == 2 ? frag(h01.y, h23.x, h23.y, h4)
                                : frag(__builtin_amdgcn_alignbit(h01.y, h01.x, 16), __builtin_amdgcn_alignbit(h23.x, h01.y, 16),
                                       __builtin_amdgcn_alignbit(h23.y, h23.x, 16), __builtin_amdgcn_alignbit(h4, h23.y, 16));
      // mid plane of the input x hi plane of dout first (small terms first)
      if constexpr (F16) {
        const f16x8 fam = __builtin_bit_cast(f16x8, am), fah = __builtin_bit_cast(f16x8, ah);
        const f16x8 fbh = __builtin_bit_cast(f16x8, b_hi), fbm = __builtin_bit_cast(f16x8, b_mid);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fam, scale_2m11(fbh), acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(scale_2m11(fah), fbm, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fah, fbh, acc[i], 0, 0, 0);
      } else {
      acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, b_hi, acc[i], 0, 0, 0);
      acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, b_mid, acc[i], 0, 0, 0);
      acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, b_hi, acc[i], 0, 0, 0);
      }
    }
  }
}

template <bool F16>
__global__ __launch_bounds__(NT) void conv3d_bwd_weight_x3_kernel(const float *__restrict__ in,
                                                                  const float *__restrict__ dout,
                                                                  float *__restrict__ slab, ConvShape s, int nbz, int nby,
                                                                  int nbx, int co_tiles, float *__restrict__ dbpart,
                                                                  const uint32_t *__restrict__ amax_dout) {
  __shared__ uint32_t lds[2 * BUF];
  float sy = 1.f;
  if constexpr (F16) sy = amax_dout ? w_scale(amax_dout[0], false) : 1.f;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int grp = wave & 3, half = wave >> 2;
  const int pair = blockIdx.y;
  const int ci0 = (pair / co_tiles) * 32, co0 = (pair % co_tiles) * 32;
  const int bricks = s.B * nbz * nby * nbx;   // (host: < 2^31)

  // the next brick travels in two phases: phase 0 = input items 0, 1 of this thread, phase 1 = input item 2 + its dout item
  float4 ia[2][2], da[2];
  int iok[2], dok = 0;  // bit v: voxel v of the pair is inside the volume
  // bias gradient: dout passes through this thread's registers exactly once per brick; its 4 channels (cg = t & 7,
  // NT % 8 == 0) are summed here by the workgroups of the first ci tile -> no separate pass over dout
  const bool want_db = dbpart != nullptr && ci0 == 0;
  float4 dbs = make_float4(0.f, 0.f, 0.f, 0.f);

  // (32-bit brick arithmetic: the 64-bit divisions of the first version were ~1 000 scalar instructions per brick and wave,
  // eight waves of them per CU against ~10 000 cycles per brick)
  auto load = [&](int brick, int ph) {
    int q = brick;
    const int bx = q % nbx; q /= nbx;
    const int by = q % nby; q /= nby;
    const int bz = q % nbz;
    const int b = q / nbz;
    const int z0 = bz * BRZ, y0 = by * BRY, x0 = bx * BRX;
    const float *inb = in + (int64_t)b * s.D * s.H * s.W * s.Ci;
#pragma unroll
    for (int j = 0; j < (ph == 0 ? 2 : 1); ++j) {
      const int idx = min(t + NT * (ph * 2 + j), IN_ITEMS - 1);
      const int hrow = idx / 40, rem = idx % 40, pr = rem >> 3, cg = rem & 7;
      const int gz = z0 + hrow / HLY - 1, gy = y0 + hrow % HLY - 1, gx = x0 + 2 * pr - 1;
      // unconditional loads from clamped coordinates (a load inside a branch makes the compiler wait for it at the
      // end of the branch, which serialises the whole prefetch); out-of-range voxels are zeroed in store()
      const bool rowok = gz >= 0 && gz < s.D && gy >= 0 && gy < s.H && ci0 + cg * 4 < s.Ci;
      const int cz = min(max(gz, 0), s.D - 1), cy = min(max(gy, 0), s.H - 1), cc = min(ci0 + cg * 4, s.Ci - 4);
      // (uniform base + 32-bit byte offsets, 24-bit multiplies: the host checks the ranges)
      const uint32_t ro = __umul24(__umul24(__umul24((uint32_t)cz, (uint32_t)s.H) + (uint32_t)cy, (uint32_t)s.W), (uint32_t)s.Ci) + (uint32_t)cc;
      const char *p = reinterpret_cast<const char *>(inb);
      ia[j][0] = *reinterpret_cast<const float4 *>(p + (ro + __umul24((uint32_t)min(max(gx, 0), s.W - 1), (uint32_t)s.Ci)) * 4u);
      ia[j][1] = *reinterpret_cast<const float4 *>(p + (ro + __umul24((uint32_t)min(max(gx + 1, 0), s.W - 1), (uint32_t)s.Ci)) * 4u);
      iok[j] = (rowok && gx >= 0 && gx < s.W ? 1 : 0) | (rowok && gx + 1 >= 0 && gx + 1 < s.W ? 2 : 0);
    }
    if (ph == 1) {
      const float *dob = dout + (int64_t)b * s.D * s.H * s.W * s.Co;
      const int row = t >> 5, pr = (t & 31) >> 3, cg = t & 7;
      const int gz = z0 + (row >> 2), gy = y0 + (row & 3), gx = x0 + 2 * pr;
      const bool rowok = gz < s.D && gy < s.H && co0 + cg * 4 < s.Co;
      const int cz = min(gz, s.D - 1), cy = min(gy, s.H - 1), cc = min(co0 + cg * 4, s.Co - 4);
      const uint32_t ro = __umul24(__umul24(__umul24((uint32_t)cz, (uint32_t)s.H) + (uint32_t)cy, (uint32_t)s.W), (uint32_t)s.Co) + (uint32_t)cc;
      const char *p = reinterpret_cast<const char *>(dob);
      da[0] = *reinterpret_cast<const float4 *>(p + (ro + __umul24((uint32_t)min(gx, s.W - 1), (uint32_t)s.Co)) * 4u);
      da[1] = *reinterpret_cast<const float4 *>(p + (ro + __umul24((uint32_t)min(gx + 1, s.W - 1), (uint32_t)s.Co)) * 4u);
      dok = (rowok && gx < s.W ? 1 : 0) | (rowok && gx + 1 < s.W ? 2 : 0);
    }
  };

  auto store = [&](uint32_t *buf, int ph) {
#pragma unroll
    for (int j = 0; j < (ph == 0 ? 2 : 1); ++j) {
      const int idx = t + NT * (ph * 2 + j);
      if (idx < IN_ITEMS) {
        const int hrow = idx / 40, rem = idx % 40, pr = rem >> 3, cg = rem & 7;
        uint32_t *d = buf + (cg * 4) * CIS + hrow * ROWDW + pr;
        const float v0[4] = {ia[j][0].x, ia[j][0].y, ia[j][0].z, ia[j][0].w};
        const float v1[4] = {ia[j][1].x, ia[j][1].y, ia[j][1].z, ia[j][1].w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          uint32_t h, m;
          if constexpr (F16) split_x((iok[j] & 1) ? v0[c] : 0.f, (iok[j] & 2) ? v1[c] : 0.f, h, m);
          else split2((iok[j] & 1) ? v0[c] : 0.f, (iok[j] & 2) ? v1[c] : 0.f, h, m);
          d[c * CIS] = h;
          d[IN_PLANE + c * CIS] = m;
        }
      }
    }
    if (ph == 1) {
      uint32_t *dbuf = buf + 2 * IN_PLANE;
      const int row = t >> 5, pr = (t & 31) >> 3, cg = t & 7;
      uint32_t *d = dbuf + (cg * 4) * COS + row * 4 + pr;
      float v0[4] = {da[0].x, da[0].y, da[0].z, da[0].w};
      float v1[4] = {da[1].x, da[1].y, da[1].z, da[1].w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        v0[c] = (dok & 1) ? v0[c] : 0.f;
        v1[c] = (dok & 2) ? v1[c] : 0.f;
        uint32_t h, m;
        if constexpr (F16) split_x(v0[c] * sy, v1[c] * sy, h, m);
        else split2(v0[c], v1[c], h, m);
        d[c * COS] = h;
        d[DO_PLANE + c * COS] = m;
      }
      if (want_db) {
        dbs.x += v0[0] + v1[0]; dbs.y += v0[1] + v1[1]; dbs.z += v0[2] + v1[2]; dbs.w += v0[3] + v1[3];
      }
    }
  };

  f32x16 acc[TAPS_PER_WAVE];
#pragma unroll
  for (int i = 0; i < TAPS_PER_WAVE; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  int brick = (int)blockIdx.x;
  if (brick < bricks) {
    load(brick, 0);
    store(lds, 0);
    load(brick, 1);
    store(lds, 1);
  }
  __syncthreads();
  int cur = 0;
  for (; brick < bricks; brick += (int)gridDim.x) {
    const int next = brick + (int)gridDim.x;
    const bool more = next < bricks;
    if (more) load(next, 0);
    const uint32_t *ibuf = lds + cur * BUF, *dbuf = ibuf + 2 * IN_PLANE;
#pragma unroll 1
    for (int kq = 0; kq < 4; ++kq) {
      const int r = 2 * (half * 4 + kq) + lh;  // x-row of the brick handled by this half-wave: r = vz*4 + vy
      switch (grp) {  // wave-uniform
        case 0: wgrad_rows<0, F16>(ibuf, dbuf, l31, r, acc); break;
        case 1: wgrad_rows<1, F16>(ibuf, dbuf, l31, r, acc); break;
        case 2: wgrad_rows<2, F16>(ibuf, dbuf, l31, r, acc); break;
        default: wgrad_rows<3, F16>(ibuf, dbuf, l31, r, acc); break;
      }
      if (kq == 1 && more) {  // first part of the next brick has arrived: park it in the other buffer, fetch the rest
        store(lds + (cur ^ 1) * BUF, 0);
        load(next, 1);
      }
    }
    if (more) store(lds + (cur ^ 1) * BUF, 1);
    __syncthreads();
    cur ^= 1;
  }

  if (want_db) {  // fixed-order sum of the 64 threads per channel group through LDS (free after the last barrier)
    float *sred = reinterpret_cast<float *>(lds);
    sred[t * 4 + 0] = dbs.x; sred[t * 4 + 1] = dbs.y; sred[t * 4 + 2] = dbs.z; sred[t * 4 + 3] = dbs.w;
    __syncthreads();
    if (t < 32) {
      const int cg = t >> 2, c = t & 3;
      float sum = 0.f;
      for (int i = 0; i < NT / 8; ++i) sum += sred[(i * 8 + cg) * 4 + c];
      if (co0 + t < s.Co) dbpart[(int64_t)blockIdx.x * s.Co + co0 + t] = sum;
    }
  }
  // slab layout shared with conv3d.hip's reduce kernel: [part][tap][pair][32 ci][32 co]
  float inv = 1.f;
  if constexpr (F16) inv = amax_dout ? w_scale(amax_dout[0], true) : 1.f;
  const int pairs = gridDim.y;
  const int64_t part = (int64_t)blockIdx.x * 2 + half;
#pragma unroll
  for (int i = 0; i < TAPS_PER_WAVE; ++i) {
    const int tap = grp * TAPS_PER_WAVE + i;
    if (tap < 27) {
      float *o = slab + ((part * 27 + tap) * pairs + pair) * 1024;
#pragma unroll
      for (int r = 0; r < 16; ++r) o[((r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + l31] = F16 ? acc[i][r] * inv : acc[i][r];
    }
  }
}

// ---- wave-specialised version of the kernel above (round 5).  The kernel above runs every role in all 8 waves in lockstep, so
// the split / transposing LDS writes / load waits of one wave never run under the MFMAs of the other wave on its SIMD (its
// measurement builds: the MFMA phase overlaps nothing).  Here waves 0-3 (one per SIMD) are CONSUMERS: LDS fragment reads and
// MFMAs only, all x-rows of the brick for their tap group; waves 4-7 are PRODUCERS: global loads of brick b+2, split and
// transposed writes of brick b+1 into the stage the consumers are not reading.  Same LDS stages, one barrier per brick; the
// MFMA holds its SIMD's vector issue for 8 of its 32 cycles, the producer's VALU / LDS writes take the other 24.  The two
// roles run separate loops (same barrier count), so the accumulators and the prefetch registers are never live together.
// PAIR (Ci <= 16): rows 16-31 of the A tile hold the same channels one halo row (dz, dy) further on, with the same dx: the 9
// rows x 3 dx taps become 5 row pairs x 3 = 15 tile-taps instead of 27 half-empty ones (only a per-lane row offset changes).
// One slab part per workgroup (the consumer covers both brick halves).
constexpr int WS_NP = NT / 2;   // producer threads

// LDS operands of one x-row pair (r = 2 kq + lh) for tap group G: the dout row and the halo rows (row pairs for PAIR) of its taps
template <int G, bool PAIR>
struct WsFrag {
  static constexpr int NTT = PAIR ? 15 : 27, TPW = PAIR ? 4 : TAPS_PER_WAVE;
  static constexpr int T0 = G * TPW, T1 = (T0 + TPW < NTT) ? T0 + TPW : NTT;
  static constexpr int RA = T0 / 3, NR = (T1 - 1) / 3 - RA + 1;
  uint4 bh, bm;
  uint2 m01[NR], m23[NR], h01[NR], h23[NR];
  uint32_t m4[NR], h4[NR];
};

template <int G, bool PAIR>
__device__ __forceinline__ void ws_fetch(const uint32_t *__restrict__ ibuf, const uint32_t *__restrict__ dbuf, int l31, int r,
                                         WsFrag<G, PAIR> &f) {
  using F = WsFrag<G, PAIR>;
  const int vz = r >> 2, vy = r & 3;
  f.bh = *reinterpret_cast<const uint4 *>(dbuf + l31 * COS + r * 4);
  f.bm = *reinterpret_cast<const uint4 *>(dbuf + DO_PLANE + l31 * COS + r * 4);
  const uint32_t *pl = ibuf + (PAIR ? (l31 & 15) : l31) * CIS + (vz * HLY + vy) * ROWDW;
#pragma unroll
  for (int k = 0; k < F::NR; ++k) {
    const int R = F::RA + k;
    // halo row (dz, dy) of this lane: R itself, or for PAIR row 2R (lanes 0-15) / 2R + 1 (lanes 16-31; row 9 does not exist:
    // row 8 again, its products are discarded at the slab write)
    const int ra = PAIR ? 2 * R : R, rb = PAIR ? (2 * R + 1 < 9 ? 2 * R + 1 : 8) : R;
    const int oa = ((ra / 3) * HLY + ra % 3) * ROWDW, ob = ((rb / 3) * HLY + rb % 3) * ROWDW;
    const uint32_t *ph = pl + (PAIR && l31 >= 16 ? ob : oa);
    f.m01[k] = *reinterpret_cast<const uint2 *>(ph + IN_PLANE);
    f.m23[k] = *reinterpret_cast<const uint2 *>(ph + IN_PLANE + 2);
    f.m4[k] = ph[IN_PLANE + 4];
    f.h01[k] = *reinterpret_cast<const uint2 *>(ph);
    f.h23[k] = *reinterpret_cast<const uint2 *>(ph + 2);
    f.h4[k] = ph[4];
  }
}

// the MFMAs of one x-row pair: per tap the three split products in the order of the kernel above
template <int G, bool F16, bool PAIR>
__device__ __forceinline__ void ws_mfma(const WsFrag<G, PAIR> &f, f32x16 (&acc)[TAPS_PER_WAVE]) {
  using F = WsFrag<G, PAIR>;
  const bf16x8 b_hi = frag(f.bh.x, f.bh.y, f.bh.z, f.bh.w), b_mid = frag(f.bm.x, f.bm.y, f.bm.z, f.bm.w);
#pragma unroll
  for (int k = 0; k < F::NR; ++k) {
    const int R = F::RA + k;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int tt = R * 3 + dx;
      if (tt < F::T0 || tt >= F::T1) continue;
      const int i = tt - F::T0;
      const uint2 m01 = f.m01[k], m23 = f.m23[k], h01 = f.h01[k], h23 = f.h23[k];
      const uint32_t m4 = f.m4[k], h4 = f.h4[k];
      const bf16x8 am = dx == 0 ? frag(m01.x, m01.y, m23.x, m23.y)
                      : dx == 2 ? frag(m01.y, m23.x, m23.y, m4)
                                : frag(__builtin_amdgcn_alignbit(m01.y, m01.x, 16), __builtin_amdgcn_alignbit(m23.x, m01.y, 16),
                                       __builtin_amdgcn_alignbit(m23.y, m23.x, 16), __builtin_amdgcn_alignbit(m4, m23.y, 16));
      const bf16x8 ah = dx == 0 ? frag(h01.x, h01.y, h23.x, h23.y)
                      : dx == 2 ? frag(h01.y, h23.x, h23.y, h4)
                                : frag(__builtin_amdgcn_alignbit(h01.y, h01.x, 16), __builtin_amdgcn_alignbit(h23.x, h01.y, 16),
                                       __builtin_amdgcn_alignbit(h23.y, h23.x, 16), __builtin_amdgcn_alignbit(h4, h23.y, 16));
      if constexpr (F16) {
        const f16x8 fam = __builtin_bit_cast(f16x8, am), fah = __builtin_bit_cast(f16x8, ah);
        const f16x8 fbh = __builtin_bit_cast(f16x8, b_hi), fbm = __builtin_bit_cast(f16x8, b_mid);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fam, scale_2m11(fbh), acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(scale_2m11(fah), fbm, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fah, fbh, acc[i], 0, 0, 0);
      } else {
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, b_hi, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, b_mid, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, b_hi, acc[i], 0, 0, 0);
      }
    }
  }
}

// consumer wave of tap group G: all 16 x-rows of each brick, accumulators over all bricks, then its slab tiles
template <int G, bool F16, bool PAIR>
__device__ __forceinline__ void ws_consume(const uint32_t *lds, int n_it, float *__restrict__ slab, int pair,
                                           const uint32_t *__restrict__ amax_dout) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, lh = lane >> 5;
  f32x16 acc[TAPS_PER_WAVE];
#pragma unroll
  for (int i = 0; i < TAPS_PER_WAVE; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  __syncthreads();   // stage 0 filled
  int cur = 0;
  for (int it = 0; it < n_it; ++it) {
    const uint32_t *ibuf = lds + cur * BUF, *dbuf = ibuf + 2 * IN_PLANE;
    // (software-pipelining the LDS reads of pair kq + 1 under the MFMAs of pair kq measured the same: not kept)
#pragma unroll 1
    for (int kq = 0; kq < 8; ++kq) {   // x-row r = 2 kq + lh = vz*4 + vy
      WsFrag<G, PAIR> f;
      ws_fetch<G, PAIR>(ibuf, dbuf, l31, 2 * kq + lh, f);
      ws_mfma<G, F16, PAIR>(f, acc);
    }
    __syncthreads();
    cur ^= 1;
  }
  // slab layout shared with conv3d.hip's reduce kernel: [part][tap][pair][32 ci][32 co], one part per workgroup
  float inv = 1.f;
  if constexpr (F16) inv = amax_dout ? w_scale(amax_dout[0], true) : 1.f;
  const int pairs = gridDim.y;
  const int64_t part = blockIdx.x;
  constexpr int NTT = PAIR ? 15 : 27, TPW = PAIR ? 4 : TAPS_PER_WAVE;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int tt = G * TPW + i;
    if (tt >= NTT) continue;
    if constexpr (PAIR) {  // accumulator rows 0-15: halo row 2R, channels 0-15; rows 16-31: halo row 2R + 1
      const int R = tt / 3, dx = tt % 3;
      float *lo = slab + ((part * 27 + (2 * R) * 3 + dx) * pairs + pair) * 1024;
      float *hi = slab + ((part * 27 + (2 * R + 1) * 3 + dx) * pairs + pair) * 1024;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float v = F16 ? acc[i][r] * inv : acc[i][r];
        if (r < 8) lo[row * 32 + l31] = v;
        else if (2 * R + 1 < 9) hi[(row - 16) * 32 + l31] = v;
      }
    } else {
      float *o = slab + ((part * 27 + tt) * pairs + pair) * 1024;
#pragma unroll
      for (int r = 0; r < 16; ++r) o[((r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + l31] = F16 ? acc[i][r] * inv : acc[i][r];
    }
  }
}

template <bool F16, bool PAIR>
__global__ __launch_bounds__(NT) void conv3d_bwd_weight_ws_kernel(const float *__restrict__ in, const float *__restrict__ dout,
                                                                  float *__restrict__ slab, ConvShape s, int nbz, int nby,
                                                                  int nbx, int co_tiles, float *__restrict__ dbpart,
                                                                  const uint32_t *__restrict__ amax_dout) {
  constexpr int CG = PAIR ? 4 : 8;                                 // 4-channel groups of the input tile that are loaded
  constexpr int IN_N = HROWS * 5 * CG;                             // (halo row, voxel pair, channel group) items
  constexpr int IN_PT = (IN_N + WS_NP - 1) / WS_NP;                // 6 (3 for PAIR) input items per producer thread
  constexpr int DO_PT = DO_ITEMS / WS_NP;                          // 2 dout items
  static_assert(DO_ITEMS % WS_NP == 0 && WS_NP % 8 == 0, "a producer thread's dout items share one channel group");
  __shared__ uint32_t lds[2 * BUF];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int pair = blockIdx.y;
  const int ci0 = (pair / co_tiles) * 32, co0 = (pair % co_tiles) * 32;
  const int bricks = s.B * nbz * nby * nbx;   // (host: < 2^31)
  const int n_it = (bricks - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;   // host: gridDim.x <= bricks
  const bool want_db = dbpart != nullptr && ci0 == 0;
  float4 dbs = make_float4(0.f, 0.f, 0.f, 0.f);

  if (wave < 4) {
    // ---------------- consumer: tap group `wave` (one whole loop per group: a switch inside the loop made the compiler copy
    // the 112 accumulator registers around it every x-row pair, and spill)
    switch (wave) {
      case 0: ws_consume<0, F16, PAIR>(lds, n_it, slab, pair, amax_dout); break;
      case 1: ws_consume<1, F16, PAIR>(lds, n_it, slab, pair, amax_dout); break;
      case 2: ws_consume<2, F16, PAIR>(lds, n_it, slab, pair, amax_dout); break;
      default: ws_consume<3, F16, PAIR>(lds, n_it, slab, pair, amax_dout); break;
    }
  } else {
    // ---------------- producer: thread p moves input items p + 256 j and dout items p + 256 j of every brick
    const int p = t - WS_NP;
    float sy = 1.f;
    if constexpr (F16) sy = amax_dout ? w_scale(amax_dout[0], false) : 1.f;
    float4 ia[IN_PT][2], da[DO_PT][2];
    int iok[IN_PT], dok[DO_PT];  // bit v: voxel v of the pair is inside the volume

    auto load = [&](int brick) {
      int q = brick;
      const int bx = q % nbx; q /= nbx;
      const int by = q % nby; q /= nby;
      const int bz = q % nbz;
      const int b = q / nbz;
      const int z0 = bz * BRZ, y0 = by * BRY, x0 = bx * BRX;
      const char *inb = reinterpret_cast<const char *>(in + (int64_t)b * s.D * s.H * s.W * s.Ci);
#pragma unroll
      for (int j = 0; j < IN_PT; ++j) {
        const int idx = min(p + WS_NP * j, IN_N - 1);
        const int hrow = idx / (5 * CG), rem = idx % (5 * CG), pr = rem / CG, cg = rem % CG;
        const int gz = z0 + hrow / HLY - 1, gy = y0 + hrow % HLY - 1, gx = x0 + 2 * pr - 1;
        // unconditional loads from clamped coordinates, out-of-range voxels zeroed in store() (see the kernel above)
        const bool rowok = gz >= 0 && gz < s.D && gy >= 0 && gy < s.H && ci0 + cg * 4 < s.Ci;
        const int cz = min(max(gz, 0), s.D - 1), cy = min(max(gy, 0), s.H - 1), cc = min(ci0 + cg * 4, s.Ci - 4);
        const uint32_t ro = __umul24(__umul24(__umul24((uint32_t)cz, (uint32_t)s.H) + (uint32_t)cy, (uint32_t)s.W), (uint32_t)s.Ci) + (uint32_t)cc;
        ia[j][0] = *reinterpret_cast<const float4 *>(inb + (ro + __umul24((uint32_t)min(max(gx, 0), s.W - 1), (uint32_t)s.Ci)) * 4u);
        ia[j][1] = *reinterpret_cast<const float4 *>(inb + (ro + __umul24((uint32_t)min(max(gx + 1, 0), s.W - 1), (uint32_t)s.Ci)) * 4u);
        iok[j] = (rowok && gx >= 0 && gx < s.W ? 1 : 0) | (rowok && gx + 1 >= 0 && gx + 1 < s.W ? 2 : 0);
      }
      const char *dob = reinterpret_cast<const char *>(dout + (int64_t)b * s.D * s.H * s.W * s.Co);
#pragma unroll
      for (int j = 0; j < DO_PT; ++j) {
        const int idx = p + WS_NP * j;
        const int row = idx >> 5, pr = (idx & 31) >> 3, cg = idx & 7;
        const int gz = z0 + (row >> 2), gy = y0 + (row & 3), gx = x0 + 2 * pr;
        const bool rowok = gz < s.D && gy < s.H && co0 + cg * 4 < s.Co;
        const int cz = min(gz, s.D - 1), cy = min(gy, s.H - 1), cc = min(co0 + cg * 4, s.Co - 4);
        const uint32_t ro = __umul24(__umul24(__umul24((uint32_t)cz, (uint32_t)s.H) + (uint32_t)cy, (uint32_t)s.W), (uint32_t)s.Co) + (uint32_t)cc;
        da[j][0] = *reinterpret_cast<const float4 *>(dob + (ro + __umul24((uint32_t)min(gx, s.W - 1), (uint32_t)s.Co)) * 4u);
        da[j][1] = *reinterpret_cast<const float4 *>(dob + (ro + __umul24((uint32_t)min(gx + 1, s.W - 1), (uint32_t)s.Co)) * 4u);
        dok[j] = (rowok && gx < s.W ? 1 : 0) | (rowok && gx + 1 < s.W ? 2 : 0);
      }
    };

    auto store = [&](uint32_t *buf) {
#pragma unroll
      for (int j = 0; j < IN_PT; ++j) {
        const int idx = p + WS_NP * j;
        if (IN_N % WS_NP == 0 || idx < IN_N) {
          const int hrow = idx / (5 * CG), rem = idx % (5 * CG), pr = rem / CG, cg = rem % CG;
          uint32_t *d = buf + (cg * 4) * CIS + hrow * ROWDW + pr;
          const float4 a0 = ia[j][0], a1 = ia[j][1];
          const int ok = iok[j];
          const float v0[4] = {a0.x, a0.y, a0.z, a0.w};
          const float v1[4] = {a1.x, a1.y, a1.z, a1.w};
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            uint32_t h, m;
            if constexpr (F16) split_x((ok & 1) ? v0[c] : 0.f, (ok & 2) ? v1[c] : 0.f, h, m);
            else split2((ok & 1) ? v0[c] : 0.f, (ok & 2) ? v1[c] : 0.f, h, m);
            d[c * CIS] = h;
            d[IN_PLANE + c * CIS] = m;
          }
        }
      }
      uint32_t *dbuf = buf + 2 * IN_PLANE;
#pragma unroll
      for (int j = 0; j < DO_PT; ++j) {
        const int idx = p + WS_NP * j;
        const int row = idx >> 5, pr = (idx & 31) >> 3, cg = idx & 7;
        uint32_t *d = dbuf + (cg * 4) * COS + row * 4 + pr;
        const float4 a0 = da[j][0], a1 = da[j][1];
        const int ok = dok[j];
        float v0[4] = {a0.x, a0.y, a0.z, a0.w};
        float v1[4] = {a1.x, a1.y, a1.z, a1.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          v0[c] = (ok & 1) ? v0[c] : 0.f;
          v1[c] = (ok & 2) ? v1[c] : 0.f;
          uint32_t h, m;
          if constexpr (F16) split_x(v0[c] * sy, v1[c] * sy, h, m);
          else split2(v0[c], v1[c], h, m);
          d[c * COS] = h;
          d[DO_PLANE + c * COS] = m;
        }
        if (want_db) {
          dbs.x += v0[0] + v1[0]; dbs.y += v0[1] + v1[1]; dbs.z += v0[2] + v1[2]; dbs.w += v0[3] + v1[3];
        }
      }
    };

    const int b0 = blockIdx.x, g = gridDim.x;
    load(b0);
    store(lds);
    if (n_it > 1) load(b0 + g);
    __syncthreads();   // stage 0 filled
    int cur = 0;
    // iteration it (consumers on brick it): split brick it + 1 (in registers) into the other stage, issue the loads of it + 2
    for (int it = 0; it < n_it; ++it) {
      if (it + 1 < n_it) {
        store(lds + (cur ^ 1) * BUF);
        if (it + 2 < n_it) load(b0 + (it + 2) * g);
      }
      __syncthreads();
      cur ^= 1;
    }
  }

  if (want_db) {  // fixed-order sum of the 32 producer threads per channel group through LDS (free after the last barrier)
    float *sred = reinterpret_cast<float *>(lds);
    if (wave >= 4) {
      const int p = t - WS_NP;
      sred[p * 4 + 0] = dbs.x; sred[p * 4 + 1] = dbs.y; sred[p * 4 + 2] = dbs.z; sred[p * 4 + 3] = dbs.w;
    }
    __syncthreads();
    if (t < 32) {
      const int cg = t >> 2, c = t & 3;
      float sum = 0.f;
      for (int i = 0; i < WS_NP / 8; ++i) sum += sred[(i * 8 + cg) * 4 + c];
      if (co0 + t < s.Co) dbpart[(int64_t)blockIdx.x * s.Co + co0 + t] = sum;
    }
  }
}

// persistent workgroups per channel-tile pair: one workgroup per CU in total (LDS bound)
int x3_parts(int B, int D, int H, int W, int Ci, int Co) {
  int64_t bricks = (int64_t)B * cdiv(D, BRZ) * cdiv(H, BRY) * cdiv(W, BRX);
  int64_t pairs = cdiv(Ci, 32) * cdiv(Co, 32);
  int64_t parts = cdiv(256, pairs);
  if (parts > bricks) parts = bricks;
  return (int)(parts < 1 ? 1 : parts);
}

}  // namespace

extern "C" int64_t svr_conv3d_k3_bwd_weight_bf16x3_workspace(int32_t B, int32_t D, int32_t H, int32_t W, int32_t Ci,
                                                             int32_t Co) {
  int64_t tiles = cdiv(Ci, 32) * cdiv(Co, 32);
  const int64_t parts = x3_parts(B, D, H, W, Ci, Co);
  return (parts * 2 * 27 * tiles * 1024 + parts * Co) * (int64_t)sizeof(float);
}

namespace {
int bwd_weight_x3(const float *in, const float *dout, float *dWp, float *db, int32_t B, int32_t D, int32_t H, int32_t W, int32_t Ci,
                  int32_t Co, void *workspace, void *stream, int param_layout, bool f16 = false, const uint32_t *amax_dout = nullptr);
}

// The kernel choice of the split-precision entry points below, from the shape alone (svr_conv3d_k3_bwd_weight_variant exports
// it; bwd_weight_x3 asks this function, so the two cannot drift).  The wave-specialised kernel when every workgroup gets at
// least WS_MIN_BRICKS bricks (its pipeline fills and drains once per launch, and one consumer wave per SIMD has no partner to
// hide its own latencies), on paired-row tiles for Ci <= 16; the 8-wave kernel for the short launches (the 8^3 layer: 2 bricks
// per workgroup).
int svr::conv3d_bwd_weight_x3_variant(int B, int D, int H, int W, int Ci, int Co, WgradVariant *v) {
  SVR_CHECK(B > 0 && D > 0 && H > 0 && W > 0, SVR_E_BADSHAPE, "conv3d_bwd_weight_bf16x3: empty volume %dx%dx%dx%d", B, D, H, W);
  SVR_CHECK(Ci >= 4 && Ci % 4 == 0 && Co % 4 == 0 && Co >= 4, SVR_E_UNSUPPORTED,
            "conv3d_bwd_weight_bf16x3: need Ci, Co %% 4 == 0 (Ci=%d Co=%d)", Ci, Co);
  // the kernels' 24-bit row multiplies and 32-bit byte offsets inside one sample, 32-bit brick ids
  const int64_t nbricks = (int64_t)B * cdiv(D, BRZ) * cdiv(H, BRY) * cdiv(W, BRX);
  SVR_CHECK((int64_t)D * H * W <= (1LL << 24) && (int64_t)D * H * W * (Ci > Co ? Ci : Co) < (1LL << 30) && nbricks < (1LL << 31),
            SVR_E_UNSUPPORTED, "conv3d_bwd_weight_bf16x3: volume %dx%dx%dx%d too large for 32-bit offsets", B, D, H, W);
  constexpr int WS_MIN_BRICKS = 8;
  v->parts = x3_parts(B, D, H, W, Ci, Co);
  v->per_part = cdiv(nbricks, v->parts);
  v->kernel = nbricks < (int64_t)v->parts * WS_MIN_BRICKS ? SVR_WGRAD_X3 : (Ci <= 16 ? SVR_WGRAD_WS_PAIR : SVR_WGRAD_WS);
  return SVR_OK;
}

// Which kernel a 3x3x3 weight-gradient entry point runs for a shape (host only, no device memory: callable without a GPU).
extern "C" int svr_conv3d_k3_bwd_weight_variant(int32_t op, int32_t B, int32_t D, int32_t H, int32_t W, int32_t Ci, int32_t Co,
                                                int32_t *kernel, int32_t *parts, int64_t *max_bricks_per_part) {
  SVR_CHECK(op >= SVR_CONV_BWD_WEIGHT_F32 && op <= SVR_CONV_BWD_WEIGHT_BF16X3, SVR_E_BADARG, "conv3d_k3_bwd_weight_variant: op %d", op);
  WgradVariant v;
  if (int rc = op == SVR_CONV_BWD_WEIGHT_F32 ? conv3d_bwd_weight_f32_variant(B, D, H, W, Ci, Co, &v)
                                             : conv3d_bwd_weight_x3_variant(B, D, H, W, Ci, Co, &v))
    return rc;
  if (kernel) *kernel = v.kernel;
  if (parts) *parts = v.parts;
  if (max_bricks_per_part) *max_bricks_per_part = v.per_part;
  return SVR_OK;
}

// The weight gradient on the scaled f16 split ("f16x3s": f32 level, see svr_linear_bwd_weight_f16x3); amax_dout: svr_amax_f32 of
// dout (or the amax output of the kernel that produced it).  param_layout != 0: dW(Co,Ci,3,3,3), else the packed [tap][ci][co].
extern "C" int svr_conv3d_k3_bwd_weight_f16x3(const float *in, const float *dout, float *dW, float *db, int32_t B, int32_t D,
                                              int32_t H, int32_t W, int32_t Ci, int32_t Co, int32_t param_layout,
                                              const uint32_t *amax_dout, void *workspace, void *stream) {
  return bwd_weight_x3(in, dout, dW, db, B, D, H, W, Ci, Co, workspace, stream, param_layout ? 1 : 0, true, amax_dout);
}

extern "C" int svr_conv3d_k3_bwd_weight_bf16x3(const float *in, const float *dout, float *dWp, float *db, int32_t B,
                                               int32_t D, int32_t H, int32_t W, int32_t Ci, int32_t Co, void *workspace,
                                               void *stream) {
  return bwd_weight_x3(in, dout, dWp, db, B, D, H, W, Ci, Co, workspace, stream, 0);
}

// The same gradient written straight in the PARAMETER's layout dW(Co,Ci,3,3,3) (what autograd of nn.Conv3d returns):
// no svr_conv3d_unpack_wgrad launch behind it.
extern "C" int svr_conv3d_k3_bwd_weight_bf16x3_param(const float *in, const float *dout, float *dW, float *db, int32_t B,
                                                     int32_t D, int32_t H, int32_t W, int32_t Ci, int32_t Co, void *workspace,
                                                     void *stream) {
  return bwd_weight_x3(in, dout, dW, db, B, D, H, W, Ci, Co, workspace, stream, 1);
}

namespace {
int bwd_weight_x3(const float *in, const float *dout, float *dWp, float *db, int32_t B, int32_t D, int32_t H, int32_t W, int32_t Ci,
                  int32_t Co, void *workspace, void *stream, int param_layout, bool f16, const uint32_t *amax_dout) {
  SVR_CHECK(B > 0 && D > 0 && H > 0 && W > 0, SVR_E_BADSHAPE, "conv3d_bwd_weight_bf16x3: empty volume %dx%dx%dx%d", B, D, H, W);
  SVR_CHECK(in && dout && dWp && workspace, SVR_E_BADARG, "conv3d_bwd_weight_bf16x3: null pointer");
  WgradVariant v;
  if (int rc = conv3d_bwd_weight_x3_variant(B, D, H, W, Ci, Co, &v)) return rc;
  SVR_CHECK((((uintptr_t)in | (uintptr_t)dout) & 15) == 0, SVR_E_ALIGN, "conv3d_bwd_weight_bf16x3: 16-byte alignment");
  hipStream_t s = (hipStream_t)stream;
  ConvShape sh{B, D, H, W, Ci, Co};
  const int cit = (int)cdiv(Ci, 32), cot = (int)cdiv(Co, 32);
  const int nbz = (int)cdiv(D, BRZ), nby = (int)cdiv(H, BRY), nbx = (int)cdiv(W, BRX);
  const int parts = v.parts;
  float *slab = (float *)workspace;
  float *dbpart = db ? slab + (int64_t)parts * 2 * 27 * cit * cot * 1024 : nullptr;
  if (v.kernel != SVR_WGRAD_X3) {
    const dim3 grid((unsigned)parts, (unsigned)(cit * cot));
    const uint32_t *am = f16 ? amax_dout : nullptr;
    if (v.kernel == SVR_WGRAD_WS_PAIR) {
      if (f16) hipLaunchKernelGGL((conv3d_bwd_weight_ws_kernel<true, true>), grid, dim3(NT), 0, s, in, dout, slab, sh, nbz, nby, nbx, cot, dbpart, am);
      else hipLaunchKernelGGL((conv3d_bwd_weight_ws_kernel<false, true>), grid, dim3(NT), 0, s, in, dout, slab, sh, nbz, nby, nbx, cot, dbpart, am);
    } else {
      if (f16) hipLaunchKernelGGL((conv3d_bwd_weight_ws_kernel<true, false>), grid, dim3(NT), 0, s, in, dout, slab, sh, nbz, nby, nbx, cot, dbpart, am);
      else hipLaunchKernelGGL((conv3d_bwd_weight_ws_kernel<false, false>), grid, dim3(NT), 0, s, in, dout, slab, sh, nbz, nby, nbx, cot, dbpart, am);
    }
    conv3d_bwd_weight_reduce_launch(slab, dWp, Ci, Co, cit, cot, parts, s, param_layout, dbpart, db, parts);
    return launch_status("conv3d_bwd_weight_bf16x3");
  }
  if (f16)
    hipLaunchKernelGGL(conv3d_bwd_weight_x3_kernel<true>, dim3((unsigned)parts, (unsigned)(cit * cot)), dim3(NT), 0, s, in, dout,
                       slab, sh, nbz, nby, nbx, cot, dbpart, amax_dout);
  else
    hipLaunchKernelGGL(conv3d_bwd_weight_x3_kernel<false>, dim3((unsigned)parts, (unsigned)(cit * cot)), dim3(NT), 0, s, in, dout,
                       slab, sh, nbz, nby, nbx, cot, dbpart, (const uint32_t *)nullptr);
  // one launch: slabs -> dW (either layout) and, in its last Co workgroups, the bias-gradient partials -> db
  conv3d_bwd_weight_reduce_launch(slab, dWp, Ci, Co, cit, cot, parts * 2, s, param_layout, dbpart, db, parts);
  return launch_status("conv3d_bwd_weight_bf16x3");
}
}  // namespace
