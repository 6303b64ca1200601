// Device helpers of the split-precision kernels, defined once: the vector types, the scaled f16 split ("f16x3", see
// gemm_f16x3.hip for the arithmetic), the bf16 splits ("bf16x3" / "bf16x6", gemm_bf16x3.hip / gemm_bf16x6.hip) and the
// conflict-free 16-byte LDS slot with its fragment reads.  Everything is __forceinline__: a translation unit built with
// -ffp-contract=off (gather_fc0.hip, bf16_path.hip) gets these bodies under its own flags.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- f16 split ----
__device__ __forceinline__ uint32_t pack_f16(float a, float b) {
  f32x2 v = {a, b};
  f16x2 h = __builtin_convertvector(v, f16x2);  // round to nearest even
  return __builtin_bit_cast(uint32_t, h);
}
__device__ __forceinline__ f32x2 unpack_f16(uint32_t p) {
  return __builtin_convertvector(__builtin_bit_cast(f16x2, p), f32x2);
}

// (x0, x1) -> packed hi pair, packed (lo * 2^11) pair
__device__ __forceinline__ void split_x(float x0, float x1, uint32_t &hi, uint32_t &lo) {
  hi = pack_f16(x0, x1);
  const f32x2 h = unpack_f16(hi);
  lo = pack_f16((x0 - h.x) * 2048.f, (x1 - h.y) * 2048.f);
}

// Weights (already multiplied by w_scale): hi = rn16(w), lo = rn16(w - hi) -- lo is NOT scaled by 2^11, unlike split_x: the
// kernels make wq = hi 2^-11 in registers (scale_2m11) instead.
__device__ __forceinline__ void split_w(float w0, float w1, uint32_t &hi, uint32_t &lo) {
  hi = pack_f16(w0, w1);
  const f32x2 h = unpack_f16(hi);
  lo = pack_f16(w0 - h.x, w1 - h.y);
}
__device__ __forceinline__ void split_w(float w, _Float16 &hi, _Float16 &lo) {  // one value; the same roundings
  hi = (_Float16)w;  // round to nearest even, like pack_f16
  lo = (_Float16)(w - (float)hi);
}

__device__ __forceinline__ f16x8 scale_2m11(f16x8 v) {  // exact: every normal hi(Ws) stays normal (see gemm_f16x3.hip)
  return v * (_Float16)(1.f / 2048.f);
}

// 2^s (or 2^-s) with amax * 2^s in [2^13, 2^14); s = 0 for an all-zero or non-finite W.  amax_bits: what svr::w_amax_launch
// (gemm_f16x3.hip) or svr_amax_publish leaves.
__device__ __forceinline__ float w_scale(uint32_t amax_bits, bool inverse) {
  const float amax = __uint_as_float(amax_bits);
  int e = 0;
  if (amax > 0.f && amax < 3.0e38f) {
    frexpf(amax, &e);  // amax = f * 2^e, f in [0.5, 1)
    e = 14 - e;
    e = e > 100 ? 100 : (e < -100 ? -100 : e);
  }
  return ldexpf(1.f, inverse ? -e : e);
}

// ---- bf16 splits ----
__device__ __forceinline__ float bf_lo(uint32_t p) { return __uint_as_float(p << 16); }          // element 0 of a pair
__device__ __forceinline__ float bf_hi(uint32_t p) { return __uint_as_float(p & 0xffff0000u); }  // element 1
__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {  // round to nearest even (v_cvt_pk_bf16_f32), NaN safe
  f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// (x0, x1) -> packed bf16 pairs hi = bf16_rne(x), mid = bf16_rne(x - hi)
__device__ __forceinline__ void split2(float x0, float x1, uint32_t &hi, uint32_t &mid) {
  hi = pack_bf16(x0, x1);
  mid = pack_bf16(x0 - bf_lo(hi), x1 - bf_hi(hi));
}
// ... and lo = bf16_rne((x - hi) - mid): three terms carry 24 mantissa bits
__device__ __forceinline__ void split3(float x0, float x1, uint32_t &hi, uint32_t &mid, uint32_t &lo) {
  split2(x0, x1, hi, mid);
  lo = pack_bf16((x0 - bf_lo(hi)) - bf_lo(mid), (x1 - bf_hi(hi)) - bf_hi(mid));
}

// ---- LDS operand tiles ----
// A fragment = 8 consecutive k (16-bit values) of one row = 16 bytes, and it has to come out of ONE ds_read_b128 (256 B/clk;
// the 8-byte aligned padded rows of the first version made it a ds_read2_b64: 128 B/clk, and at one fragment KB per MFMA the
// convolutions saturated exactly that).  ds_read_b128 serves a wave in four groups of 16 lanes, {0-3,12-15,20-27},
// {4-11,16-19,28-31} and the same + 32 (MI355X_MICROARCH.md "LDS"), conflict free when the 16 lanes hit 16 different 16-byte
// slots mod 16.  Rows are SL slots wide without padding (SL = 2: 16 values per row, one k-step of the GEMMs; SL = 4: the
// 32-channel chunks of conv3d_bf16.hip), slot = SL*row + (sub ^ g(row)) with g = bit 3 of the row (SL = 2) or bits 2-3
// (SL = 4).  With row = lane & 31 the rows of a group pair up mod 8 at distances 8 and 24, so its 16 lanes hit 16 different
// slots mod 16.  (conv3d_bf16.hip's halo tile reaches the same row pattern through its lane -> voxel map, see there.)
template <int SL = 2>
__device__ __forceinline__ int slot_dw(int row, int sub) {  // dword offset of slot `sub` of a row
  static_assert(SL == 2 || SL == 4, "16- or 32-value rows");
  const int g = SL == 2 ? (row >> 3) & 1 : (row >> 2) & 3;
  return (row * SL + (sub ^ g)) * 4;
}
__device__ __forceinline__ f16x8 frag_f16(const uint32_t *p) {  // 8 halves at a 16-byte aligned address
  union { uint4 q; f16x8 v; } f;
  f.q = *reinterpret_cast<const uint4 *>(p);
  return f.v;
}
__device__ __forceinline__ bf16x8 frag_bf16(const uint32_t *p) {  // the same 16 bytes as 8 bf16
  union { uint4 q; bf16x8 v; } f;
  f.q = *reinterpret_cast<const uint4 *>(p);
  return f.v;
}

}  // namespace
