// RGB preprocessing of the scene network's input on the device (dataset/scene_net_data.py: rgb_transform):
//
//   [FLIP_LEFT_RIGHT] -> SquarePad(0) -> Image.resize((W, W), Image.BILINEAR) -> ToTensor -> Normalize(0.5, 0.5)
//
// and the reconstruction's vertex affine back to camera space.  The resize is Pillow's 8-bit resampler (Resample.c:
// precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc) restated: per axis a table of
// {first source index, tap count, 22-bit fixed-point taps} per output index, built on the HOST in double
// (svr_rgb_resize_table); a pass is  clamp((2^21 + sum in[xmin + t] * k[t]) >> 22, 0, 255)  per band in int32
// (255 * 2^22 + 2^21 < 2^31), horizontal first into an 8-bit intermediate, then vertical on that.  A pass whose input and
// output sizes agree is skipped, as Pillow skips it.  The pad is never materialised: a read outside the image is a 0 that
// takes part in the filter, and the flip is a mirrored column index of the read.
//
// One thread per output pixel, all bands; the tap loop runs over the table's runtime count (2-3 taps when upscaling, ~87
// for 300 -> 7).  Every source read is bounds-checked against the image (that check IS the pad) and the count is capped at
// the table's stride, so no table content can make a thread read outside `src` or its own table row.
// The float output is norm[u]: a 256-entry table the caller fills with the float32 operations it wants reproduced
// (u/255, then (x - 0.5)/0.5) -- bit equality with the host transform by construction.
// Compiled with -ffp-contract=off: the host table code rounds every double operation on its own, like Pillow's C.
#include "common.h"
#include <math.h>

using namespace svr;

namespace {

constexpr int kThreads = 256;
constexpr int kPrecisionBits = 32 - 8 - 2;
constexpr int64_t kMaxElems = ((int64_t)1 << 31) - 1;

// the padded (and flipped) image as the passes see it
struct Source {
  const uint8_t *p;
  int H, W;      // stored extent
  int vp, hp;    // rows / columns of zeros in front
  int flip;      // stored column = W - 1 - column
};

template <int C>
__device__ __forceinline__ void fetch(const Source &s, int b, int y, int x, int (&v)[C]) {
  y -= s.vp;
  x -= s.hp;
  if (y < 0 || y >= s.H || x < 0 || x >= s.W) {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = 0;
    return;
  }
  if (s.flip) x = s.W - 1 - x;
  const uint8_t *q = s.p + (((int64_t)b * s.H + y) * s.W + x) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = q[c];
}

// AXIS 0: copy; 1: resample along x (table row per output column); 2: along y (table row per output row).
// out_u8 (B, Ho, Wo, C) and out_f32 (B, C, Ho, Wo) may each be null.
template <int C, int AXIS>
__global__ __launch_bounds__(kThreads) void rgb_pass_kernel(Source s, const int32_t *__restrict__ table, int K, int Ho, int Wo,
                                                            uint8_t *__restrict__ out_u8, float *__restrict__ out_f32,
                                                            const float *__restrict__ norm, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % Wo);
  const int64_t q = i / Wo;
  const int y = (int)(q % Ho);
  const int b = (int)(q / Ho);
  int r[C];
  if (AXIS == 0) {
    fetch<C>(s, b, y, x, r);
  } else {
    const int32_t *row = table + (int64_t)(AXIS == 1 ? x : y) * (K + 2);
    const int first = row[0];
    int count = row[1];
    if (count > K) count = K;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (kPrecisionBits - 1);
    for (int t = 0; t < count; ++t) {
      const int k = row[2 + t];
      int v[C];
      if (AXIS == 1)
        fetch<C>(s, b, y, first + t, v);
      else
        fetch<C>(s, b, first + t, x, v);
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += v[c] * k;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int a = acc[c] >> kPrecisionBits;
      r[c] = a < 0 ? 0 : (a > 255 ? 255 : a);
    }
  }
  if (out_u8) {
#pragma unroll
    for (int c = 0; c < C; ++c) out_u8[i * C + c] = (uint8_t)r[c];
  }
  if (out_f32) {
    const int64_t plane = (int64_t)Ho * Wo;
#pragma unroll
    for (int c = 0; c < C; ++c) out_f32[((int64_t)b * C + c) * plane + (int64_t)y * Wo + x] = norm[r[c]];
  }
}

template <int C>
void launch_pass(int axis, const Source &s, const int32_t *table, int K, int B, int Ho, int Wo, uint8_t *out_u8, float *out_f32,
                 const float *norm, hipStream_t st) {
  const int64_t n = (int64_t)B * Ho * Wo;
  const dim3 grid((unsigned)cdiv(n, kThreads)), block(kThreads);
  if (axis == 0)
    hipLaunchKernelGGL((rgb_pass_kernel<C, 0>), grid, block, 0, st, s, table, K, Ho, Wo, out_u8, out_f32, norm, n);
  else if (axis == 1)
    hipLaunchKernelGGL((rgb_pass_kernel<C, 1>), grid, block, 0, st, s, table, K, Ho, Wo, out_u8, out_f32, norm, n);
  else
    hipLaunchKernelGGL((rgb_pass_kernel<C, 2>), grid, block, 0, st, s, table, K, Ho, Wo, out_u8, out_f32, norm, n);
}

template <int C>
void run_passes(const uint8_t *src, int B, int H, int W, int Wout, int flip, const int32_t *table_x, int Kx, const int32_t *table_y,
                int Ky, const float *norm, uint8_t *tmp, uint8_t *out_u8, float *out_f32, hipStream_t st) {
  Source s{src, H, W, 0, 0, flip};
  if (!Wout) {
    launch_pass<C>(0, s, nullptr, 0, B, H, W, out_u8, out_f32, norm, st);
    return;
  }
  const int m = H > W ? H : W;
  s.hp = (m - W) / 2;
  s.vp = (m - H) / 2;
  const int Hp = H + 2 * s.vp, Wp = W + 2 * s.hp;
  const bool px = Wp != Wout, py = Hp != Wout;
  if (px && py) {
    launch_pass<C>(1, s, table_x, Kx, B, Hp, Wout, tmp, nullptr, norm, st);
    const Source mid{tmp, Hp, Wout, 0, 0, 0};
    launch_pass<C>(2, mid, table_y, Ky, B, Wout, Wout, out_u8, out_f32, norm, st);
  } else if (px) {
    launch_pass<C>(1, s, table_x, Kx, B, Wout, Wout, out_u8, out_f32, norm, st);
  } else if (py) {
    launch_pass<C>(2, s, table_y, Ky, B, Wout, Wout, out_u8, out_f32, norm, st);
  } else {
    launch_pass<C>(0, s, nullptr, 0, B, Wout, Wout, out_u8, out_f32, norm, st);
  }
}

__global__ __launch_bounds__(kThreads) void grid_to_camera_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t n,
                                                                  float s0, float t0, float s1, float t1, float s2, float t2) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  dst[3 * i + 0] = (src[3 * i + 0] - t0) / s0;
  dst[3 * i + 1] = (src[3 * i + 1] - t1) / s1;
  dst[3 * i + 2] = (src[3 * i + 2] - t2) / s2;
}

// Pillow's filter support for BILINEAR is 1.0
double filter_scale(int32_t in, int32_t out) {
  const double scale = (double)in / out;
  return scale < 1.0 ? 1.0 : scale;
}

// Pillow's bilinear_filter
double triangle(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

}  // namespace

extern "C" int32_t svr_rgb_resize_taps(int32_t in, int32_t out) {
  SVR_CHECK(in > 0 && out > 0, SVR_E_BADSHAPE, "rgb_resize_taps: in=%d out=%d", in, out);
  const double support = 1.0 * filter_scale(in, out);
  SVR_CHECK(support < (double)(1 << 20), SVR_E_BADSHAPE, "rgb_resize_taps: in=%d out=%d", in, out);
  return (int32_t)ceil(support) * 2 + 1;
}

extern "C" int svr_rgb_resize_table(int32_t in, int32_t out, int32_t K, int32_t *table) {
  const int32_t need = svr_rgb_resize_taps(in, out);
  if (need < 0) return need;
  SVR_CHECK(table, SVR_E_BADARG, "rgb_resize_table: null table");
  SVR_CHECK(K >= need, SVR_E_BADARG, "rgb_resize_table: stride %d for up to %d taps", K, need);
  const double scale = (double)in / out, fs = filter_scale(in, out);
  const double support = 1.0 * fs, ss = 1.0 / fs;
  for (int32_t xx = 0; xx < out; ++xx) {
    int32_t *row = table + (int64_t)xx * (K + 2);
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    if (xmax > K) xmax = K;      // cannot happen: xmax - xmin <= 2 * support + 1 <= need
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += triangle((x + xmin - center + 0.5) * ss);
    row[0] = xmin;
    row[1] = xmax;
    for (int x = 0; x < K; ++x) {
      double v = x < xmax ? triangle((x + xmin - center + 0.5) * ss) : 0.0;
      if (ww != 0.0) v /= ww;
      row[2 + x] = v < 0 ? (int)(-0.5 + v * (1 << kPrecisionBits)) : (int)(0.5 + v * (1 << kPrecisionBits));
    }
  }
  return SVR_OK;
}

extern "C" int svr_rgb_preprocess(const uint8_t *src, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Wout, int32_t flip,
                                  const int32_t *table_x, int32_t Kx, const int32_t *table_y, int32_t Ky, const float *norm,
                                  uint8_t *tmp, uint8_t *out_u8, float *out_f32, void *stream) {
  SVR_CHECK(B > 0 && H > 0 && W > 0 && Wout >= 0, SVR_E_BADSHAPE, "rgb_preprocess: B=%d H=%d W=%d Wout=%d", B, H, W, Wout);
  SVR_CHECK(C == 1 || C == 3, SVR_E_UNSUPPORTED, "rgb_preprocess: %d bands (1 or 3)", C);
  SVR_CHECK(src && (out_u8 || out_f32), SVR_E_BADARG, "rgb_preprocess: null source, or no output");
  SVR_CHECK(!out_f32 || norm, SVR_E_BADARG, "rgb_preprocess: the float output needs the 256-entry norm table");
  const int64_t m = H > W ? H : W, o = Wout ? Wout : m;
  SVR_CHECK((int64_t)B * m * m * C <= kMaxElems && (int64_t)B * m * o * C <= kMaxElems && (int64_t)B * o * o * C <= kMaxElems,
            SVR_E_BADSHAPE, "rgb_preprocess: 2^31 elements or more");
  if (Wout) {
    const int Hp = H + 2 * (int)((m - H) / 2), Wp = W + 2 * (int)((m - W) / 2);
    const bool px = Wp != Wout, py = Hp != Wout;
    SVR_CHECK(!px || (table_x && Kx > 0), SVR_E_BADARG, "rgb_preprocess: columns %d -> %d need table_x", Wp, Wout);
    SVR_CHECK(!py || (table_y && Ky > 0), SVR_E_BADARG, "rgb_preprocess: rows %d -> %d need table_y", Hp, Wout);
    SVR_CHECK(!(px && py) || tmp, SVR_E_BADARG, "rgb_preprocess: two passes need the intermediate");
  }
  hipStream_t st = (hipStream_t)stream;
  if (C == 3)
    run_passes<3>(src, B, H, W, Wout, flip ? 1 : 0, table_x, Kx, table_y, Ky, norm, tmp, out_u8, out_f32, st);
  else
    run_passes<1>(src, B, H, W, Wout, flip ? 1 : 0, table_x, Kx, table_y, Ky, norm, tmp, out_u8, out_f32, st);
  return launch_status("rgb_preprocess");
}

extern "C" int svr_grid_to_camera(const float *src, float *dst, int64_t n, const float *scale_shift, void *stream) {
  SVR_CHECK(n >= 0 && n <= kMaxElems, SVR_E_BADSHAPE, "grid_to_camera: n=%lld", (long long)n);
  SVR_CHECK(scale_shift && (n == 0 || (src && dst)), SVR_E_BADARG, "grid_to_camera: null pointer");
  const float *k = scale_shift;
  SVR_CHECK(k[0] != 0.f && k[2] != 0.f && k[4] != 0.f, SVR_E_BADARG, "grid_to_camera: zero scale");
  if (n == 0) return SVR_OK;
  hipLaunchKernelGGL(grid_to_camera_kernel, dim3((unsigned)cdiv(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, src, dst, n,
                     k[0], k[1], k[2], k[3], k[4], k[5]);
  return launch_status("grid_to_camera");
}
