// Depth head of the UNet regressor (trainer/trainer_unet.py:43-61 of the reference) in one forward and one backward kernel:
//
//   y     = F.interpolate(raw, size=S, mode='bilinear')[:, :, r0:r1, :]        (S == 0: y = raw)
//   depth = sigmoid(y) * (max_z - min_z) + min_z
//   loss  = mean((depth - target)^2)
//
// Compiled with -ffp-contract=off: source index, weights and the four-tap sum round as ATen's CPU kernel rounds them
// (UpSample.h: area_pixel_compute_source_index, compute_indices_weights), each product and sum on its own.
//
// Forward: one thread per CROPPED destination pixel, grid-stride; rows outside r0:r1 are never computed.  With a target
// every block leaves the f64 sum of its squared differences in the caller's workspace and a one-wave kernel adds the block
// sums in a fixed order.  With `gdst` the forward also leaves d loss / d y per destination pixel (for unit upstream gradient).
// Backward: the transposed interpolation in GATHER form, one thread per source pixel: it inverts the index map approximately
// to a candidate range of destination rows / columns and confirms every candidate with the forward's own tap() -- so the
// backward is the exact transpose of the forward at every scale, sums in a fixed order, needs no atomics and writes an
// exact 0 where no cropped destination pixel touches the source pixel.
#include "common.h"

using namespace svr;

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxBlocks = 1024;

struct Tap {
  int i0, i1;
  float l0, l1;
};

// destination index -> the two source taps and their weights (align_corners=False)
__device__ __forceinline__ Tap tap(int dst, float scale, int in) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  Tap t;
  t.i0 = (int)src;
  if (t.i0 > in - 1) t.i0 = in - 1;      // cannot happen for dst < out (src < in - 1/2); keeps every read in bounds
  t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
  t.l1 = src - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// weight of source index s in destination index dst (0 if dst does not touch s); *hit says whether it touches
__device__ __forceinline__ float tap_weight(int dst, float scale, int in, int s, bool *hit) {
  Tap t = tap(dst, scale, in);
  float w = 0.f;
  if (t.i0 == s) w = t.l0;
  if (t.i1 == s) w = w + t.l1;
  *hit = t.i0 == s || t.i1 == s;
  return w;
}

// candidate destination range [lo, hi] (clamped to [first, last]) of the indices that may touch source index s:
// src in (s - 1, s + 1)  <=>  dst in ((s - 1/2) / scale - 1/2, (s + 3/2) / scale - 1/2), widened by one on each side.
// Destinations whose source index is clamped to 0 lie below the lower end of s = 0, which is negative.
__device__ __forceinline__ void candidates(int s, float scale, int first, int last, int *lo, int *hi) {
  float a = floorf(((float)s - 0.5f) / scale - 0.5f) - 1.f;
  float b = ceilf(((float)s + 1.5f) / scale - 0.5f) + 1.f;
  *lo = a < (float)first ? first : (a > (float)last ? last + 1 : (int)a);
  *hi = b > (float)last ? last : (b < (float)first ? first - 1 : (int)b);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

__global__ __launch_bounds__(kThreads) void depth_head_fwd_kernel(
    const float *__restrict__ raw, const float *__restrict__ target, float *__restrict__ depth, float *__restrict__ gdst,
    double *__restrict__ partial, int64_t n, int Hs, int Ws, int Ho, int Wo, int resize, int r0, float scale_y, float scale_x,
    float min_z, float max_z, float range, float norm) {
  double acc = 0.0;
  const int64_t plane = (int64_t)Hs * Ws;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    float y;
    if (resize) {
      const int x = (int)(i % Wo);
      const int64_t q = i / Wo;
      const int r = (int)(q % Ho);
      const float *src = raw + (q / Ho) * plane;
      const Tap ty = tap(r + r0, scale_y, Hs), tx = tap(x, scale_x, Ws);
      const float *p0 = src + (int64_t)ty.i0 * Ws, *p1 = src + (int64_t)ty.i1 * Ws;
      const float a00 = p0[tx.i0], a01 = p0[tx.i1], a10 = p1[tx.i0], a11 = p1[tx.i1];
      y = ty.l0 * (tx.l0 * a00 + tx.l1 * a01) + ty.l1 * (tx.l0 * a10 + tx.l1 * a11);
    } else {
      y = raw[i];
    }
    const float s = 1.f / (1.f + expf(-y));
    // s in [0, 1]: the sum is >= min_z; its rounding may pass max_z by one ulp, which the bound takes back
    const float d = fminf(s * range + min_z, max_z);
    depth[i] = d;
    if (target) {
      const float e = d - target[i];
      acc += (double)e * (double)e;
      // mse_loss -> mul -> sigmoid backward, in autograd's order: (2/n * e) * range * (1 - s) * s
      if (gdst) gdst[i] = norm * e * range * (1.f - s) * s;
    }
  }
  if (!target) return;
  __shared__ double red[kThreads / 64];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(64) void depth_head_loss_kernel(const double *__restrict__ partial, float *__restrict__ loss, int blocks,
                                                             double n) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < blocks; i += 64) acc += partial[i];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) loss[0] = (float)(acc / n);
}

__global__ __launch_bounds__(kThreads) void depth_head_bwd_kernel(const float *__restrict__ gdst, float *__restrict__ draw, int64_t n_src,
                                                                  int Hs, int Ws, int Ho, int Wo, int r0, float scale_y,
                                                                  float scale_x) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_src) return;
  const int sx = (int)(i % Ws);
  const int64_t q = i / Ws;
  const int sy = (int)(q % Hs);
  const float *g = gdst + (q / Hs) * ((int64_t)Ho * Wo);
  int ylo, yhi, xlo, xhi;
  candidates(sy, scale_y, r0, r0 + Ho - 1, &ylo, &yhi);
  candidates(sx, scale_x, 0, Wo - 1, &xlo, &xhi);
  float acc = 0.f;
  for (int dy = ylo; dy <= yhi; ++dy) {
    bool hit;
    const float wy = tap_weight(dy, scale_y, Hs, sy, &hit);
    if (!hit) continue;
    const float *row = g + (int64_t)(dy - r0) * Wo;
    float racc = 0.f;
    for (int dx = xlo; dx <= xhi; ++dx) {
      const float wx = tap_weight(dx, scale_x, Ws, sx, &hit);
      if (hit) racc += wx * row[dx];
    }
    acc += wy * racc;
  }
  draw[i] = acc;
}

constexpr int64_t kMaxPixels = (int64_t)1 << 38;

// B * H * W of positive extents, saturated at kMaxPixels (the plain product of three int32 can pass 2^63)
int64_t pixels(int32_t B, int32_t H, int32_t W) {
  const int64_t bh = (int64_t)B * H;
  return bh > kMaxPixels / W ? kMaxPixels : bh * W;
}

int64_t fwd_blocks(int64_t n) {
  int64_t b = cdiv(n, kThreads);
  return b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b);
}

// shapes of both entry points; Ho / Wo of the output
int check_shape(const char *what, int32_t B, int32_t Hs, int32_t Ws, int32_t S, int32_t r0, int32_t r1, int32_t *Ho, int32_t *Wo) {
  SVR_CHECK(B > 0 && Hs > 0 && Ws > 0 && S >= 0, SVR_E_BADSHAPE, "%s: B=%d Hs=%d Ws=%d S=%d", what, B, Hs, Ws, S);
  if (S == 0) {
    *Ho = Hs;
    *Wo = Ws;
  } else {
    SVR_CHECK(r0 >= 0 && r0 < r1 && r1 <= S, SVR_E_BADSHAPE, "%s: rows %d:%d of %d", what, r0, r1, S);
    *Ho = r1 - r0;
    *Wo = S;
  }
  // (the backward's grid is one block per 256 source pixels: fewer than 2^31 blocks)
  SVR_CHECK(pixels(B, Hs, Ws) < kMaxPixels && pixels(B, *Ho, *Wo) < kMaxPixels, SVR_E_BADSHAPE, "%s: 2^38 pixels or more", what);
  return SVR_OK;
}

}  // namespace

extern "C" int64_t svr_depth_head_workspace(int32_t B, int32_t Ho, int32_t Wo) {
  if (B <= 0 || Ho <= 0 || Wo <= 0) return (int64_t)sizeof(double);
  return fwd_blocks(pixels(B, Ho, Wo)) * (int64_t)sizeof(double);
}

extern "C" int svr_depth_head_fwd(const float *raw, const float *target, float *depth, float *loss, float *gdst, int32_t B,
                                  int32_t Hs, int32_t Ws, int32_t S, int32_t r0, int32_t r1, double min_z, double max_z,
                                  void *workspace, void *stream) {
  int32_t Ho, Wo;
  if (int rc = check_shape("depth_head_fwd", B, Hs, Ws, S, r0, r1, &Ho, &Wo)) return rc;
  SVR_CHECK(raw && depth, SVR_E_BADARG, "depth_head_fwd: null pointer");
  SVR_CHECK(!target || (loss && workspace), SVR_E_BADARG, "depth_head_fwd: a target needs loss and workspace");
  SVR_CHECK(target || !gdst, SVR_E_BADARG, "depth_head_fwd: a gradient needs a target");
  SVR_CHECK(max_z >= min_z, SVR_E_BADARG, "depth_head_fwd: min_z=%g > max_z=%g", min_z, max_z);
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)B * Ho * Wo;
  const int64_t blocks = fwd_blocks(n);
  const float scale_y = S ? (float)Hs / (float)S : 1.f, scale_x = S ? (float)Ws / (float)S : 1.f;
  hipLaunchKernelGGL(depth_head_fwd_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, raw, target, depth, gdst,
                     (double *)workspace, n, Hs, Ws, Ho, Wo, S ? 1 : 0, r0, scale_y, scale_x, (float)min_z, (float)max_z,
                     (float)(max_z - min_z), (float)(2.0 / (double)n));
  if (target)
    hipLaunchKernelGGL(depth_head_loss_kernel, dim3(1), dim3(64), 0, s, (const double *)workspace, loss, (int)blocks, (double)n);
  return launch_status("depth_head_fwd");
}

extern "C" int svr_depth_head_bwd(const float *gdst, float *draw, int32_t B, int32_t Hs, int32_t Ws, int32_t S, int32_t r0,
                                  int32_t r1, void *stream) {
  int32_t Ho, Wo;
  if (int rc = check_shape("depth_head_bwd", B, Hs, Ws, S, r0, r1, &Ho, &Wo)) return rc;
  SVR_CHECK(S > 0, SVR_E_BADARG, "depth_head_bwd: identity mode has no backward pass (gdst is d raw)");
  SVR_CHECK(gdst && draw, SVR_E_BADARG, "depth_head_bwd: null pointer");
  const int64_t n_src = (int64_t)B * Hs * Ws;
  hipLaunchKernelGGL(depth_head_bwd_kernel, dim3((unsigned)cdiv(n_src, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, gdst,
                     draw, n_src, Hs, Ws, Ho, Wo, r0, (float)Hs / (float)S, (float)Ws / (float)S);
  return launch_status("depth_head_bwd");
}
