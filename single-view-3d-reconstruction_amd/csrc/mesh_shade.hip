// Shading pass over the ray caster's face map, and the box filter behind supersampling, gfx950.
//
// The rule is written down in include/svr_hip.h and restated in numpy by tests/mesh_render_oracle.py.
//   svr_mesh_shade           ms_shade_kernel       one thread per pixel: shade_pixel() of csrc/shade_pixel.h -- the winner's
//                                                  barycentrics again by ray_triangle's expressions, the interpolated vertex
//                                                  normal (or the face's), the head light, the interpolated vertex colour (or
//                                                  the albedo), three bytes
//   svr_box_downsample_rgb8  ms_downsample_kernel  one thread per output pixel: the rounded mean of its s x s block, in integers
// No LDS and no atomics: a pixel reads its own face's nine doubles, three indices and up to three normals and colours, all
// from cache for neighbouring pixels of one face, and owns its three output bytes.  Built with -ffp-contract=off: float64, one
// rounding per operation, so the bytes equal the oracle's.
// Bounds: a face-map entry outside [0, F) and a vertex index outside [0, V) are never turned into an address (shade_pixel);
// both kernels return for a pixel outside the image.
#include "common.h"
#include "shade_pixel.h"

using namespace svr;

namespace {

constexpr int kBlock = 256;

struct ShadeArgs {
  double k[9];                                     // f, cx, cy, s00, t0, s11, t1, s22, t2, widened
  double ambient;
  uint8_t albedo[3], background[3];
};

__global__ __launch_bounds__(kBlock) void ms_shade_kernel(const double *__restrict__ tri, const int32_t *__restrict__ faces, int64_t F, int64_t V,
                                                          const int32_t *__restrict__ face_map, int32_t H, int32_t W,
                                                          const float *__restrict__ normals, const uint8_t *__restrict__ colors, ShadeArgs a,
                                                          uint8_t *__restrict__ rgb) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int v = (int)(p / W), u = (int)(p - (int64_t)v * W);
  uint8_t px[3];
  shade_pixel(u, v, face_map[p], tri, faces, F, V, normals, colors, a.k, a.albedo, a.background, a.ambient, px);
  rgb[p * 3 + 0] = px[0];
  rgb[p * 3 + 1] = px[1];
  rgb[p * 3 + 2] = px[2];
}

__global__ __launch_bounds__(kBlock) void ms_downsample_kernel(const uint8_t *__restrict__ src, int32_t H, int32_t W, int32_t s,
                                                               uint8_t *__restrict__ dst) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int64_t r = p / W, c = p - r * W;
  uint32_t sum[3] = {0, 0, 0};
  for (int32_t i = 0; i < s; ++i) {
    const uint8_t *row = src + ((r * s + i) * ((int64_t)W * s) + c * s) * 3;
    for (int32_t j = 0; j < s * 3; j += 3) {
      sum[0] += row[j + 0];
      sum[1] += row[j + 1];
      sum[2] += row[j + 2];
    }
  }
  const uint32_t n = (uint32_t)(s * s);
  dst[p * 3 + 0] = (uint8_t)((sum[0] + n / 2) / n);
  dst[p * 3 + 1] = (uint8_t)((sum[1] + n / 2) / n);
  dst[p * 3 + 2] = (uint8_t)((sum[2] + n / 2) / n);
}

bool image_ok(int32_t H, int32_t W) { return H >= 1 && H <= 32768 && W >= 1 && W <= 32768; }

}  // namespace

extern "C" int svr_mesh_shade(const double *tri, const int32_t *faces, int64_t F, int64_t V, const int32_t *face_map, const float *consts,
                              int32_t H, int32_t W, const float *normals, const uint8_t *colors, const uint8_t *albedo,
                              const uint8_t *background, float ambient, uint8_t *rgb, void *stream) {
  SVR_CHECK(image_ok(H, W), SVR_E_BADSHAPE, "mesh_shade: image %d x %d (need 1 <= H, W <= 32768)", H, W);
  SVR_CHECK(F >= 0 && F < (1LL << 31) && V >= 0 && V < (1LL << 31), SVR_E_BADSHAPE, "mesh_shade: F=%ld V=%ld (need 0 <= F, V < 2^31)", (long)F,
            (long)V);
  SVR_CHECK(face_map && consts && albedo && background && rgb && (tri || F == 0), SVR_E_BADARG, "mesh_shade: null pointer");
  SVR_CHECK(!(normals || colors) || faces || F == 0, SVR_E_BADARG, "mesh_shade: normals or colors without faces");
  SVR_CHECK(ambient >= 0.0f && ambient <= 1.0f, SVR_E_BADARG, "mesh_shade: ambient=%g (need 0 <= ambient <= 1)", (double)ambient);
  ShadeArgs a;
  for (int i = 0; i < 9; ++i) a.k[i] = (double)consts[i];
  a.ambient = (double)ambient;
  for (int i = 0; i < 3; ++i) a.albedo[i] = albedo[i], a.background[i] = background[i];
  const int64_t pixels = (int64_t)H * W;
  hipLaunchKernelGGL(ms_shade_kernel, dim3((unsigned)cdiv(pixels, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, tri, faces, F, V, face_map, H,
                     W, normals, colors, a, rgb);
  return launch_status("mesh_shade");
}

extern "C" int svr_box_downsample_rgb8(const uint8_t *src, int32_t H, int32_t W, int32_t s, uint8_t *dst, void *stream) {
  SVR_CHECK(s >= 1 && s <= 4, SVR_E_BADARG, "box_downsample_rgb8: s=%d (need 1 <= s <= 4)", s);
  SVR_CHECK(image_ok(H, W) && (int64_t)H * s <= 32768 && (int64_t)W * s <= 32768, SVR_E_BADSHAPE,
            "box_downsample_rgb8: image %d x %d from %d x %d (need 1 <= H, W and s H, s W <= 32768)", H, W, H * s, W * s);
  SVR_CHECK(src && dst, SVR_E_BADARG, "box_downsample_rgb8: null pointer");
  const uintptr_t in = (uintptr_t)src, out = (uintptr_t)dst, nin = (uintptr_t)H * W * 3 * s * s, nout = (uintptr_t)H * W * 3;
  SVR_CHECK(out >= in + nin || in >= out + nout, SVR_E_BADARG, "box_downsample_rgb8: dst overlaps src");
  const int64_t pixels = (int64_t)H * W;
  hipLaunchKernelGGL(ms_downsample_kernel, dim3((unsigned)cdiv(pixels, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, src, H, W, s, dst);
  return launch_status("box_downsample_rgb8");
}
