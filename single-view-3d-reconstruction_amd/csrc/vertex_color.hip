// Vertex colours of a mesh from the image it was reconstructed from, gfx950 (the .ply writer that carries them: io_mesh.cpp).
//
// The rule is written down in include/svr_hip.h and restated in numpy by tests/vertex_color_oracle.py; the file is built
// with -ffp-contract=off, so every float64 operation below rounds once, as numpy's does.
//   * vc_sample_kernel      one thread per vertex: projection with raycast.hip's formula, the visibility test against the
//                           depth map of the same camera (up to four pixels), the image position through the caller's
//                           affine pixel map, clamp-to-edge bilinear fetch.  Plain loads and stores, no shared state.
//   * vc_accumulate_kernel  one thread per face: for every corner still without a colour, the colours of the face's coloured
//                           corners into the corner's {r, g, b, count} row of the workspace, with integer atomics;
//   * vc_finalise_kernel    one thread per vertex: a row with count > 0 becomes the rounded mean and state 2, the row goes
//                           back to zero (no memset per pass) and the block adds how many vertices it changed to a counter.
// `state` is read by the accumulate launch only and written by the finalise launch only, so a pass sees the states of its
// start and stream order is the only barrier.  The sums are uint32: whichever way the atomics arrive, the bits are the same.
#include "common.h"
#include "reduce.h"
#include <cmath>

using namespace svr;

namespace {

constexpr int kBlock = 256;

// the constants of svr_unproject_fwd that the projection uses, widened (raycast.hip's Camera)
struct Camera {
  double f, cx, cy, s00, t0, s11, t1, s22, t2;
};

Camera camera(const float *k) {
  return Camera{(double)k[0], (double)k[1], (double)k[2], (double)k[3], (double)k[4], (double)k[5], (double)k[6], (double)k[7], (double)k[8]};
}

struct PixelMap {
  double ax, bx, ay, by;
};

struct Fill {
  uint8_t c[3];
};

__device__ __forceinline__ int32_t clampi(int32_t v, int32_t lo, int32_t hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(kBlock) void vc_sample_kernel(const float *__restrict__ verts, int64_t V, Camera c,
                                                           const float *__restrict__ depth, int32_t H, int32_t W, double bias,
                                                           const uint8_t *__restrict__ image, int32_t Hi, int32_t Wi, PixelMap m, Fill fill,
                                                           uint8_t *__restrict__ colors, uint8_t *__restrict__ state) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= V) return;
  const double g0 = (double)verts[i * 3 + 0], g1 = (double)verts[i * 3 + 1], g2 = (double)verts[i * 3 + 2];
  const double zc = (g2 - c.t2) / c.s22;
  const double u = c.cx + (c.f * (g0 - c.t0)) / (c.s00 * zc);
  const double v = c.cy - (c.f * (g1 - c.t1)) / (c.s11 * zc);
  uint8_t out[3] = {fill.c[0], fill.c[1], fill.c[2]};
  uint8_t st = 0;
  // every comparison is false for NaN: a vertex that projects to NaN is not in the frame
  if (zc > 0.0 && u >= -0.5 && u <= (double)W - 0.5 && v >= -0.5 && v <= (double)H - 0.5) {
    const int32_t iu = (int32_t)floor(u), iv = (int32_t)floor(v);  // in [-1, W - 1] x [-1, H - 1]
    bool seen = false;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int32_t pc = iu + a, pr = iv + b;
        if (pc >= 0 && pc < W && pr >= 0 && pr < H) {
          const float D = depth[(int64_t)pr * W + pc];
          seen = seen || (D > 0.f && zc <= (double)D + bias);
        }
      }
    const double x = m.ax * u + m.bx, y = m.ay * v + m.by;
    if (seen && x >= -0.5 && x <= (double)Wi - 0.5 && y >= -0.5 && y <= (double)Hi - 0.5) {
      const double x0 = floor(x), y0 = floor(y);
      const double wx = x - x0, wy = y - y0;
      const int32_t ix = (int32_t)x0, iy = (int32_t)y0;  // in [-1, Wi - 1] x [-1, Hi - 1]
      const int32_t c0 = clampi(ix, 0, Wi - 1), c1 = clampi(ix + 1, 0, Wi - 1);
      const int32_t r0 = clampi(iy, 0, Hi - 1), r1 = clampi(iy + 1, 0, Hi - 1);
      const uint8_t *q00 = image + ((int64_t)r0 * Wi + c0) * 3, *q10 = image + ((int64_t)r0 * Wi + c1) * 3;
      const uint8_t *q01 = image + ((int64_t)r1 * Wi + c0) * 3, *q11 = image + ((int64_t)r1 * Wi + c1) * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const double p00 = (double)q00[ch], p10 = (double)q10[ch], p01 = (double)q01[ch], p11 = (double)q11[ch];
        const double top = p00 + wx * (p10 - p00);
        const double bot = p01 + wx * (p11 - p01);
        const double val = top + wy * (bot - top);  // between the four values: rounding is monotone
        out[ch] = (uint8_t)(int32_t)rint(val);
      }
      st = 1;
    }
  }
  colors[i * 3 + 0] = out[0];
  colors[i * 3 + 1] = out[1];
  colors[i * 3 + 2] = out[2];
  state[i] = st;
}

// acc: (V, 4) uint32 {r, g, b, count}.  Per corner d without a colour the face's coloured corners are summed in registers
// first: the corner's six ordered pairs cost it four atomics, not eight.
__global__ __launch_bounds__(kBlock) void vc_accumulate_kernel(const int32_t *__restrict__ faces, int64_t F, int64_t V,
                                                               const uint8_t *__restrict__ colors, const uint8_t *__restrict__ state,
                                                               uint32_t *__restrict__ acc) {
  const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  int32_t idx[3];
  bool known = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    idx[k] = faces[f * 3 + k];
    known = known && idx[k] >= 0 && (int64_t)idx[k] < V;
  }
  if (!known) return;  // an index that is no vertex must not become an address
  bool has[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) has[k] = state[idx[k]] != 0;
  if (has[0] == has[1] && has[1] == has[2]) return;  // nothing to hand over inside this face
  uint32_t col[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) col[k][ch] = has[k] ? (uint32_t)colors[(int64_t)idx[k] * 3 + ch] : 0u;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (has[d]) continue;
    const int a = (d + 1) % 3, b = (d + 2) % 3;
    uint32_t *row = acc + (int64_t)idx[d] * 4;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const uint32_t s = col[a][ch] + col[b][ch];
      if (s) atomicAdd(row + ch, s);
    }
    atomicAdd(row + 3, (uint32_t)has[a] + (uint32_t)has[b]);
  }
}

__global__ __launch_bounds__(kBlock) void vc_finalise_kernel(int64_t V, uint32_t *__restrict__ acc, uint8_t *__restrict__ colors,
                                                             uint8_t *__restrict__ state, unsigned long long *__restrict__ changed) {
  __shared__ uint64_t part[2][kBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  uint64_t mine = 0;
  if (i < V) {
    uint4 *row = reinterpret_cast<uint4 *>(acc) + i;
    const uint4 r = *row;
    if (r.w > 0) {
      const uint32_t two = 2u * r.w;
      colors[i * 3 + 0] = (uint8_t)((2u * r.x + r.w) / two);
      colors[i * 3 + 1] = (uint8_t)((2u * r.y + r.w) / two);
      colors[i * 3 + 2] = (uint8_t)((2u * r.z + r.w) / two);
      state[i] = 2;
      *row = make_uint4(0u, 0u, 0u, 0u);
      mine = 1;
    }
  }
  block_add_totals_u64<kBlock>(mine, 0, part, changed);  // every thread of the block arrives here
}

struct Ws { uint32_t *acc; unsigned long long *changed; };   // V rows of four words; two words: block_add_totals_u64's pair
Ws ws_layout(WsCursor &c, int64_t V) { return {c.take<uint32_t>(4 * V), c.take<unsigned long long>(2)}; }

}  // namespace

extern "C" int64_t svr_vertex_color_workspace_bytes(int64_t V) {
  SVR_CHECK(V >= 0 && V < (1LL << 31), SVR_E_BADSHAPE, "vertex_color_workspace_bytes: V=%ld (need 0 <= V < 2^31)", (long)V);
  return ws_measure(ws_layout, V);
}

extern "C" int svr_vertex_color_sample(const float *verts, int64_t V, const float *consts, const float *depth, int32_t H, int32_t W,
                                       double bias, const uint8_t *image, int32_t Hi, int32_t Wi, const double *map,
                                       const uint8_t *fill, uint8_t *colors, uint8_t *state, void *stream) {
  SVR_CHECK(V >= 0 && V < (1LL << 31), SVR_E_BADSHAPE, "vertex_color_sample: V=%ld (need 0 <= V < 2^31)", (long)V);
  SVR_CHECK(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, SVR_E_BADSHAPE, "vertex_color_sample: bad depth map %d x %d (1 <= H, W <= 32768)", H, W);
  SVR_CHECK(Hi >= 1 && Wi >= 1 && Hi <= 32768 && Wi <= 32768, SVR_E_BADSHAPE, "vertex_color_sample: bad image %d x %d (1 <= Hi, Wi <= 32768)", Hi,
            Wi);
  SVR_CHECK(consts && map && fill, SVR_E_BADARG, "vertex_color_sample: null pointer");
  if (V == 0) return SVR_OK;
  SVR_CHECK(verts && depth && image && colors && state, SVR_E_BADARG, "vertex_color_sample: null pointer");
  const PixelMap m{map[0], map[1], map[2], map[3]};
  const Fill fl{{fill[0], fill[1], fill[2]}};
  hipLaunchKernelGGL(vc_sample_kernel, dim3((unsigned)cdiv(V, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, verts, V, camera(consts), depth,
                     H, W, bias, image, Hi, Wi, m, fl, colors, state);
  return launch_status("vertex_color_sample");
}

extern "C" int svr_vertex_color_spread(const int32_t *faces, int64_t F, int64_t V, uint8_t *colors, uint8_t *state, void *ws,
                                       int64_t ws_bytes, int64_t max_passes, int32_t check_every, int64_t *passes, void *stream) {
  SVR_CHECK(V >= 0 && V < (1LL << 31), SVR_E_BADSHAPE, "vertex_color_spread: V=%ld (need 0 <= V < 2^31)", (long)V);
  SVR_CHECK(F >= 0 && F < (1LL << 31), SVR_E_BADSHAPE, "vertex_color_spread: F=%ld (need 0 <= F < 2^31)", (long)F);
  SVR_CHECK(check_every >= 1, SVR_E_BADARG, "vertex_color_spread: check_every=%d (need >= 1)", check_every);
  if (passes) *passes = 0;
  if (V == 0 || F == 0 || max_passes == 0) return SVR_OK;
  SVR_CHECK(faces && colors && state && ws, SVR_E_BADARG, "vertex_color_spread: null pointer");
  WsCursor c(ws);
  const Ws w = ws_layout(c, V);
  SVR_CHECK(ws_bytes >= c.bytes(), SVR_E_BADARG, "vertex_color_spread: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)c.bytes());
  hipStream_t st = (hipStream_t)stream;
  // both pieces, once per call; the passes keep them zero
  hipError_t e = hipMemsetAsync(w.acc, 0, (size_t)(c.bytes() - WsCursor::kSlack), st);
  SVR_CHECK(e == hipSuccess, (int)e, "vertex_color_spread: memset failed: %s", hipGetErrorString(e));
  // a pass that changes anything colours a vertex, so the fixed point comes within V passes; one more shows it
  const int64_t limit = max_passes < 0 || max_passes > V + 1 ? V + 1 : max_passes;
  unsigned long long seen = 0;
  int64_t done = 0;
  while (done < limit) {
    const int64_t n = limit - done < check_every ? limit - done : check_every;
    for (int64_t p = 0; p < n; ++p) {
      hipLaunchKernelGGL(vc_accumulate_kernel, dim3((unsigned)cdiv(F, kBlock)), dim3(kBlock), 0, st, faces, F, V, colors, state, w.acc);
      hipLaunchKernelGGL(vc_finalise_kernel, dim3((unsigned)cdiv(V, kBlock)), dim3(kBlock), 0, st, V, w.acc, colors, state, w.changed);
    }
    if (int rc = launch_status("vertex_color_spread")) return rc;
    done += n;
    if (done >= limit) break;  // nothing left to decide
    unsigned long long now = 0;
    e = hipMemcpyAsync(&now, w.changed, sizeof(now), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    SVR_CHECK(e == hipSuccess, (int)e, "vertex_color_spread: reading the counter failed: %s", hipGetErrorString(e));
    if (now == seen) break;  // none of the last n passes changed a vertex: neither will any later one
    seen = now;
  }
  if (passes) *passes = done;
  return SVR_OK;
}
