// Depth, distance, face and normal maps of a triangle mesh seen through the pipeline's pinhole camera, gfx950 (the
// distance.exr of a raw view, which the reference rendered with a tool it never shipped; data_processing/render_view.py).
//
// The rule -- Moeller-Trumbore in float64, one rounding per operation, the lowest face index winning a tie -- is written
// down in include/svr_hip.h and restated in numpy by tests/raycast_oracle.py; the file is built with -ffp-contract=off.
// Brute force at the real shape is 76 800 rays x 45 k faces, so the image is cut into tiles of T x T pixels and every
// tile gets a candidate list, the structure of mesh_df.hip with screen tiles in place of bricks:
//   * rc_face_bounds_kernel  one thread per face: the three vertices projected, the pixel rectangle of the projection
//                            widened by one pixel; a face with a vertex not in front of the camera covers every tile;
//   * rc_count_kernel        one workgroup per tile, threads striding over the faces: rectangles that overlap the tile;
//   * exclusive scan (rocPRIM) of the counts -> offsets the host reads back to batch the tiles;
//   * rc_emit_kernel         the same test again, faces in ascending order, compacted by ballot + prefix;
//   * rc_eval_kernel         one workgroup per tile, one thread per pixel, the candidates streaming through LDS in tiles of
//                            one triangle per thread, double-buffered, one barrier per tile; every lane reads the SAME
//                            triangle (broadcast) and tests its own ray.  No atomics, no cross-workgroup merge.
// The pair routine is raycast_pair.h's ray_triangle, the function the host check compiles too.
#include "common.h"
#include "raycast_pair.h"
#include <cmath>
#include <limits>

using namespace svr;

namespace {

struct Tiles {
  int32_t H, W, T, ntx, nty;
  int64_t n;  // tiles
};

bool tiles(int32_t H, int32_t W, int32_t T, Tiles &S) {
  if (H < 1 || W < 1 || H > 32768 || W > 32768 || (T != 8 && T != 16)) return false;
  S.H = H, S.W = W, S.T = T;
  S.ntx = (int32_t)cdiv(W, T), S.nty = (int32_t)cdiv(H, T);
  S.n = (int64_t)S.ntx * S.nty;
  return true;
}

// the 12 float32 constants of svr_unproject_fwd, widened
struct Camera {
  double f, cx, cy, s00, t0, s11, t1, s22, t2;
};

Camera camera(const float *k) {
  return Camera{(double)k[0], (double)k[1], (double)k[2], (double)k[3], (double)k[4], (double)k[5], (double)k[6], (double)k[7], (double)k[8]};
}

constexpr int kCullThreads = 256;
constexpr int32_t kRectMax = 1 << 30;      // |pixel coordinate| of a rectangle's side: far outside any image, exact in int32
constexpr double kMinDepth = 0x1p-20;      // a vertex nearer to the camera plane than this (metres) gives up the projection ...
constexpr double kMaxDepthRatio = 1024.0;  // ... and so does a face whose farthest vertex is this many times deeper than its nearest

// face -> {x0, x1, y0, y1}, the pixel rectangle (inclusive) that holds every pixel whose ray can hit it
__global__ __launch_bounds__(256) void rc_face_bounds_kernel(const double *__restrict__ tri, int64_t F, Camera c, int32_t *__restrict__ rects) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const double *t = tri + f * 9;
  const double inf = std::numeric_limits<double>::infinity();
  double umin = inf, umax = -inf, vmin = inf, vmax = -inf, zmin = inf, zmax = -inf;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double zc = (t[3 * k + 2] - c.t2) / c.s22;
    const double u = c.cx + (c.f * (t[3 * k + 0] - c.t0)) / (c.s00 * zc);
    const double v = c.cy - (c.f * (t[3 * k + 1] - c.t1)) / (c.s11 * zc);
    ok = ok && zc > kMinDepth && fabs(u) <= (double)kRectMax && fabs(v) <= (double)kRectMax;  // false for NaN and inf
    umin = fmin(umin, u), umax = fmax(umax, u), vmin = fmin(vmin, v), vmax = fmax(vmax, v);
    zmin = fmin(zmin, zc), zmax = fmax(zmax, zc);
  }
  ok = ok && zmax <= kMaxDepthRatio * zmin;
  int32_t r[4] = {-kRectMax, kRectMax, -kRectMax, kRectMax};
  if (ok) {
    const double lim = (double)kRectMax;
    r[0] = (int32_t)fmax(fmin(floor(umin) - 1.0, lim), -lim);
    r[1] = (int32_t)fmax(fmin(ceil(umax) + 1.0, lim), -lim);
    r[2] = (int32_t)fmax(fmin(floor(vmin) - 1.0, lim), -lim);
    r[3] = (int32_t)fmax(fmin(ceil(vmax) + 1.0, lim), -lim);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) rects[f * 4 + e] = r[e];
}

struct TileBox {
  int32_t x0, x1, y0, y1;  // the pixels the tile holds, inclusive
};

__device__ __forceinline__ TileBox tile_box(const Tiles &S, int64_t t) {
  TileBox b;
  b.x0 = (int32_t)(t % S.ntx) * S.T, b.y0 = (int32_t)(t / S.ntx) * S.T;
  b.x1 = min(b.x0 + S.T, S.W) - 1, b.y1 = min(b.y0 + S.T, S.H) - 1;
  return b;
}

__device__ __forceinline__ bool overlaps(const int32_t *__restrict__ rects, int32_t f, const TileBox &b) {
  const int4 r = *reinterpret_cast<const int4 *>(rects + (int64_t)f * 4);
  return r.x <= b.x1 && r.y >= b.x0 && r.z <= b.y1 && r.w >= b.y0;
}

// counts[t] = candidates of tile t; counts[S.n] = 0 closes the scan
__global__ __launch_bounds__(kCullThreads) void rc_count_kernel(const int32_t *__restrict__ rects, int32_t F, Tiles S,
                                                                 unsigned long long *__restrict__ counts) {
  __shared__ int cnt[kCullThreads / 64];
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  const TileBox b = tile_box(S, t);
  int c = 0;
  for (int32_t f = tid; f < F; f += kCullThreads) c += overlaps(rects, f, b);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((tid & 63) == 0) cnt[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int i = 0; i < kCullThreads / 64; ++i) total += cnt[i];
    counts[t] = (unsigned long long)total;
    if (t == 0) counts[S.n] = 0;
  }
}

// the list of tile b0 + blockIdx.x: the faces that pass the count's test, ascending
__global__ __launch_bounds__(kCullThreads) void rc_emit_kernel(const int32_t *__restrict__ rects, int32_t F, Tiles S,
                                                                const int64_t *__restrict__ offsets, int64_t b0, int32_t *__restrict__ list,
                                                                int64_t capacity) {
  __shared__ int wave_n[kCullThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t t = b0 + blockIdx.x;
  const TileBox b = tile_box(S, t);
  const int64_t start = offsets[t] - offsets[b0];
  // never past this tile's share nor past the buffer, whatever the test says
  const int64_t room = min(offsets[t + 1] - offsets[t], capacity - start);
  int64_t done = 0;
  for (int32_t f0 = 0; f0 < F; f0 += kCullThreads) {
    const int32_t f = f0 + tid;
    const bool keep = f < F && overlaps(rects, f, b);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wave_n[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < kCullThreads / 64; ++i) {
      before += i < wave ? wave_n[i] : 0;
      total += wave_n[i];
    }
    const int64_t pos = done + before + __popcll(mask & ((1ull << lane) - 1ull));
    if (keep && pos < room) list[start + pos] = f;
    done += total;
    __syncthreads();
  }
}

// ---- the exact kernel ----------------------------------------------------------------------------------------------
// LDS tile: one triangle per thread, 10 doubles each: a, b, c and the face index (-1: past the list's end or not a face).
constexpr int kTriSlot = 10;

struct Maps {
  float *depth;       // (H, W)
  int32_t *face;      // (H, W), optional
  float *distance;    // (H, W), optional
  float *normal;      // (H, W, 3), optional
  uint8_t *shade;     // (H, W), optional
};

template <int T>
__global__ __launch_bounds__(T * T) void rc_eval_kernel(const double *__restrict__ tri, int32_t F, Tiles S, Camera c, float focal, double near,
                                                        double far, float miss, const int64_t *__restrict__ offsets,
                                                        const int32_t *__restrict__ list, int64_t b0, Maps out) {
  constexpr int THREADS = T * T;
  __shared__ double tile[2][THREADS * kTriSlot];
  const int tid = threadIdx.x;
  const int64_t t = b0 + blockIdx.x;
  const int32_t col = (int32_t)(t % S.ntx) * T + tid % T, row = (int32_t)(t / S.ntx) * T + tid / T;
  const bool inside = col < S.W && row < S.H;
  const int64_t lbase = list ? offsets[t] - offsets[b0] : 0;
  const int32_t n = list ? (int32_t)(offsets[t + 1] - offsets[t]) : F;
  const double o[3] = {c.t0, c.t1, c.t2};
  double d[3];
  ray_direction(col, row, c.f, c.cx, c.cy, c.s00, c.s11, c.s22, d);
  double best = std::numeric_limits<double>::infinity();
  int32_t bidx = -1;
  const int ntiles = (n + THREADS - 1) / THREADS;
  double stage[kTriSlot];
  auto load = [&](int it) {
    const int32_t idx = it * THREADS + tid;
    stage[9] = -1.0;
    if (idx < n) {
      const int32_t f = list ? list[lbase + idx] : idx;
      const bool known = f >= 0 && f < F;  // a list this library did not write must not become an address
      const double *p = tri + (int64_t)(known ? f : 0) * 9;
#pragma unroll
      for (int e = 0; e < 9; ++e) stage[e] = p[e];
      if (known) stage[9] = (double)f;
    } else {
#pragma unroll
      for (int e = 0; e < 9; ++e) stage[e] = 0.0;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int e = 0; e < kTriSlot; ++e) tile[buf][tid * kTriSlot + e] = stage[e];
  };
  if (ntiles > 0) {
    load(0);
    store(0);
  }
  __syncthreads();
  for (int it = 0; it < ntiles; ++it) {
    if (it + 1 < ntiles) load(it + 1);
    const double *cur = tile[it & 1];
    const int nvalid = min(THREADS, n - it * THREADS);
    for (int j = 0; j < nvalid; ++j) {
      double a[kTriSlot];
#pragma unroll
      for (int e = 0; e < kTriSlot; ++e) a[e] = cur[j * kTriSlot + e];  // every lane the same address: a broadcast read
      if (a[9] < 0.0) continue;
      double z;
      if (inside && ray_triangle(o, d, a, near, far, &z) && z < best) {  // strict, ascending face order: the lowest index keeps a tie
        best = z;
        bidx = (int32_t)a[9];
      }
    }
    if (it + 1 < ntiles) store((it + 1) & 1);
    __syncthreads();
  }
  if (!inside) return;
  const int64_t px = (int64_t)row * S.W + col;
  const float depth = bidx >= 0 ? (float)best : miss;
  out.depth[px] = depth;
  if (out.face) out.face[px] = bidx;
  if (out.distance) {
    const int r = row - S.H / 2, cc = col - S.W / 2;
    const float rc = (float)(r * r + cc * cc);
    out.distance[px] = depth * sqrtf(rc / (focal * focal) + 1.f);
  }
  if (out.normal || out.shade) {
    double m[3] = {0.0, 0.0, 0.0};
    if (bidx >= 0) ray_facing_normal(d, tri + (int64_t)bidx * 9, m);
    if (out.normal) {
      out.normal[px * 3 + 0] = (float)m[0];
      out.normal[px * 3 + 1] = (float)m[1];
      out.normal[px * 3 + 2] = (float)m[2];
    }
    if (out.shade) {
      // round(255 |m . d| / |d|), half to even; NaN (a winner without area) and a miss give 0
      const double g = rint((255.0 * fabs(ray_dot3(m[0], m[1], m[2], d[0], d[1], d[2]))) / sqrt(ray_dot3(d[0], d[1], d[2], d[0], d[1], d[2])));
      out.shade[px] = g >= 0.0 && g <= 255.0 ? (uint8_t)g : (uint8_t)(g > 255.0 ? 255 : 0);
    }
  }
}

struct Ws { unsigned long long *counts; char *tmp; size_t tmp_bytes; };   // counts: tiles + 1
Ws ws_layout(WsCursor &c, int64_t n) {
  const size_t tmp_bytes = scan_sum_excl_u64_temp_bytes(n + 1);
  return {c.take<unsigned long long>(n + 1), c.take<char>((int64_t)tmp_bytes), tmp_bytes};
}
}  // namespace

#define RC_TILES(name)                                                                                                  \
  Tiles S;                                                                                                              \
  SVR_CHECK(tiles(H, W, T, S), SVR_E_BADSHAPE, name ": bad image %d x %d, tile %d (1 <= H, W <= 32768, tile 8 or 16)", H, W, T)

extern "C" int64_t svr_raycast_tiles(int32_t H, int32_t W, int32_t T) {
  RC_TILES("raycast_tiles");
  return S.n;
}

extern "C" int64_t svr_raycast_workspace_bytes(int32_t H, int32_t W, int32_t T) {
  RC_TILES("raycast_workspace_bytes");
  return ws_measure(ws_layout, S.n);
}

extern "C" int svr_raycast_face_bounds(const double *tri, int64_t F, const float *consts, int32_t *rects, void *stream) {
  SVR_CHECK(F > 0 && F < (1LL << 31), SVR_E_BADSHAPE, "raycast_face_bounds: F=%ld (need 1 <= F < 2^31)", (long)F);
  SVR_CHECK(tri && consts && rects, SVR_E_BADARG, "raycast_face_bounds: null pointer");
  hipLaunchKernelGGL(rc_face_bounds_kernel, dim3((unsigned)cdiv(F, 256)), dim3(256), 0, (hipStream_t)stream, tri, F, camera(consts), rects);
  return launch_status("raycast_face_bounds");
}

extern "C" int svr_raycast_count(const int32_t *rects, int64_t F, int32_t H, int32_t W, int32_t T, void *ws, int64_t ws_bytes,
                                 int64_t *offsets, void *stream) {
  RC_TILES("raycast_count");
  SVR_CHECK(F > 0 && F < (1LL << 31), SVR_E_BADSHAPE, "raycast_count: F=%ld (need 1 <= F < 2^31)", (long)F);
  SVR_CHECK(rects && ws && offsets, SVR_E_BADARG, "raycast_count: null pointer");
  WsCursor c(ws);
  const Ws w = ws_layout(c, S.n);
  SVR_CHECK(ws_bytes >= c.bytes(), SVR_E_BADARG, "raycast_count: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)c.bytes());
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rc_count_kernel, dim3((unsigned)S.n), dim3(kCullThreads), 0, st, rects, (int32_t)F, S, w.counts);
  if (int rc = launch_status("raycast_count")) return rc;
  hipError_t e = scan_sum_excl_u64(w.tmp, w.tmp_bytes, (const uint64_t *)w.counts, (uint64_t *)offsets, S.n + 1, st);
  SVR_CHECK(e == hipSuccess, (int)e, "raycast_count: scan failed: %s", hipGetErrorString(e));
  return launch_status("raycast_scan");
}

extern "C" int svr_raycast_emit(const int32_t *rects, int64_t F, int32_t H, int32_t W, int32_t T, const int64_t *offsets, int64_t b0,
                                int64_t b1, int32_t *list, int64_t capacity, void *stream) {
  RC_TILES("raycast_emit");
  SVR_CHECK(F > 0 && F < (1LL << 31), SVR_E_BADSHAPE, "raycast_emit: F=%ld (need 1 <= F < 2^31)", (long)F);
  SVR_CHECK(0 <= b0 && b0 <= b1 && b1 <= S.n, SVR_E_BADARG, "raycast_emit: tiles [%ld, %ld) of %ld", (long)b0, (long)b1, (long)S.n);
  SVR_CHECK(capacity >= 0, SVR_E_BADARG, "raycast_emit: capacity=%ld", (long)capacity);
  if (b0 == b1 || capacity == 0) return SVR_OK;
  SVR_CHECK(rects && offsets && list, SVR_E_BADARG, "raycast_emit: null pointer");
  hipLaunchKernelGGL(rc_emit_kernel, dim3((unsigned)(b1 - b0)), dim3(kCullThreads), 0, (hipStream_t)stream, rects, (int32_t)F, S, offsets,
                     b0, list, capacity);
  return launch_status("raycast_emit");
}

extern "C" int svr_raycast_eval(const double *tri, int64_t F, const float *consts, int32_t H, int32_t W, int32_t T, double near_z,
                                double far_z, float miss, const int64_t *offsets, const int32_t *list, int64_t b0, int64_t b1,
                                float *depth, int32_t *face, float *distance, float *normal, uint8_t *shade, void *stream) {
  RC_TILES("raycast_eval");
  SVR_CHECK(F > 0 && F < (1LL << 31), SVR_E_BADSHAPE, "raycast_eval: F=%ld (need 1 <= F < 2^31)", (long)F);
  SVR_CHECK(0 <= b0 && b0 <= b1 && b1 <= S.n, SVR_E_BADARG, "raycast_eval: tiles [%ld, %ld) of %ld", (long)b0, (long)b1, (long)S.n);
  if (b0 == b1) return SVR_OK;
  SVR_CHECK(tri && consts && depth && (!list || offsets), SVR_E_BADARG, "raycast_eval: null pointer");
  const dim3 grid((unsigned)(b1 - b0));
  hipStream_t st = (hipStream_t)stream;
  const Maps out{depth, face, distance, normal, shade};
  const Camera c = camera(consts);
  if (T == 8)
    hipLaunchKernelGGL((rc_eval_kernel<8>), grid, dim3(64), 0, st, tri, (int32_t)F, S, c, consts[0], near_z, far_z, miss, offsets, list, b0, out);
  else
    hipLaunchKernelGGL((rc_eval_kernel<16>), grid, dim3(256), 0, st, tri, (int32_t)F, S, c, consts[0], near_z, far_z, miss, offsets, list, b0,
                       out);
  return launch_status("raycast_eval");
}
