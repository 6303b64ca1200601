// Unsigned distance field of a triangle mesh on a lattice, gfx950 (the input of process_sample: distance_field.df).
//
// The reference never shipped the tool that made its .df files; this is the project's own.  The rule -- Ericson's
// closest-point-on-triangle region test in float64, one rounding per operation, the lowest face index winning a tie --
// is written down line by line in include/svr_hip.h and restated in numpy by tests/df_oracle.py; the file is built with
// -ffp-contract=off.  Brute force at the real shape is 1.6 M points x 45 k faces, so the lattice is cut into bricks
// of s^3 points and every brick gets a candidate list:
//   * df_cull_count_kernel   one workgroup per brick, threads striding over the faces: dmin = min d(c, face) at the brick's
//                            centre, then the number of faces with d(c, face) <= min(dmin, T) + 2 r + slack;
//   * exclusive scan (rocPRIM) of the counts -> offsets the host reads back to batch the bricks;
//   * df_emit_kernel         the same test again, faces in ascending order, compacted by ballot + prefix;
//   * df_eval_kernel         one workgroup per brick, every lattice point owned by one thread (s = 8: 512 points on 256
//                            threads, two per thread; s = 4: 64 points on one wave), the candidates streaming through LDS in
//                            tiles of one triangle per thread, double-buffered, one barrier per tile; every lane reads the
//                            SAME triangle (broadcast) and updates its points.  No atomics, no cross-workgroup merge.
// The pair routine is the same function in all three, so the culling compares what the exact kernel computes.
#include "common.h"
#include <algorithm>
#include <cmath>
#include <limits>

using namespace svr;

namespace {

struct Bricks {
  int32_t X, Y, Z, s, nbx, nby, nbz;
  int64_t n;  // bricks
};

bool bricks(int32_t X, int32_t Y, int32_t Z, int32_t s, Bricks &B) {
  if (X < 1 || Y < 1 || Z < 1 || (s != 4 && s != 8)) return false;
  if ((int64_t)X * Y * Z >= (1LL << 31)) return false;
  B.X = X, B.Y = Y, B.Z = Z, B.s = s;
  B.nbx = (int32_t)cdiv(X, s), B.nby = (int32_t)cdiv(Y, s), B.nbz = (int32_t)cdiv(Z, s);
  B.n = (int64_t)B.nbx * B.nby * B.nbz;
  return true;
}

__device__ __forceinline__ double dot3(double ux, double uy, double uz, double vx, double vy, double vz) {
  return (ux * vx + uy * vy) + uz * vz;
}

// ab x ac == (0, 0, 0) exactly: the face is skipped
__device__ __forceinline__ bool tri_has_area(const double *t) {
  const double abx = t[3] - t[0], aby = t[4] - t[1], abz = t[5] - t[2];
  const double acx = t[6] - t[0], acy = t[7] - t[1], acz = t[8] - t[2];
  const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
  return !(nx == 0.0 && ny == 0.0 && nz == 0.0);
}

// the pair's squared distance: include/svr_hip.h, line by line
__device__ __forceinline__ double pair_dd(double px, double py, double pz, const double *t) {
  const double ax = t[0], ay = t[1], az = t[2], bx = t[3], by = t[4], bz = t[5], cx = t[6], cy = t[7], cz = t[8];
  const double abx = bx - ax, aby = by - ay, abz = bz - az;
  const double acx = cx - ax, acy = cy - ay, acz = cz - az;
  const double apx = px - ax, apy = py - ay, apz = pz - az;
  const double bpx = px - bx, bpy = py - by, bpz = pz - bz;
  const double cpx = px - cx, cpy = py - cy, cpz = pz - cz;
  const double d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
  const double d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
  const double d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
  double v, w;
  if (d1 <= 0.0 && d2 <= 0.0) {
    v = 0.0, w = 0.0;
  } else if (d3 >= 0.0 && d4 <= d3) {
    v = 1.0, w = 0.0;
  } else if (d1 * d4 - d3 * d2 <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    v = d1 / (d1 - d3), w = 0.0;
  } else if (d6 >= 0.0 && d5 <= d6) {
    v = 0.0, w = 1.0;
  } else if (d5 * d2 - d1 * d6 <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    v = 0.0, w = d2 / (d2 - d6);
  } else {
    const double va = d3 * d6 - d5 * d4, e43 = d4 - d3, e56 = d5 - d6;
    if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {
      w = e43 / (e43 + e56);
      v = 1.0 - w;
    } else {
      const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6;
      const double den = (va + vb) + vc;
      v = vb / den, w = vc / den;
    }
  }
  const double ex = px - ((ax + v * abx) + w * acx), ey = py - ((ay + v * aby) + w * acy), ez = pz - ((az + v * abz) + w * acz);
  return dot3(ex, ey, ez, ex, ey, ez);
}

struct BrickGeom {
  int32_t ox, oy, oz;  // first point
  double cx, cy, cz, r;
};

__device__ __forceinline__ BrickGeom brick_geom(const Bricks &B, int64_t b) {
  BrickGeom g;
  const int32_t bz = (int32_t)(b % B.nbz), by = (int32_t)((b / B.nbz) % B.nby), bx = (int32_t)(b / ((int64_t)B.nbz * B.nby));
  g.ox = bx * B.s, g.oy = by * B.s, g.oz = bz * B.s;
  const double ex = (double)(min(B.s, B.X - g.ox) - 1), ey = (double)(min(B.s, B.Y - g.oy) - 1), ez = (double)(min(B.s, B.Z - g.oz) - 1);
  g.cx = (double)g.ox + 0.5 * ex, g.cy = (double)g.oy + 0.5 * ey, g.cz = (double)g.oz + 0.5 * ez;  // exact
  g.r = 0.5 * sqrt((ex * ex + ey * ey) + ez * ez);
  return g;
}

constexpr int kCullThreads = 256;

__global__ __launch_bounds__(256) void df_valid_kernel(const double *__restrict__ tri, int64_t F, unsigned long long *__restrict__ n) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool ok = f < F && tri_has_area(tri + f * 9);
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n, (unsigned long long)__popcll(m));
}

// counts[b] = candidates of brick b, thr2[b] = the squared threshold; counts[B.n] = 0 closes the scan
__global__ __launch_bounds__(kCullThreads) void df_cull_count_kernel(const double *__restrict__ tri, int32_t F, Bricks B, double cap,
                                                                      double slack, unsigned long long *__restrict__ counts,
                                                                      double *__restrict__ thr2_out) {
  __shared__ double red[kCullThreads];
  __shared__ int cnt[kCullThreads / 64];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const BrickGeom g = brick_geom(B, b);
  double m = std::numeric_limits<double>::infinity();
  for (int32_t f = tid; f < F; f += kCullThreads) {
    const double *t = tri + (int64_t)f * 9;
    if (!tri_has_area(t)) continue;
    const double dd = pair_dd(g.cx, g.cy, g.cz, t);
    m = dd < m ? dd : m;
  }
  red[tid] = m;
  __syncthreads();
  for (int s = kCullThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid + s] < red[tid] ? red[tid + s] : red[tid];
    __syncthreads();
  }
  double base = sqrt(red[0]);
  if (cap > 0.0 && base > cap) base = cap;
  const double thr = (base + 2.0 * g.r) + slack;
  const double thr2 = (thr * thr) * (1.0 + 0x1p-50);  // the square rounded up: dd <= thr2 wherever sqrt(dd) <= thr
  int c = 0;
  for (int32_t f = tid; f < F; f += kCullThreads) {
    const double *t = tri + (int64_t)f * 9;
    if (!tri_has_area(t)) continue;
    c += pair_dd(g.cx, g.cy, g.cz, t) <= thr2;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((tid & 63) == 0) cnt[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int i = 0; i < kCullThreads / 64; ++i) total += cnt[i];
    counts[b] = (unsigned long long)total;
    thr2_out[b] = thr2;
    if (b == 0) counts[B.n] = 0;
  }
}

// the list of brick b0 + blockIdx.x: the faces that pass the count's test, ascending
__global__ __launch_bounds__(kCullThreads) void df_emit_kernel(const double *__restrict__ tri, int32_t F, Bricks B,
                                                                const double *__restrict__ thr2_in, const int64_t *__restrict__ offsets,
                                                                int64_t b0, int32_t *__restrict__ list, int64_t capacity) {
  __shared__ int wave_n[kCullThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = b0 + blockIdx.x;
  const BrickGeom g = brick_geom(B, b);
  const double thr2 = thr2_in[b];
  const int64_t start = offsets[b] - offsets[b0];
  // never past this brick's share nor past the buffer, whatever the test says
  const int64_t room = min(offsets[b + 1] - offsets[b], capacity - start);
  int64_t done = 0;
  for (int32_t f0 = 0; f0 < F; f0 += kCullThreads) {
    const int32_t f = f0 + tid;
    bool keep = false;
    if (f < F) {
      const double *t = tri + (int64_t)f * 9;
      keep = tri_has_area(t) && pair_dd(g.cx, g.cy, g.cz, t) <= thr2;
    }
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
// LDS tile: one triangle per thread, 10 doubles each: a, b, c and the face index (-1: skipped or past the list's end).
constexpr int kTriSlot = 10;

template <int S, int THREADS, int PPT>
__global__ __launch_bounds__(THREADS) void df_eval_kernel(const double *__restrict__ tri, int32_t F, Bricks B, float cap,
                                                          const int64_t *__restrict__ offsets, const int32_t *__restrict__ list,
                                                          int64_t b0, float *__restrict__ field, int32_t *__restrict__ face) {
  static_assert(THREADS * PPT == S * S * S, "every point of a brick has one owner");
  __shared__ double tile[2][THREADS * kTriSlot];
  const int tid = threadIdx.x;
  const int64_t b = b0 + blockIdx.x;
  const BrickGeom g = brick_geom(B, b);
  const int64_t lbase = list ? offsets[b] - offsets[b0] : 0;
  const int32_t n = list ? (int32_t)(offsets[b + 1] - offsets[b]) : F;
  double px[PPT], py[PPT], pz[PPT], best[PPT];
  int32_t bidx[PPT];
  bool inside[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int l = tid + k * THREADS;
    const int32_t i = g.ox + l / (S * S), j = g.oy + (l / S) % S, kk = g.oz + l % S;
    inside[k] = i < B.X && j < B.Y && kk < B.Z;
    px[k] = (double)i, py[k] = (double)j, pz[k] = (double)kk;
    best[k] = std::numeric_limits<double>::infinity();
    bidx[k] = -1;
  }
  const int ntiles = (n + THREADS - 1) / THREADS;
  double stage[kTriSlot];
  auto load = [&](int it) {
    const int32_t idx = it * THREADS + tid;
    stage[9] = -1.0;
    if (idx < n) {
      const int32_t f = list ? list[lbase + idx] : idx;
      const bool known = f >= 0 && f < F;  // a list this library did not write must not become an address
      const double *t = tri + (int64_t)(known ? f : 0) * 9;
#pragma unroll
      for (int e = 0; e < 9; ++e) stage[e] = t[e];
      if (known && tri_has_area(stage)) stage[9] = (double)f;
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
      double t[kTriSlot];
#pragma unroll
      for (int e = 0; e < kTriSlot; ++e) t[e] = cur[j * kTriSlot + e];  // every lane the same address: a broadcast read
      if (t[9] < 0.0) continue;
      const int32_t fj = (int32_t)t[9];
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        if (!inside[k]) continue;
        const double dd = pair_dd(px[k], py[k], pz[k], t);
        const bool better = dd < best[k];  // strict, ascending face order: the lowest index keeps a tie, NaN never wins
        best[k] = better ? dd : best[k];
        bidx[k] = better ? fj : bidx[k];
      }
    }
    if (it + 1 < ntiles) store((it + 1) & 1);
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    if (!inside[k]) continue;
    const int64_t o = ((int64_t)px[k] * B.Y + (int64_t)py[k]) * B.Z + (int64_t)pz[k];
    float v = (float)sqrt(best[k]);
    int32_t fi = bidx[k];
    if (cap > 0.0f && v > cap) v = cap, fi = -1;
    field[o] = v;
    if (face) face[o] = fi;
  }
}

struct Ws {
  unsigned long long *counts;  // bricks + 1
  double *thr2;                // bricks
  void *tmp;
  size_t tmp_bytes;
};

Ws ws_layout(WsCursor &c, int64_t nb) {   // the launchers have always used the caller's pointer as it is: base alignment 1
  const size_t tmp_bytes = scan_sum_excl_u64_temp_bytes(nb + 1);
  return {c.take<unsigned long long>(nb + 1), c.take<double>(nb), c.take<char>((int64_t)tmp_bytes), tmp_bytes};
}

}  // namespace

#define DF_BRICKS(name)                                                                                                      \
  Bricks B;                                                                                                                  \
  SVR_CHECK(bricks(X, Y, Z, s, B), SVR_E_BADSHAPE,                                                                           \
            name ": bad lattice %d x %d x %d, brick %d (extents >= 1, fewer than 2^31 points, brick 4 or 8)", X, Y, Z, s)

extern "C" int64_t svr_mesh_df_bricks(int32_t X, int32_t Y, int32_t Z, int32_t s) {
  DF_BRICKS("mesh_df_bricks");
  return B.n;
}

extern "C" int64_t svr_mesh_df_workspace_bytes(int32_t X, int32_t Y, int32_t Z, int32_t s) {
  DF_BRICKS("mesh_df_workspace_bytes");
  return ws_measure(ws_layout, B.n);
}

extern "C" int svr_mesh_df_valid_faces(const double *tri, int64_t F, void *ws, int64_t *n_valid, void *stream) {
  SVR_CHECK(F >= 0 && F < (1LL << 31), SVR_E_BADARG, "mesh_df_valid_faces: F=%ld", (long)F);
  SVR_CHECK(n_valid, SVR_E_BADARG, "mesh_df_valid_faces: null n_valid");
  *n_valid = 0;
  SVR_CHECK(F > 0, SVR_E_BADSHAPE, "mesh_df: the mesh has no face");
  SVR_CHECK(tri && ws, SVR_E_BADARG, "mesh_df_valid_faces: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(ws, 0, 8, st);
  SVR_CHECK(e == hipSuccess, (int)e, "mesh_df_valid_faces: memset failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(df_valid_kernel, dim3((unsigned)cdiv(F, 256)), dim3(256), 0, st, tri, F, (unsigned long long *)ws);
  if (int rc = launch_status("mesh_df_valid_faces")) return rc;
  e = hipMemcpyAsync(n_valid, ws, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  SVR_CHECK(e == hipSuccess, (int)e, "mesh_df_valid_faces: read back failed: %s", hipGetErrorString(e));
  SVR_CHECK(*n_valid > 0, SVR_E_BADSHAPE, "mesh_df: none of the %ld faces has an area", (long)F);
  return SVR_OK;
}

extern "C" int svr_mesh_df_count(const double *tri, int64_t F, int32_t X, int32_t Y, int32_t Z, int32_t s, double truncate,
                                 double slack, void *ws, int64_t ws_bytes, int64_t *offsets, void *stream) {
  DF_BRICKS("mesh_df_count");
  SVR_CHECK(F > 0 && F < (1LL << 31), SVR_E_BADSHAPE, "mesh_df_count: F=%ld (need 1 <= F < 2^31)", (long)F);
  SVR_CHECK(tri && ws && offsets, SVR_E_BADARG, "mesh_df_count: null pointer");
  SVR_CHECK(slack >= 0.0, SVR_E_BADARG, "mesh_df_count: slack=%g", slack);  // false for NaN too
  WsCursor c(ws, 1);
  const Ws w = ws_layout(c, B.n);
  SVR_CHECK(ws_bytes >= c.bytes(), SVR_E_BADARG, "mesh_df_count: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)c.bytes());
  hipStream_t st = (hipStream_t)stream;
  // the cap on dmin: (float)T is what the exact kernel compares with; a hair above it, so that rounding T never drops a face
  const double cap = truncate > 0.0 ? (double)(float)truncate * (1.0 + 0x1p-22) : 0.0;
  hipLaunchKernelGGL(df_cull_count_kernel, dim3((unsigned)B.n), dim3(kCullThreads), 0, st, tri, (int32_t)F, B, cap, slack, w.counts,
                     w.thr2);
  if (int rc = launch_status("mesh_df_cull_count")) return rc;
  hipError_t e = scan_sum_excl_u64(w.tmp, w.tmp_bytes, (const uint64_t *)w.counts, (uint64_t *)offsets, B.n + 1, st);
  SVR_CHECK(e == hipSuccess, (int)e, "mesh_df_count: scan failed: %s", hipGetErrorString(e));
  return launch_status("mesh_df_scan");
}

extern "C" int svr_mesh_df_emit(const double *tri, int64_t F, int32_t X, int32_t Y, int32_t Z, int32_t s, const void *ws,
                                const int64_t *offsets, int64_t b0, int64_t b1, int32_t *list, int64_t capacity, void *stream) {
  DF_BRICKS("mesh_df_emit");
  SVR_CHECK(F > 0 && F < (1LL << 31), SVR_E_BADSHAPE, "mesh_df_emit: F=%ld (need 1 <= F < 2^31)", (long)F);
  SVR_CHECK(0 <= b0 && b0 <= b1 && b1 <= B.n, SVR_E_BADARG, "mesh_df_emit: bricks [%ld, %ld) of %ld", (long)b0, (long)b1, (long)B.n);
  SVR_CHECK(capacity >= 0, SVR_E_BADARG, "mesh_df_emit: capacity=%ld", (long)capacity);
  if (b0 == b1 || capacity == 0) return SVR_OK;
  SVR_CHECK(tri && ws && offsets && list, SVR_E_BADARG, "mesh_df_emit: null pointer");
  WsCursor c(ws, 1);
  const Ws w = ws_layout(c, B.n);
  hipLaunchKernelGGL(df_emit_kernel, dim3((unsigned)(b1 - b0)), dim3(kCullThreads), 0, (hipStream_t)stream, tri, (int32_t)F, B, w.thr2,
                     offsets, b0, list, capacity);
  return launch_status("mesh_df_emit");
}

extern "C" int svr_mesh_df_eval(const double *tri, int64_t F, int32_t X, int32_t Y, int32_t Z, int32_t s, double truncate,
                                const int64_t *offsets, const int32_t *list, int64_t b0, int64_t b1, float *field, int32_t *face,
                                void *stream) {
  DF_BRICKS("mesh_df_eval");
  SVR_CHECK(F > 0 && F < (1LL << 31), SVR_E_BADSHAPE, "mesh_df_eval: F=%ld (need 1 <= F < 2^31)", (long)F);
  SVR_CHECK(0 <= b0 && b0 <= b1 && b1 <= B.n, SVR_E_BADARG, "mesh_df_eval: bricks [%ld, %ld) of %ld", (long)b0, (long)b1, (long)B.n);
  if (b0 == b1) return SVR_OK;
  SVR_CHECK(tri && field && (!list || offsets), SVR_E_BADARG, "mesh_df_eval: null pointer");
  const float cap = truncate > 0.0 ? (float)truncate : 0.0f;
  const dim3 grid((unsigned)(b1 - b0));
  hipStream_t st = (hipStream_t)stream;
  if (s == 8)
    hipLaunchKernelGGL((df_eval_kernel<8, 256, 2>), grid, dim3(256), 0, st, tri, (int32_t)F, B, cap, offsets, list, b0, field, face);
  else
    hipLaunchKernelGGL((df_eval_kernel<4, 64, 1>), grid, dim3(64), 0, st, tri, (int32_t)F, B, cap, offsets, list, b0, field, face);
  return launch_status("mesh_df_eval");
}
