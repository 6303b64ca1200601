// On-device mesh evaluation (IoU / Chamfer-L2 / normal consistency), gfx950.
//
// Replaces what the reference's util/evaluate.py:9-119 takes from trimesh (mesh.sample, face_normals) and pykdtree
// (KDTree.query), and the surface sampler of data_processing/mesh_occupancies.py:9-22:
//   * svr_mesh_face_table   host C++: unit normals and the sequential running sum of the face areas (float64);
//   * svr_mesh_sample       one thread per sample: binary search in the running sum, reflected barycentric weights;
//   * svr_nn_search         exact all-pairs nearest neighbour with indices, targets staged through LDS;
//   * svr_nn_normals_dot, svr_eval_sums, svr_iou_counts   the epilogue and the reductions of the metrics.
// Every arithmetic rule is written down in include/svr_hip.h and restated in numpy by tests/eval_oracle.py; the file is
// built with -ffp-contract=off so that each operation rounds once, as numpy's does.
#include "common.h"
#include <algorithm>
#include <cmath>

using namespace svr;

namespace {

// ---- surface sampler -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mesh_sample_kernel(const double *__restrict__ tri, const double *__restrict__ cum,
                                                          int64_t n_faces, const double *__restrict__ uni, int64_t n,
                                                          float *__restrict__ points, int32_t *__restrict__ face) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double total = cum[n_faces - 1];
  const double x = uni[i * 3] * total;
  int64_t lo = 0, hi = n_faces;  // first j with cum[j] > x
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (cum[mid] > x) hi = mid;
    else lo = mid + 1;
  }
  if (lo >= n_faces) {  // x rounded up to the total: the first j with cum[j] >= total (the last face with an area)
    lo = 0, hi = n_faces;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (cum[mid] >= total) hi = mid;
      else lo = mid + 1;
    }
    if (lo >= n_faces) lo = n_faces - 1;  // NaN areas: stay in bounds
  }
  double u = uni[i * 3 + 1], v = uni[i * 3 + 2];
  if (u + v > 1.0) {
    u = 1.0 - u;
    v = 1.0 - v;
  }
  const double *t = tri + lo * 9;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double A = t[a], B = t[3 + a], Cc = t[6 + a];
    points[i * 3 + a] = (float)((A + u * (B - A)) + v * (Cc - A));
  }
  face[i] = (int32_t)lo;
}

// ---- exact nearest neighbour -----------------------------------------------------------------------------------
// Workgroup (bx, by): queries [1024 bx, 1024 bx + 1024), four per thread in registers (q = base + tid + 256 k, so the
// loads coalesce), against the target chunk `by`.  The chunk streams through LDS in tiles of 1024 targets stored as
// float4 (w unused), double-buffered: the next tile's 12 dwords per thread are in flight while the current one is
// consumed, one barrier per tile.  In the inner loop every lane reads the SAME float4 (broadcast, no bank conflict) and
// updates its four queries: 8 unfused f32 operations, one unsigned compare and two selects per pair.
// d2 >= +0 always (a sum of squares), so its bit pattern orders like its value; NaN patterns sort above +inf.  The
// compare is therefore done on the bits, strict, in ascending target order: the lowest index wins a tie and a NaN
// never beats a number.  Chunks merge through a 64-bit unsigned atomic min on (bits << 32 | index): order-independent.
constexpr int kNnThreads = 256, kNnQpt = 4, kNnTile = 1024, kNnQBlock = kNnThreads * kNnQpt;
constexpr int kNnStage = kNnTile * 3 / kNnThreads;  // dwords of a tile each thread moves

__global__ __launch_bounds__(kNnThreads) void nn_search_kernel(const float *__restrict__ queries, int64_t Q,
                                                               const float *__restrict__ targets, int32_t T, int32_t chunk,
                                                               unsigned long long *__restrict__ keys) {
  __shared__ float4 tile[2][kNnTile];
  const int tid = threadIdx.x;
  const int64_t qbase = (int64_t)blockIdx.x * kNnQBlock + tid;
  float qx[kNnQpt], qy[kNnQpt], qz[kNnQpt];
  uint32_t best[kNnQpt];
  int32_t bidx[kNnQpt];
#pragma unroll
  for (int k = 0; k < kNnQpt; ++k) {
    int64_t q = qbase + (int64_t)k * kNnThreads;
    if (q >= Q) q = Q - 1;  // a valid address; the result is not written
    qx[k] = queries[q * 3], qy[k] = queries[q * 3 + 1], qz[k] = queries[q * 3 + 2];
    best[k] = 0xFFFFFFFFu;
    bidx[k] = 0x7FFFFFFF;
  }
  const int32_t t_begin = (int32_t)blockIdx.y * chunk;  // chunk * gridDim.y < T + chunk <= 2^31 - 1 + chunk: see the launcher
  const int32_t t_end = (int32_t)min((int64_t)T, (int64_t)t_begin + chunk);
  const int ntiles = (t_end - t_begin + kNnTile - 1) / kNnTile;
  const int64_t lim = (int64_t)t_end * 3;
  float stage[kNnStage];
  auto load = [&](int it) {
    const int64_t base = ((int64_t)t_begin + (int64_t)it * kNnTile) * 3 + tid;
#pragma unroll
    for (int i = 0; i < kNnStage; ++i) {
      const int64_t f = base + i * kNnThreads;
      stage[i] = f < lim ? targets[f] : 0.0f;
    }
  };
  auto store = [&](int buf) {
    float *dst = reinterpret_cast<float *>(tile[buf]);
#pragma unroll
    for (int i = 0; i < kNnStage; ++i) {
      const int l = tid + i * kNnThreads;
      dst[(l / 3) * 4 + l % 3] = stage[i];
    }
  };
  load(0);
  store(0);
  __syncthreads();
  for (int it = 0; it < ntiles; ++it) {
    if (it + 1 < ntiles) load(it + 1);
    const float4 *cur = tile[it & 1];
    const int32_t tile_base = t_begin + it * kNnTile;
    const int nvalid = min(kNnTile, t_end - tile_base);
#pragma unroll 8
    for (int j = 0; j < nvalid; ++j) {
      const float4 t = cur[j];
      const int32_t tj = tile_base + j;
#pragma unroll
      for (int k = 0; k < kNnQpt; ++k) {
        const float dx = qx[k] - t.x, dy = qy[k] - t.y, dz = qz[k] - t.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const uint32_t b = __float_as_uint(d2);
        const bool better = b < best[k];
        best[k] = better ? b : best[k];
        bidx[k] = better ? tj : bidx[k];
      }
    }
    if (it + 1 < ntiles) store((it + 1) & 1);
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kNnQpt; ++k) {
    const int64_t q = qbase + (int64_t)k * kNnThreads;
    if (q < Q) atomicMin(&keys[q], ((unsigned long long)best[k] << 32) | (uint32_t)bidx[k]);
  }
}

__global__ __launch_bounds__(256) void nn_fill_kernel(unsigned long long *__restrict__ keys, int64_t Q) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < Q) keys[i] = ~0ull;
}

__global__ __launch_bounds__(256) void nn_finish_kernel(const unsigned long long *__restrict__ keys, int64_t Q,
                                                        float *__restrict__ dist, int32_t *__restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Q) return;
  const unsigned long long k = keys[i];
  const uint32_t bits = (uint32_t)(k >> 32);
  if (bits > 0x7F800000u) {  // every d2 of this query is NaN: no winner
    dist[i] = __uint_as_float(0x7FC00000u);
    idx[i] = -1;
  } else {
    // float64 sqrt of a float32, rounded to float32, is the correctly rounded float32 sqrt (53 >= 2 * 24 + 2)
    dist[i] = (float)sqrt((double)__uint_as_float(bits));
    idx[i] = (int32_t)(uint32_t)k;
  }
}

// ---- epilogue --------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_unit(const void *p, int is_f64, int64_t row, double out[3]) {
  double v[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) v[a] = is_f64 ? ((const double *)p)[row * 3 + a] : (double)((const float *)p)[row * 3 + a];
  const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
#pragma unroll
  for (int a = 0; a < 3; ++a) out[a] = v[a] / len;
}

__global__ __launch_bounds__(256) void normals_dot_kernel(const void *__restrict__ nq, const void *__restrict__ nt, int is_f64,
                                                          const int32_t *__restrict__ idx, int64_t Q, int64_t T,
                                                          double *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Q) return;
  const int64_t j = idx[i];
  if (j < 0 || j >= T) {
    out[i] = __longlong_as_double(0x7FF8000000000000ll);
    return;
  }
  double a[3], b[3];
  load_unit(nq, is_f64, i, a);
  load_unit(nt, is_f64, j, b);
  out[i] = fabs((b[0] * a[0] + b[1] * a[1]) + b[2] * a[2]);
}

// Fixed-order float64 sums: kSumBlocks x 256 threads, thread t of block b adds elements (b * 256 + t) + m * stride in
// ascending m, the block folds its 256 values in a fixed binary tree, and ONE block folds the kSumBlocks partials in
// the same tree.  Grid and order do not depend on the data or the device's schedule: bit-identical run to run.
constexpr int kSumBlocks = 256;

__device__ __forceinline__ double block_tree_sum(double v, double *sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void eval_sums_partial_kernel(const float *__restrict__ dist, const double *__restrict__ dot,
                                                                int64_t n, double *__restrict__ partial) {
  __shared__ double sh[256];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)kSumBlocks * 256) {
    const double d = (double)dist[i];
    s0 += d;
    s1 += d * d;
    if (dot) s2 += dot[i];
  }
  s0 = block_tree_sum(s0, sh);
  s1 = block_tree_sum(s1, sh);
  s2 = block_tree_sum(s2, sh);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = s0;
    partial[kSumBlocks + blockIdx.x] = s1;
    partial[2 * kSumBlocks + blockIdx.x] = s2;
  }
}

__global__ __launch_bounds__(256) void eval_sums_final_kernel(const double *__restrict__ partial, int has_dot,
                                                              double *__restrict__ sums) {
  __shared__ double sh[256];
  for (int c = 0; c < 3; ++c) {
    const double r = block_tree_sum(partial[c * kSumBlocks + threadIdx.x], sh);
    if (threadIdx.x == 0) sums[c] = (c == 2 && !has_dot) ? __longlong_as_double(0x7FF8000000000000ll) : r;
  }
}

// counts of a & b and a | b (integer adds: any order gives the same number)
__global__ __launch_bounds__(256) void iou_counts_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int64_t n,
                                                         unsigned long long *__restrict__ counts) {
  __shared__ unsigned long long sh[2];
  if (threadIdx.x < 2) sh[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long ci = 0, cu = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const bool x = a[i] != 0, y = b[i] != 0;
    ci += (x && y);
    cu += (x || y);
  }
  atomicAdd(&sh[0], ci);
  atomicAdd(&sh[1], cu);
  __syncthreads();
  if (threadIdx.x < 2) atomicAdd(&counts[threadIdx.x], sh[threadIdx.x]);
}

}  // namespace

extern "C" int svr_mesh_face_table(const double *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces,
                                   double *normals_out, double *cum_area_out) {
  SVR_CHECK(verts && faces && normals_out && cum_area_out && n_verts > 0 && n_faces > 0, SVR_E_BADARG,
            "mesh_face_table: bad argument (n_verts=%ld n_faces=%ld)", (long)n_verts, (long)n_faces);
  for (int64_t f = 0; f < n_faces * 3; ++f)
    SVR_CHECK(faces[f] >= 0 && faces[f] < n_verts, SVR_E_BADARG, "mesh_face_table: face index out of range");
  double run = 0.0;
  for (int64_t f = 0; f < n_faces; ++f) {
    const double *A = verts + (int64_t)faces[f * 3] * 3, *B = verts + (int64_t)faces[f * 3 + 1] * 3,
                 *Cc = verts + (int64_t)faces[f * 3 + 2] * 3;
    const double e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
    const double e2x = Cc[0] - A[0], e2y = Cc[1] - A[1], e2z = Cc[2] - A[2];
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double len = std::sqrt((nx * nx + ny * ny) + nz * nz);
    const bool ok = len > 0.0;  // false for a zero-area face and for NaN
    normals_out[f * 3] = ok ? nx / len : 0.0;
    normals_out[f * 3 + 1] = ok ? ny / len : 0.0;
    normals_out[f * 3 + 2] = ok ? nz / len : 0.0;
    run = run + (ok ? 0.5 * len : 0.0);
    cum_area_out[f] = run;
  }
  return SVR_OK;
}

extern "C" int svr_mesh_sample(const double *tri, const double *cum_area, int64_t n_faces, const double *uniforms, int64_t n,
                               float *points_out, int32_t *face_out, void *stream) {
  SVR_CHECK(n >= 0 && n_faces > 0 && n_faces < (1LL << 31), SVR_E_BADARG, "mesh_sample: bad count (n=%ld n_faces=%ld)", (long)n,
            (long)n_faces);
  if (n == 0) return SVR_OK;
  SVR_CHECK(tri && cum_area && uniforms && points_out && face_out, SVR_E_BADARG, "mesh_sample: null pointer");
  hipLaunchKernelGGL(mesh_sample_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, tri, cum_area, n_faces,
                     uniforms, n, points_out, face_out);
  return launch_status("mesh_sample");
}

extern "C" int64_t svr_nn_search_workspace(int64_t Q) {
  if (Q < 0) {
    set_error("nn_search_workspace: Q=%ld", (long)Q);
    return SVR_E_BADARG;
  }
  return Q * 8;
}

extern "C" int svr_nn_search(const float *queries, int64_t Q, const float *targets, int64_t T, float *dist_out, int32_t *idx_out,
                             void *workspace, int64_t workspace_bytes, void *stream) {
  SVR_CHECK(Q >= 0, SVR_E_BADARG, "nn_search: Q=%ld", (long)Q);
  SVR_CHECK(T > 0 && T < (1LL << 31), SVR_E_BADSHAPE, "nn_search: T=%ld (need 1 <= T < 2^31)", (long)T);
  if (Q == 0) return SVR_OK;
  SVR_CHECK(queries && targets && dist_out && idx_out && workspace, SVR_E_BADARG, "nn_search: null pointer");
  SVR_CHECK(workspace_bytes >= Q * 8, SVR_E_BADARG, "nn_search: workspace %ld bytes, need %ld", (long)workspace_bytes, (long)(Q * 8));
  const int64_t qblocks = cdiv(Q, kNnQBlock);
  SVR_CHECK(qblocks < (1LL << 31), SVR_E_BADSHAPE, "nn_search: Q=%ld", (long)Q);
  // Split the targets so that the grid has ~2048 workgroups (8 per CU: Q = 100 000 alone gives 98), in whole tiles.
  const int64_t tiles = cdiv(T, kNnTile);
  int64_t split = std::min<int64_t>(std::max<int64_t>(cdiv(2048, qblocks), 1), tiles);
  const int64_t chunk = cdiv(tiles, split) * kNnTile;  // <= T + 1023 < 2^31 + 1023: fits the kernel's int32 after the cast below
  split = cdiv(T, chunk);
  SVR_CHECK(chunk < (1LL << 31) && split <= 65535, SVR_E_BADSHAPE, "nn_search: T=%ld", (long)T);
  hipStream_t s = (hipStream_t)stream;
  unsigned long long *keys = (unsigned long long *)workspace;
  hipLaunchKernelGGL(nn_fill_kernel, dim3((unsigned)cdiv(Q, 256)), dim3(256), 0, s, keys, Q);
  hipLaunchKernelGGL(nn_search_kernel, dim3((unsigned)qblocks, (unsigned)split), dim3(kNnThreads), 0, s, queries, Q, targets,
                     (int32_t)T, (int32_t)chunk, keys);
  hipLaunchKernelGGL(nn_finish_kernel, dim3((unsigned)cdiv(Q, 256)), dim3(256), 0, s, keys, Q, dist_out, idx_out);
  return launch_status("nn_search");
}

extern "C" int svr_nn_normals_dot(const void *normals_q, const void *normals_t, int32_t normals_f64, const int32_t *idx, int64_t Q,
                                  int64_t T, double *dot_out, void *stream) {
  SVR_CHECK(Q >= 0 && T > 0, SVR_E_BADARG, "nn_normals_dot: Q=%ld T=%ld", (long)Q, (long)T);
  if (Q == 0) return SVR_OK;
  SVR_CHECK(normals_q && normals_t && idx && dot_out, SVR_E_BADARG, "nn_normals_dot: null pointer");
  hipLaunchKernelGGL(normals_dot_kernel, dim3((unsigned)cdiv(Q, 256)), dim3(256), 0, (hipStream_t)stream, normals_q, normals_t,
                     normals_f64, idx, Q, T, dot_out);
  return launch_status("nn_normals_dot");
}

extern "C" int svr_eval_sums(const float *dist, const double *dot, int64_t n, double *sums_out, void *workspace,
                             int64_t workspace_bytes, void *stream) {
  SVR_CHECK(n >= 0 && dist && sums_out && workspace, SVR_E_BADARG, "eval_sums: bad argument (n=%ld)", (long)n);
  SVR_CHECK(workspace_bytes >= SVR_EVAL_SUMS_WORKSPACE_BYTES, SVR_E_BADARG, "eval_sums: workspace %ld bytes, need %d",
            (long)workspace_bytes, SVR_EVAL_SUMS_WORKSPACE_BYTES);
  static_assert(SVR_EVAL_SUMS_WORKSPACE_BYTES == 3 * kSumBlocks * 8, "header and kernel disagree");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(eval_sums_partial_kernel, dim3(kSumBlocks), dim3(256), 0, s, dist, dot, n, (double *)workspace);
  hipLaunchKernelGGL(eval_sums_final_kernel, dim3(1), dim3(256), 0, s, (const double *)workspace, dot != nullptr, sums_out);
  return launch_status("eval_sums");
}

extern "C" int svr_iou_counts(const uint8_t *a, const uint8_t *b, int64_t n, int64_t *counts_out, void *stream) {
  SVR_CHECK(n >= 0 && counts_out && (n == 0 || (a && b)), SVR_E_BADARG, "iou_counts: bad argument (n=%ld)", (long)n);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts_out, 0, 16, s);
  if (e != hipSuccess) {
    set_error("iou_counts: memset failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  if (n == 0) return SVR_OK;
  const int64_t blocks = std::min<int64_t>(cdiv(n, 256), 4096);
  hipLaunchKernelGGL(iou_counts_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, b, n, (unsigned long long *)counts_out);
  return launch_status("iou_counts");
}
