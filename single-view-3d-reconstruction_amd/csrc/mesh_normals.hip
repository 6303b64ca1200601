// Area-weighted vertex normals of a triangle mesh on the device, gfx950, all-integer up to the final normalisation.
//
// The rule is written down in include/svr_hip.h and restated in numpy by tests/mesh_render_oracle.py.
// The positions become int64 fixed point (10 fractional bits), a face's cross product is computed in int64 and added to the
// three accumulators of its corners modulo 2^64; the only floating-point operations are the conversion of each vertex's own
// words and, per vertex, three conversions, one square root and three divisions at the end.
//   svr_mesh_vertex_normals  mn_zero_kernel    one thread per vertex: its three accumulators = 0
//                            mn_face_kernel    one thread per face: valid?  n = e1 x e2; nine 64-bit integer atomicAdds
//                            mn_vertex_kernel  one thread per vertex: the normal, the state, the three counts
// Why no bit depends on the order of atomics: integer addition modulo 2^64 is associative and commutative, so the sums are the
// same for every arrival order; everything after them is per vertex.  The counts are integer sums.  Built with
// -ffp-contract=off (x*x + y*y must round twice).
// Bounds: a face's three indices are compared with [0, V) before any of them addresses a vertex or an accumulator
// (face_corners); mn_vertex_kernel touches row i < V only.  F == 0: no workspace, mn_vertex_kernel sees null accumulators.
#include "common.h"

using namespace svr;

namespace {

constexpr int kBlock = 256;
constexpr float kCoordLimit = 65536.0f;
constexpr double kFixed = 1024.0;                  // 10 fractional bits: |q| <= 2^26, |e| <= 2^27, |n| <= 2^55
constexpr int64_t kMaxFaces = 1LL << 28;
enum : uint8_t { kHasNormal = 0, kNoNormal = 1, kBad = 3 };
typedef unsigned long long u64;

__device__ __forceinline__ bool usable(float x, float y, float z) {  // finite and below the limit (NaN fails the comparison)
  return fabsf(x) < kCoordLimit && fabsf(y) < kCoordLimit && fabsf(z) < kCoordLimit;
}
// q = rint(v 2^10), ties to even; the product is exact (a power of two)
__device__ __forceinline__ long long fixed(float v) { return (long long)rint((double)v * kFixed); }

__global__ __launch_bounds__(kBlock) void mn_zero_kernel(int64_t V, u64 *__restrict__ acc) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= V) return;
  acc[i * 3 + 0] = 0;
  acc[i * 3 + 1] = 0;
  acc[i * 3 + 2] = 0;
}

// the three corners of a face whose indices are vertices and pairwise distinct, or false; an index that is no vertex must not
// become an address
__device__ __forceinline__ bool face_corners(const int32_t *__restrict__ faces, int64_t f, int64_t V, int32_t *a, int32_t *b, int32_t *c) {
  *a = faces[f * 3 + 0];
  *b = faces[f * 3 + 1];
  *c = faces[f * 3 + 2];
  if (!(*a >= 0 && *b >= 0 && *c >= 0 && (int64_t)*a < V && (int64_t)*b < V && (int64_t)*c < V)) return false;
  return !(*a == *b || *b == *c || *c == *a);
}

__global__ __launch_bounds__(kBlock) void mn_face_kernel(const float *__restrict__ verts, int64_t V, const int32_t *__restrict__ faces, int64_t F,
                                                         u64 *__restrict__ acc) {
  const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  int32_t i[3];
  if (!face_corners(faces, f, V, &i[0], &i[1], &i[2])) return;
  long long q[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float x = verts[(int64_t)i[k] * 3 + 0], y = verts[(int64_t)i[k] * 3 + 1], z = verts[(int64_t)i[k] * 3 + 2];
    if (!usable(x, y, z)) return;
    q[k][0] = fixed(x), q[k][1] = fixed(y), q[k][2] = fixed(z);
  }
  const long long e1x = q[1][0] - q[0][0], e1y = q[1][1] - q[0][1], e1z = q[1][2] - q[0][2];
  const long long e2x = q[2][0] - q[0][0], e2y = q[2][1] - q[0][1], e2z = q[2][2] - q[0][2];
  const u64 nx = (u64)(e1y * e2z - e1z * e2y), ny = (u64)(e1z * e2x - e1x * e2z), nz = (u64)(e1x * e2y - e1y * e2x);
#pragma unroll
  for (int k = 0; k < 3; ++k) {                    // unsigned: the sums wrap modulo 2^64 by definition
    atomicAdd(acc + (int64_t)i[k] * 3 + 0, nx);
    atomicAdd(acc + (int64_t)i[k] * 3 + 1, ny);
    atomicAdd(acc + (int64_t)i[k] * 3 + 2, nz);
  }
}

// acc == nullptr: a mesh without faces, every sum is 0
__global__ __launch_bounds__(kBlock) void mn_vertex_kernel(const float *__restrict__ verts, int64_t V, const u64 *__restrict__ acc,
                                                           float *__restrict__ out, uint8_t *__restrict__ state, u64 *__restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  uint8_t s = 255;                                 // no vertex
  if (i < V) {
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (!usable(verts[i * 3 + 0], verts[i * 3 + 1], verts[i * 3 + 2])) {
      s = kBad;
    } else {
      s = kNoNormal;
      if (acc) {
        const double x = (double)(long long)acc[i * 3 + 0], y = (double)(long long)acc[i * 3 + 1], z = (double)(long long)acc[i * 3 + 2];
        const double len = sqrt((x * x + y * y) + z * z);
        if (len > 0.0) {
          nx = (float)(x / len), ny = (float)(y / len), nz = (float)(z / len);
          s = kHasNormal;
        }
      }
    }
    out[i * 3 + 0] = nx;
    out[i * 3 + 1] = ny;
    out[i * 3 + 2] = nz;
    state[i] = s;
  }
  // the wave adds its number of vertices in each state once; every lane of the wave gets here
  const uint8_t of[3] = {kHasNormal, kNoNormal, kBad};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const u64 m = __ballot(s == of[k]);
    if (m != 0 && (threadIdx.x & 63) == 0) atomicAdd(counts + k, (u64)__popcll(m));
  }
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 0 && V < (1LL << 31) && F >= 0 && F <= kMaxFaces; }

// the one piece: three int64 accumulators per vertex
u64 *normals_layout(WsCursor &c, int64_t V, int64_t F) { return c.take<u64>(V > 0 && F > 0 ? 3 * V : 0); }

unsigned blocks(int64_t n) { return (unsigned)cdiv(n, kBlock); }

}  // namespace

extern "C" int64_t svr_mesh_vertex_normals_workspace_bytes(int64_t V, int64_t F) {
  SVR_CHECK(sizes_ok(V, F), SVR_E_BADSHAPE, "mesh_vertex_normals_workspace_bytes: V=%ld F=%ld (need 0 <= V < 2^31, 0 <= F <= 2^28)", (long)V,
            (long)F);
  return ws_measure(normals_layout, V, F);
}

extern "C" int svr_mesh_vertex_normals(const float *verts, int64_t V, const int32_t *faces, int64_t F, void *ws, int64_t ws_bytes, float *out,
                                       uint8_t *state, int64_t *counts, void *stream) {
  // every refusal comes before anything is enqueued
  SVR_CHECK(sizes_ok(V, F), SVR_E_BADSHAPE, "mesh_vertex_normals: V=%ld F=%ld (need 0 <= V < 2^31, 0 <= F <= 2^28)", (long)V, (long)F);
  SVR_CHECK(counts, SVR_E_BADARG, "mesh_vertex_normals: null counts");
  u64 *acc = nullptr;
  if (V > 0) {
    SVR_CHECK(verts && out && state, SVR_E_BADARG, "mesh_vertex_normals: null pointer");
    const uintptr_t in = (uintptr_t)verts, o = (uintptr_t)out, bytes = (uintptr_t)V * 12;
    SVR_CHECK(o >= in + bytes || in >= o + bytes, SVR_E_BADARG, "mesh_vertex_normals: out overlaps verts");
    if (F > 0) {
      SVR_CHECK(faces && ws, SVR_E_BADARG, "mesh_vertex_normals: null pointer");
      WsCursor c(ws);
      acc = normals_layout(c, V, F);
      SVR_CHECK(ws_bytes >= c.bytes(), SVR_E_BADARG, "mesh_vertex_normals: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)c.bytes());
    }
  }
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), s);
  SVR_CHECK(e == hipSuccess, (int)e, "mesh_vertex_normals: memset failed: %s", hipGetErrorString(e));
  if (V == 0) return SVR_OK;
  if (F > 0) {
    hipLaunchKernelGGL(mn_zero_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, V, acc);
    hipLaunchKernelGGL(mn_face_kernel, dim3(blocks(F)), dim3(kBlock), 0, s, verts, V, faces, F, acc);
  }
  hipLaunchKernelGGL(mn_vertex_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, verts, V, (const u64 *)acc, out, state, (u64 *)counts);
  return launch_status("mesh_vertex_normals");
}
