// Taubin lambda|mu smoothing of a triangle mesh on the device, gfx950, by an all-integer rule.
//
// The rule is written down in include/svr_hip.h and restated in numpy by tests/mesh_smooth_oracle.py.
// The positions are int64 fixed point (16 fractional bits) from the first kernel to the last; the only floating-point
// operations are the conversion of each vertex's own words at either end.  An inverted index is built once -- per vertex the
// list of its (next, prev) entries, one per corner of a valid face -- and every pass is then a pure gather over it:
//   svr_mesh_smooth  sm_prepare_kernel   one thread per vertex: usable?  q -> BOTH rows of the ping-pong pair; degree = cursor = 0;
//                                        state = 3 (not usable) or 0 for now, which is what the face kernels test
//                    sm_count_kernel     one thread per face: valid?  atomicAdd(degree[corner], 1) x 3
//                    scan_sum_excl_i32   degree -> offset (sort.hip, rocPRIM); 3 F <= 3 * 2^28 < 2^31
//                    sm_fill_kernel      one thread per valid face: per corner slot = offset + atomicAdd(cursor, 1), then the
//                                        (next, prev) pair as one 8-byte store
//                    sm_classify_kernel  one thread per vertex: the interior test over its own list, the state, the four counts
//                    sm_step_kernel      one thread per movable vertex: walks its list, sums the rows of next and prev, applies
//                                        the rule, writes the other row of the pair; launched n or 2 n times
//                    sm_finish_kernel    one thread per vertex: a moved vertex converts its q, every other copies its words
//   F == 0           sm_no_faces_kernel  state 1 or 3, the counts, the copy; no workspace
// Why no bit depends on the order of atomics: the degrees and the cursors are integer counts; the order in which
// sm_fill_kernel's cursor atomics land decides only WHERE in its owner's list an entry sits, never which list or which entry.
// What is computed from a list is a sum of integers (S) and a comparison of multisets (for every j, as many entries with
// next == j as with prev == j): both are the same for every order of the list.  The counts are integer sums.  The unit is
// built with -ffp-contract=off, though it holds no float operation that could contract.
// Why the passes need nothing zeroed and no copy: sm_prepare_kernel writes the initial q into both rows; a pass reads row A and
// writes row B for the movable vertices only, the others hold their initial q in both rows for good.  A pass is one launch
// (Jacobi: stream order is the barrier between reading the old q and reading the new).
// Bounds: every face index is compared with [0, V) before it addresses anything (face_corners), in both face kernels, which
// therefore agree on which faces are valid; a list entry names corners of a valid face, so the step kernel's gathers stay
// inside the rows; a slot is offset + (a value below degree) because count and fill see the same valid faces.
#include "common.h"
#include <algorithm>

using namespace svr;

namespace {

constexpr int kBlock = 256;
constexpr float kCoordLimit = 65536.0f;
constexpr double kFixed = 65536.0;                 // 16 fractional bits
constexpr long long kQLimit = 1LL << 33;           // the clamp: keeps |S + m| <= 2^29 * 2^33 + 2^28 inside int64
constexpr int32_t kMaxIterations = 1024;
constexpr int64_t kMaxFaces = 1LL << 28;
enum : uint8_t { kMovable = 0, kIsolated = 1, kFixedState = 2, kBad = 3 };

struct alignas(32) Row {                           // one vertex's q; w pads the row to 32 bytes: two 16-byte loads, never split
  long long x, y, z, w;
};
struct alignas(8) Entry {
  int32_t next, prev;
};

__device__ __forceinline__ bool usable(float x, float y, float z) {  // finite and below the limit (NaN fails the comparison)
  return fabsf(x) < kCoordLimit && fabsf(y) < kCoordLimit && fabsf(z) < kCoordLimit;
}
// q = rint(v 2^16), ties to even; the product is exact (a power of two) and |q| < 2^32
__device__ __forceinline__ long long fixed(float v) { return (long long)rint((double)v * kFixed); }

// the wave adds its number of vertices in each state once.  Every lane of the wave calls it; state 255: no vertex
__device__ __forceinline__ void count_states(uint8_t state, unsigned long long *counts) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long m = __ballot(state == k);
    if (m != 0 && (threadIdx.x & 63) == 0) atomicAdd(counts + k, (unsigned long long)__popcll(m));
  }
}

__global__ __launch_bounds__(kBlock) void sm_no_faces_kernel(const uint32_t *__restrict__ verts, int64_t V, uint32_t *__restrict__ out,
                                                             uint8_t *__restrict__ state, unsigned long long *__restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  uint8_t s = 255;
  if (i < V) {
    const uint32_t x = verts[i * 3 + 0], y = verts[i * 3 + 1], z = verts[i * 3 + 2];
    s = usable(__uint_as_float(x), __uint_as_float(y), __uint_as_float(z)) ? kIsolated : kBad;
    state[i] = s;
    out[i * 3 + 0] = x;
    out[i * 3 + 1] = y;
    out[i * 3 + 2] = z;
  }
  count_states(s, counts);
}

__global__ __launch_bounds__(kBlock) void sm_prepare_kernel(const float *__restrict__ verts, int64_t V, Row *__restrict__ qa, Row *__restrict__ qb,
                                                            int32_t *__restrict__ degree, int32_t *__restrict__ cursor,
                                                            uint8_t *__restrict__ state) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= V) return;
  const float x = verts[i * 3 + 0], y = verts[i * 3 + 1], z = verts[i * 3 + 2];
  const bool ok = usable(x, y, z);
  const Row q = ok ? Row{fixed(x), fixed(y), fixed(z), 0} : Row{0, 0, 0, 0};
  qa[i] = q;
  qb[i] = q;
  degree[i] = 0;
  cursor[i] = 0;
  state[i] = ok ? kMovable : kBad;
}

// the three corners of a valid face, or false; an index that is no vertex must not become an address
__device__ __forceinline__ bool face_corners(const int32_t *__restrict__ faces, int64_t f, int64_t V, const uint8_t *__restrict__ state,
                                             int32_t *a, int32_t *b, int32_t *c) {
  *a = faces[f * 3 + 0];
  *b = faces[f * 3 + 1];
  *c = faces[f * 3 + 2];
  if (!(*a >= 0 && *b >= 0 && *c >= 0 && (int64_t)*a < V && (int64_t)*b < V && (int64_t)*c < V)) return false;
  if (*a == *b || *b == *c || *c == *a) return false;
  return state[*a] != kBad && state[*b] != kBad && state[*c] != kBad;
}

__global__ __launch_bounds__(kBlock) void sm_count_kernel(const int32_t *__restrict__ faces, int64_t F, int64_t V,
                                                          const uint8_t *__restrict__ state, int32_t *__restrict__ degree) {
  const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  int32_t a, b, c;
  if (!face_corners(faces, f, V, state, &a, &b, &c)) return;
  atomicAdd(degree + a, 1);
  atomicAdd(degree + b, 1);
  atomicAdd(degree + c, 1);
}

// `slot < degree` holds because sm_count_kernel counted the same faces; it is tested all the same, so that no store can leave
// its owner's list
__device__ __forceinline__ void put(Entry *__restrict__ entries, const int32_t *__restrict__ offset, const int32_t *__restrict__ degree,
                                    int32_t *__restrict__ cursor, int32_t owner, int32_t next, int32_t prev) {
  const int32_t slot = atomicAdd(cursor + owner, 1);
  if (slot < degree[owner]) entries[(int64_t)offset[owner] + slot] = Entry{next, prev};
}
__global__ __launch_bounds__(kBlock) void sm_fill_kernel(const int32_t *__restrict__ faces, int64_t F, int64_t V,
                                                         const uint8_t *__restrict__ state, const int32_t *__restrict__ offset,
                                                         const int32_t *__restrict__ degree, int32_t *__restrict__ cursor,
                                                         Entry *__restrict__ entries) {
  const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  int32_t a, b, c;
  if (!face_corners(faces, f, V, state, &a, &b, &c)) return;
  put(entries, offset, degree, cursor, a, b, c);
  put(entries, offset, degree, cursor, b, c, a);
  put(entries, offset, degree, cursor, c, a, b);
}

// interior: for every j, as many entries with next == j as with prev == j.  Both multisets have m elements, so it is enough to
// test the j that occur as a next.  The plain walk: d entries cost d^2 loads in this one thread (a marching-cubes vertex has a
// dozen entries at most)
__device__ __forceinline__ bool interior(const Entry *__restrict__ list, int32_t m) {
  for (int32_t e = 0; e < m; ++e) {
    const int32_t j = list[e].next;
    int32_t balance = 0;
    for (int32_t k = 0; k < m; ++k) {
      const Entry t = list[k];
      balance += (t.next == j) - (t.prev == j);
    }
    if (balance != 0) return false;
  }
  return true;
}

__global__ __launch_bounds__(kBlock) void sm_classify_kernel(int64_t V, const int32_t *__restrict__ degree, const int32_t *__restrict__ offset,
                                                             const Entry *__restrict__ entries, int fix_boundary, uint8_t *__restrict__ state,
                                                             unsigned long long *__restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  uint8_t s = 255;
  if (i < V) {
    s = state[i];
    if (s != kBad) {
      const int32_t m = degree[i];
      if (m == 0) s = kIsolated;
      else if (fix_boundary && !interior(entries + offset[i], m)) s = kFixedState;
      else s = kMovable;
      state[i] = s;
    }
  }
  count_states(s, counts);
}

__device__ __forceinline__ long long floor_div(long long t, long long c) {  // c > 0; C's `/` truncates
  const long long d = t / c;
  return d - ((t % c) < 0);
}
// step = (L (mean - q) + 32768) >> 16, an arithmetic shift; |L (mean - q)| < 2^52
__device__ __forceinline__ long long moved(long long q, long long S, long long m, long long L) {
  const long long mean = floor_div(S + m, 2 * m);
  const long long next = q + ((L * (mean - q) + 32768) >> 16);
  return next < -kQLimit ? -kQLimit : (next > kQLimit ? kQLimit : next);
}

// One thread per vertex.  The rows it gathers are 32 bytes each, 3.2 MB for 100 000 vertices, so the row a pass reads fits one
// XCD's L2 at a reconstructed mesh's size, and marching cubes numbers neighbouring vertices close to each other (DESIGN.md
// section 24 has the measured pass times).
__global__ __launch_bounds__(kBlock) void sm_step_kernel(int64_t V, const uint8_t *__restrict__ state, const int32_t *__restrict__ degree,
                                                         const int32_t *__restrict__ offset, const Entry *__restrict__ entries,
                                                         const Row *__restrict__ from, Row *__restrict__ to, long long L) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= V || state[i] != kMovable) return;
  const int32_t m = degree[i];
  const Entry *__restrict__ list = entries + offset[i];
  long long sx = 0, sy = 0, sz = 0;
  for (int32_t e = 0; e < m; ++e) {
    const Entry t = list[e];
    if ((uint64_t)(uint32_t)t.next >= (uint64_t)V || (uint64_t)(uint32_t)t.prev >= (uint64_t)V) continue;  // never: entries name vertices
    const Row a = from[t.next], b = from[t.prev];
    sx += a.x + b.x;
    sy += a.y + b.y;
    sz += a.z + b.z;
  }
  const Row q = from[i];
  to[i] = Row{moved(q.x, sx, m, L), moved(q.y, sy, m, L), moved(q.z, sz, m, L), 0};
}

__global__ __launch_bounds__(kBlock) void sm_finish_kernel(const uint32_t *__restrict__ verts, int64_t V, const uint8_t *__restrict__ state,
                                                           const Row *__restrict__ q, int convert, uint32_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= V) return;
  uint32_t x = verts[i * 3 + 0], y = verts[i * 3 + 1], z = verts[i * 3 + 2];
  if (convert && state[i] == kMovable) {
    const Row r = q[i];
    x = __float_as_uint((float)((double)r.x / kFixed));
    y = __float_as_uint((float)((double)r.y / kFixed));
    z = __float_as_uint((float)((double)r.z / kFixed));
  }
  out[i * 3 + 0] = x;
  out[i * 3 + 1] = y;
  out[i * 3 + 2] = z;
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 0 && V < (1LL << 31) && F >= 0 && F <= kMaxFaces; }

// The one layout.  Per vertex: the two rows of q, its degree (= the length of its list), the offset of its list and the fill
// cursor; per face three entries; the scan's temp piece.
struct SmoothWs {
  Row *qa, *qb;
  int32_t *degree, *offset, *cursor;
  Entry *entries;
  char *tmp;
  size_t tmp_bytes;
};
SmoothWs smooth_layout(WsCursor &c, int64_t V, int64_t F) {
  const size_t t = V > 0 ? scan_sum_excl_i32_temp_bytes(V) : 0;
  return {c.take<Row>(V), c.take<Row>(V), c.take<int32_t>(V), c.take<int32_t>(V), c.take<int32_t>(V), c.take<Entry>(3 * F), c.take<char>((int64_t)t), t};
}

unsigned blocks(int64_t n) { return (unsigned)cdiv(n, kBlock); }

// the fixed-point step weight, or false: lo <= rint((double)w 2^16) <= hi, written so that a NaN fails it
bool weight(float w, double lo, double hi, long long *L) {
  const double d = rint((double)w * kFixed);
  if (!(d >= lo && d <= hi)) return false;
  *L = (long long)d;
  return true;
}

}  // namespace

extern "C" int64_t svr_mesh_smooth_workspace_bytes(int64_t V, int64_t F) {
  SVR_CHECK(sizes_ok(V, F), SVR_E_BADSHAPE, "mesh_smooth_workspace_bytes: V=%ld F=%ld (need 0 <= V < 2^31, 0 <= F <= 2^28)", (long)V, (long)F);
  return ws_measure(smooth_layout, V, F);
}

extern "C" int svr_mesh_smooth(const float *verts, int64_t V, const int32_t *faces, int64_t F, int32_t iterations, float lam, float mu,
                               int32_t fix_boundary, void *ws, int64_t ws_bytes, float *out_verts, uint8_t *state, int64_t *counts,
                               void *stream) {
  // every refusal comes before anything is enqueued
  SVR_CHECK(sizes_ok(V, F), SVR_E_BADSHAPE, "mesh_smooth: V=%ld F=%ld (need 0 <= V < 2^31, 0 <= F <= 2^28)", (long)V, (long)F);
  SVR_CHECK(iterations >= 0 && iterations <= kMaxIterations, SVR_E_BADARG, "mesh_smooth: iterations=%d (need 0 <= iterations <= 1024)",
            (int)iterations);
  long long L_lam = 0, L_mu = 0;
  SVR_CHECK(weight(lam, 1.0, kFixed, &L_lam), SVR_E_BADARG, "mesh_smooth: lam=%g (need 0 < lam <= 1 after rounding to 2^-16)", (double)lam);
  SVR_CHECK(weight(mu, -kFixed, 0.0, &L_mu), SVR_E_BADARG, "mesh_smooth: mu=%g (need -1 <= mu <= 0 after rounding to 2^-16)", (double)mu);
  SVR_CHECK(counts, SVR_E_BADARG, "mesh_smooth: null counts");
  SmoothWs w{};
  if (V > 0) {
    SVR_CHECK(verts && out_verts && state, SVR_E_BADARG, "mesh_smooth: null pointer");
    const uintptr_t in = (uintptr_t)verts, out = (uintptr_t)out_verts, bytes = (uintptr_t)V * 12;
    SVR_CHECK(out >= in + bytes || in >= out + bytes, SVR_E_BADARG, "mesh_smooth: out_verts overlaps verts (the passes read every old position)");
    if (F > 0) {
      SVR_CHECK(faces && ws, SVR_E_BADARG, "mesh_smooth: null pointer");
      WsCursor c(ws);
      w = smooth_layout(c, V, F);
      SVR_CHECK(ws_bytes >= c.bytes(), SVR_E_BADARG, "mesh_smooth: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)c.bytes());
    }
  }
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s);
  SVR_CHECK(e == hipSuccess, (int)e, "mesh_smooth: memset failed: %s", hipGetErrorString(e));
  if (V == 0) return SVR_OK;
  unsigned long long *n = (unsigned long long *)counts;
  if (F == 0) {
    hipLaunchKernelGGL(sm_no_faces_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, (const uint32_t *)verts, V, (uint32_t *)out_verts, state, n);
    return launch_status("mesh_smooth");
  }
  hipLaunchKernelGGL(sm_prepare_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, verts, V, w.qa, w.qb, w.degree, w.cursor, state);
  hipLaunchKernelGGL(sm_count_kernel, dim3(blocks(F)), dim3(kBlock), 0, s, faces, F, V, state, w.degree);
  if (int rc = launch_status("mesh_smooth_count")) return rc;
  e = scan_sum_excl_i32(w.tmp, w.tmp_bytes, w.degree, w.offset, V, s);
  SVR_CHECK(e == hipSuccess, (int)e, "mesh_smooth: scan failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(sm_fill_kernel, dim3(blocks(F)), dim3(kBlock), 0, s, faces, F, V, state, w.offset, w.degree, w.cursor, w.entries);
  hipLaunchKernelGGL(sm_classify_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, V, w.degree, w.offset, w.entries, (int)(fix_boundary != 0), state, n);
  Row *now = w.qa, *other = w.qb;                  // `now` holds the positions after the passes so far
  for (int32_t it = 0; it < iterations; ++it) {
    for (const long long L : {L_lam, L_mu}) {
      if (L == 0) continue;                        // mu = 0: plain Laplacian, one pass per iteration
      hipLaunchKernelGGL(sm_step_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, V, state, w.degree, w.offset, w.entries, (const Row *)now, other, L);
      std::swap(now, other);
    }
  }
  hipLaunchKernelGGL(sm_finish_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, (const uint32_t *)verts, V, state, (const Row *)now,
                     (int)(iterations > 0), (uint32_t *)out_verts);
  return launch_status("mesh_smooth");
}
