// Connected components of a triangle mesh on the device, their integer statistics and the filter that drops some of them, gfx950.
//
// The rule is written down in include/svr_hip.h and restated in numpy by tests/mesh_components_oracle.py.
// Nothing here is a float operation: labels, counts and compaction offsets are integers, the bounding box is an integer
// minimum / maximum of an order-preserving image of the float bits, kept vertices are copied as words.  So the order in which
// atomics land cannot change a bit of any output.
//   labelling  mcc_init_kernel     parent[i] = i
//              mcc_hook_kernel     one thread per valid face: lock-free union-find, links (a, b) and (b, c)
//              mcc_flatten_kernel  one thread per vertex: walks to its root, writes root_of[i] and the flag root_of[i] == i
//              scan_sum_excl_i32   flag -> rank: the number of roots below i (sort.hip, rocPRIM)
//              mcc_relabel_kernel  vertex_label[i] = rank[root_of[i]]; face_label[f] = vertex_label[first index] or -1; C
//   statistics mcc_rows_init_kernel; mcc_vertex_stats_kernel and mcc_face_stats_kernel: integer atomics into one 40-byte row
//              per component, folded across the wave first where its items share a label; mcc_rows_final_kernel decodes
//   filter     mcc_keep_kernel (flags), two scans, mcc_totals_kernel; mcc_emit_kernel scatters
//
// The union-find's invariant: parent[i] <= i at all times, and parent[i] < i once i is no root.  init sets parent[i] = i; the
// only writes after it are (1) the hooking compare-and-swap, which replaces parent[hi] == hi by lo < hi, and (2) path halving,
// which replaces the parent of a non-root by that parent's parent: an ancestor, so smaller again.  A word that has stopped
// being a root never becomes one again.  Hence every step of find() strictly descends, every retry of link() strictly lowers
// max(hi, lo), and no interleaving of threads can make either spin: both end after at most V steps whatever the others do.
// Only the hook launch writes `parent`; flatten is a launch of its own and reads it with plain loads: stream order is the barrier.
//
// Inside the hook launch `parent` is read with relaxed agent-scope atomic loads and halved with relaxed agent-scope atomic
// stores (served by L2: a CU's L1 is not refreshed by another CU's atomics).  A stale value would be harmless as well -- edges
// are never removed, an old parent is still an ancestor, and whether a hook happens is decided by the compare-and-swap at L2 --
// but it would cost retries, so the loads go where the atomics go.
#include "common.h"
#include <algorithm>

using namespace svr;

namespace {

constexpr int kBlock = 256;
constexpr int kPerThread = 8;  // vertices (faces) per thread of the statistics kernels
constexpr int kRow = 10;// words per component in the statistics rows: root, vertices, faces, marked, min xyz, max xyz
constexpr uint32_t kNoMin = 0xffffffffu, kNoMax = 0u;  // keys of NaN bit patterns: no coordinate that takes part maps to them

__device__ __forceinline__ int32_t load_parent(const int32_t *parent, int32_t i) {
  return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x.  Each step goes from x to parent[x] < x (the invariant), so it ends.  Halving: x's parent becomes its grandparent,
// an ancestor of x; x is no root then (p != x) and no compare-and-swap can succeed on its word.
__device__ __forceinline__ int32_t find_root(int32_t *parent, int32_t x) {
  int32_t p = load_parent(parent, x);
  while (p != x) {
    const int32_t g = load_parent(parent, p);
    if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = g;
  }
  return x;
}

// joins the trees of a and b: the larger root goes under the smaller.  When the compare-and-swap finds the word changed, the
// value it returns is that word's parent: smaller than hi, and in hi's tree -- go on from its root.  max(hi, lo) falls strictly.
__device__ __forceinline__ void link(int32_t *parent, int32_t a, int32_t b) {
  int32_t hi = find_root(parent, a), lo = find_root(parent, b);
  while (hi != lo) {
    if (hi < lo) {
      const int32_t t = hi;
      hi = lo;
      lo = t;
    }
    const int32_t seen = atomicCAS(parent + hi, hi, lo);
    if (seen == hi) return;  // hi was a root and now hangs under lo < hi
    hi = find_root(parent, seen);
  }
}

__global__ __launch_bounds__(kBlock) void mcc_init_kernel(int32_t *__restrict__ parent, int64_t V) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < V) parent[i] = (int32_t)i;
}

__device__ __forceinline__ bool valid_face(int32_t a, int32_t b, int32_t c, int64_t V) {
  return a >= 0 && b >= 0 && c >= 0 && (int64_t)a < V && (int64_t)b < V && (int64_t)c < V;
}

__global__ __launch_bounds__(kBlock) void mcc_hook_kernel(const int32_t *__restrict__ faces, int64_t F, int64_t V, int32_t *parent) {
  const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  const int32_t a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  if (!valid_face(a, b, c, V)) return;  // an index that is no vertex must not become an address
  if (a != b) link(parent, a, b);
  if (b != c) link(parent, b, c);
}

__global__ __launch_bounds__(kBlock) void mcc_flatten_kernel(const int32_t *__restrict__ parent, int64_t V, int32_t *__restrict__ root_of,
                                                             int32_t *__restrict__ is_root) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= V) return;
  int32_t x = (int32_t)i, p = parent[x];
  while (p != x) {  // strictly descending, as in find_root; nothing writes parent during this launch
    x = p;
    p = parent[x];
  }
  root_of[i] = x;
  is_root[i] = x == (int32_t)i;
}

// one grid over max(V, F): thread i relabels vertex i and face i; the thread of the last vertex also writes C
__global__ __launch_bounds__(kBlock) void mcc_relabel_kernel(const int32_t *__restrict__ root_of, const int32_t *__restrict__ is_root,
                                                             const int32_t *__restrict__ rank, int64_t V, const int32_t *__restrict__ faces,
                                                             int64_t F, int32_t *__restrict__ vertex_label, int32_t *__restrict__ face_label,
                                                             long long *__restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < V) {
    vertex_label[i] = rank[root_of[i]];
    if (i == V - 1) *count = (long long)rank[i] + is_root[i];
  }
  if (i < F) {
    const int32_t a = faces[i * 3 + 0], b = faces[i * 3 + 1], c = faces[i * 3 + 2];
    face_label[i] = valid_face(a, b, c, V) ? rank[root_of[a]] : -1;
  }
}

// ---- statistics ----------------------------------------------------------------------------------------------------------
// float bits -> uint32 whose unsigned order is the float order (-inf < ... < -0 < +0 < ... < +inf; NaNs beyond both ends)
__device__ __forceinline__ uint32_t order_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ uint32_t key_bits(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu); }

__global__ __launch_bounds__(kBlock) void mcc_rows_init_kernel(uint32_t *__restrict__ rows, int64_t C) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= C * kRow) return;
  const int w = (int)(i % kRow);
  rows[i] = w == 0 ? 0x7fffffffu : w < 4 ? 0u : w < 7 ? kNoMin : kNoMax;
}

// What a set of vertices of one component adds to its row
struct VertexSums {
  uint32_t n, m, first, lo[3], hi[3];
};
__device__ __forceinline__ VertexSums no_vertices() {
  return VertexSums{0u, 0u, 0x7fffffffu, {kNoMin, kNoMin, kNoMin}, {kNoMax, kNoMax, kNoMax}};
}
__device__ __forceinline__ void merge(VertexSums &a, const VertexSums &b) {
  a.n += b.n;
  a.m += b.m;
  a.first = min(a.first, b.first);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.lo[k] = min(a.lo[k], b.lo[k]);
    a.hi[k] = max(a.hi[k], b.hi[k]);
  }
}
__device__ __forceinline__ uint32_t load_word(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One giant component would take every atomic of the launch on one 40-byte row, and atomics on one address go one after the
// other.  The counts have to be added; a minimum or maximum only has to be sent when it would change the word, so the row is
// read first (from L2: agent scope).  A value read too early is further from the result than the word is now: that costs an
// atomic that changes nothing, never a missed one.  The no-value keys never pass the comparison.
__device__ __forceinline__ void publish(uint32_t *row, const VertexSums &s) {
  if (s.first < load_word(row + 0)) atomicMin(row + 0, s.first);
  atomicAdd(row + 1, s.n);
  if (s.m) atomicAdd(row + 3, s.m);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (s.lo[k] < load_word(row + 4 + k)) atomicMin(row + 4 + k, s.lo[k]);
    if (s.hi[k] > load_word(row + 7 + k)) atomicMax(row + 7 + k, s.hi[k]);
  }
}

// the whole wave calls it: folds the lanes' sums, the first lane publishes them to row `label`, `s` is empty afterwards
__device__ __forceinline__ void flush(uint32_t *rows, int32_t label, VertexSums &s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    VertexSums t;
    t.n = __shfl_xor(s.n, o);
    t.m = __shfl_xor(s.m, o);
    t.first = __shfl_xor(s.first, o);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      t.lo[k] = __shfl_xor(s.lo[k], o);
      t.hi[k] = __shfl_xor(s.hi[k], o);
    }
    merge(s, t);
  }
  if ((threadIdx.x & 63) == 0 && s.n) publish(rows + (int64_t)label * kRow, s);
  s = no_vertices();
}

// kPerThread vertices per thread, a block's kBlock * kPerThread consecutive ones in kPerThread coalesced sweeps.  Consecutive
// vertices of a marching-cubes mesh mostly share a label: while every vertex a wave meets has the same one, each lane keeps
// its own sums in registers; the wave folds them with shuffles and its first lane issues the atomics only when the label
// changes and at the end.  A sweep in which the wave's vertices differ publishes per lane.  The conditions are the same in
// every lane, and every lane stays to the end (the shuffles need the whole wave).
__global__ __launch_bounds__(kBlock) void mcc_vertex_stats_kernel(const float *__restrict__ verts, const int32_t *__restrict__ vertex_label,
                                                                  const uint8_t *__restrict__ mark, int64_t V, int64_t C,
                                                                  uint32_t *__restrict__ rows, int uniform_path) {
  const int64_t base = (int64_t)blockIdx.x * (kBlock * kPerThread) + threadIdx.x;
  VertexSums acc = no_vertices();
  int32_t acc_label = -1;  // the same in every lane of the wave; -1: acc is empty
  for (int j = 0; j < kPerThread; ++j) {
    const int64_t i = base + (int64_t)j * kBlock;
    int32_t l = -1;
    if (i < V) l = vertex_label[i];
    const bool live = l >= 0 && (int64_t)l < C;  // a label that is no row must not become an address
    VertexSums mine = no_vertices();
    if (live) {
      mine.n = 1;
      mine.m = mark != nullptr && mark[i] != 0;
      mine.first = (uint32_t)i;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float x = verts[i * 3 + k];
        if (x == x) mine.lo[k] = mine.hi[k] = order_key(__float_as_uint(x));  // NaN is skipped
      }
    }
    const unsigned long long alive = __ballot(live);
    if (alive == 0) continue;  // the same for the whole wave
    const int32_t l0 = __shfl(l, __ffsll((long long)alive) - 1);
    if (uniform_path && __all(!live || l == l0)) {
      if (acc_label != l0) {
        if (acc_label >= 0) flush(rows, acc_label, acc);
        acc_label = l0;
      }
      merge(acc, mine);
    } else {
      if (acc_label >= 0) flush(rows, acc_label, acc);
      acc_label = -1;
      if (live) publish(rows + (int64_t)l * kRow, mine);
    }
  }
  if (acc_label >= 0) flush(rows, acc_label, acc);
}

// The same for the faces, whose only statistic is their number: the wave counts the faces of the label it keeps meeting
__device__ __forceinline__ void flush_faces(uint32_t *rows, int32_t label, uint32_t &n) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(rows + (int64_t)label * kRow + 2, n);
  n = 0;
}

__global__ __launch_bounds__(kBlock) void mcc_face_stats_kernel(const int32_t *__restrict__ face_label, int64_t F, int64_t C,
                                                                uint32_t *__restrict__ rows, int uniform_path) {
  const int64_t base = (int64_t)blockIdx.x * (kBlock * kPerThread) + threadIdx.x;
  uint32_t acc = 0;
  int32_t acc_label = -1;
  for (int j = 0; j < kPerThread; ++j) {
    const int64_t f = base + (int64_t)j * kBlock;
    int32_t l = -1;
    if (f < F) l = face_label[f];
    const bool live = l >= 0 && (int64_t)l < C;
    const unsigned long long alive = __ballot(live);
    if (alive == 0) continue;
    const int32_t l0 = __shfl(l, __ffsll((long long)alive) - 1);
    if (uniform_path && __all(!live || l == l0)) {
      if (acc_label != l0) {
        if (acc_label >= 0) flush_faces(rows, acc_label, acc);
        acc_label = l0;
      }
      acc += live;
    } else {
      if (acc_label >= 0) flush_faces(rows, acc_label, acc);
      acc_label = -1;
      if (live) atomicAdd(rows + (int64_t)l * kRow + 2, 1u);
    }
  }
  if (acc_label >= 0) flush_faces(rows, acc_label, acc);
}

__global__ __launch_bounds__(kBlock) void mcc_rows_final_kernel(const uint32_t *__restrict__ rows, int64_t C, int32_t *__restrict__ root,
                                                                int32_t *__restrict__ vertex_count, int32_t *__restrict__ face_count,
                                                                int32_t *__restrict__ marked_count, uint32_t *__restrict__ bbox_min,
                                                                uint32_t *__restrict__ bbox_max) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= C) return;
  const uint32_t *row = rows + c * kRow;
  root[c] = (int32_t)row[0];
  vertex_count[c] = (int32_t)row[1];
  face_count[c] = (int32_t)row[2];
  marked_count[c] = (int32_t)row[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    bbox_min[c * 3 + k] = row[4 + k] == kNoMin ? 0x7f800000u : key_bits(row[4 + k]);  // no value: +inf / -inf
    bbox_max[c * 3 + k] = row[7 + k] == kNoMax ? 0xff800000u : key_bits(row[7 + k]);
  }
}

// ---- filter --------------------------------------------------------------------------------------------------------------
// A kept face is a valid face of a kept component; a kept vertex is a corner of a kept face (its component is kept and it
// lies in a valid face -- the same set).  vertex_keep was zeroed before; the stores below all write 1.
__global__ __launch_bounds__(kBlock) void mcc_keep_kernel(const int32_t *__restrict__ faces, int64_t F, int64_t V,
                                                          const int32_t *__restrict__ vertex_label, const uint8_t *__restrict__ keep,
                                                          int64_t C, int32_t *__restrict__ vertex_keep, int32_t *__restrict__ face_keep) {
  const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  const int32_t a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  bool kept = false;
  if (valid_face(a, b, c, V)) {
    const int32_t l = vertex_label[a];
    kept = l >= 0 && (int64_t)l < C && keep[l] != 0;
  }
  face_keep[f] = kept;
  if (kept) {
    vertex_keep[a] = 1;
    vertex_keep[b] = 1;
    vertex_keep[c] = 1;
  }
}

__global__ void mcc_totals_kernel(const int32_t *__restrict__ vertex_keep, const int32_t *__restrict__ vertex_off, int64_t V,
                                  const int32_t *__restrict__ face_keep, const int32_t *__restrict__ face_off, int64_t F,
                                  long long *__restrict__ totals) {
  totals[0] = V > 0 ? (long long)vertex_off[V - 1] + vertex_keep[V - 1] : 0;
  totals[1] = F > 0 ? (long long)face_off[F - 1] + face_keep[F - 1] : 0;
}

// one grid over max(V, F): thread i moves vertex i (its three words, bit for bit) and face i
__global__ __launch_bounds__(kBlock) void mcc_emit_kernel(const uint32_t *__restrict__ verts, int64_t V, const int32_t *__restrict__ faces,
                                                          int64_t F, const int32_t *__restrict__ vertex_keep,
                                                          const int32_t *__restrict__ vertex_off, const int32_t *__restrict__ face_keep,
                                                          const int32_t *__restrict__ face_off, uint32_t *__restrict__ out_verts,
                                                          int32_t *__restrict__ out_faces, int32_t *__restrict__ vertex_index) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < V && vertex_keep[i]) {
    const int64_t j = vertex_off[i];
    out_verts[j * 3 + 0] = verts[i * 3 + 0];
    out_verts[j * 3 + 1] = verts[i * 3 + 1];
    out_verts[j * 3 + 2] = verts[i * 3 + 2];
    vertex_index[j] = (int32_t)i;
  }
  if (i < F && face_keep[i]) {  // a kept face is valid: its indices were tested by mcc_keep_kernel
    const int64_t j = face_off[i];
    out_faces[j * 3 + 0] = vertex_off[faces[i * 3 + 0]];
    out_faces[j * 3 + 1] = vertex_off[faces[i * 3 + 1]];
    out_faces[j * 3 + 2] = vertex_off[faces[i * 3 + 2]];
  }
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 0 && V < (1LL << 31) && F >= 0 && F < (1LL << 31); }
size_t scan_temp(int64_t n) { return n > 0 ? scan_sum_excl_i32_temp_bytes(n) : 0; }

// One buffer serves the three stages in turn, each with a layout of its own; the exported size is the largest of the three.
struct LabelWs { int32_t *parent, *root_of, *is_root, *rank; char *tmp; size_t tmp_bytes; };
LabelWs label_layout(WsCursor &c, int64_t V) {
  const size_t tmp_bytes = scan_temp(V);
  return {c.take<int32_t>(V), c.take<int32_t>(V), c.take<int32_t>(V), c.take<int32_t>(V), c.take<char>((int64_t)tmp_bytes), tmp_bytes};
}
// the statistics rows: C <= V of them
uint32_t *rows_layout(WsCursor &c, int64_t V) { return c.take<uint32_t>(V * kRow); }
// the filter's pieces: count leaves them for emit; one temp piece serves the vertex scan and the face scan
struct FilterWs { int32_t *vertex_keep, *vertex_off, *face_keep, *face_off; char *tmp; size_t vertex_tmp_bytes, face_tmp_bytes; };
FilterWs filter_layout(WsCursor &c, int64_t V, int64_t F) {
  const size_t tv = scan_temp(V), tf = scan_temp(F);
  return {c.take<int32_t>(V), c.take<int32_t>(V), c.take<int32_t>(F), c.take<int32_t>(F), c.take<char>((int64_t)std::max(tv, tf)), tv, tf};
}

unsigned blocks(int64_t n) { return (unsigned)cdiv(n, kBlock); }

}  // namespace

extern "C" int64_t svr_mesh_components_workspace_bytes(int64_t V, int64_t F) {
  SVR_CHECK(sizes_ok(V, F), SVR_E_BADSHAPE, "mesh_components_workspace_bytes: V=%ld F=%ld (need 0 <= V, F < 2^31)", (long)V, (long)F);
  return std::max(std::max(ws_measure(label_layout, V), ws_measure(rows_layout, V)), ws_measure(filter_layout, V, F));
}

extern "C" int svr_mesh_components_label(const int32_t *faces, int64_t F, int64_t V, void *ws, int64_t ws_bytes, int32_t *vertex_label,
                                         int32_t *face_label, int64_t *count, void *stream) {
  SVR_CHECK(sizes_ok(V, F), SVR_E_BADSHAPE, "mesh_components_label: V=%ld F=%ld (need 0 <= V, F < 2^31)", (long)V, (long)F);
  SVR_CHECK(count, SVR_E_BADARG, "mesh_components_label: null count");
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), s);
  SVR_CHECK(e == hipSuccess, (int)e, "mesh_components_label: memset failed: %s", hipGetErrorString(e));
  if (V == 0 && F == 0) return SVR_OK;
  SVR_CHECK((V == 0 || (vertex_label && ws)) && (F == 0 || (faces && face_label)), SVR_E_BADARG, "mesh_components_label: null pointer");
  if (V == 0) {  // no vertex: no face is valid
    e = hipMemsetAsync(face_label, 0xff, (size_t)F * 4, s);
    SVR_CHECK(e == hipSuccess, (int)e, "mesh_components_label: memset failed: %s", hipGetErrorString(e));
    return SVR_OK;
  }
  WsCursor c(ws);
  const LabelWs w = label_layout(c, V);
  SVR_CHECK(ws_bytes >= c.bytes(), SVR_E_BADARG, "mesh_components_label: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)c.bytes());
  hipLaunchKernelGGL(mcc_init_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, w.parent, V);
  if (F > 0) hipLaunchKernelGGL(mcc_hook_kernel, dim3(blocks(F)), dim3(kBlock), 0, s, faces, F, V, w.parent);
  hipLaunchKernelGGL(mcc_flatten_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, w.parent, V, w.root_of, w.is_root);
  if (int rc = launch_status("mesh_components_label")) return rc;
  e = scan_sum_excl_i32(w.tmp, w.tmp_bytes, w.is_root, w.rank, V, s);
  SVR_CHECK(e == hipSuccess, (int)e, "mesh_components_label: scan failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(mcc_relabel_kernel, dim3(blocks(std::max(V, F))), dim3(kBlock), 0, s, w.root_of, w.is_root, w.rank, V, faces, F,
                     vertex_label, face_label, (long long *)count);
  return launch_status("mesh_components_relabel");
}

extern "C" int svr_mesh_components_stats(const float *verts, int64_t V, const int32_t *vertex_label, const int32_t *face_label, int64_t F,
                                         const uint8_t *mark, int64_t C, void *ws, int64_t ws_bytes, int32_t *root, int32_t *vertex_count,
                                         int32_t *face_count, int32_t *marked_count, float *bbox_min, float *bbox_max, int32_t uniform_path,
                                         void *stream) {
  SVR_CHECK(sizes_ok(V, F), SVR_E_BADSHAPE, "mesh_components_stats: V=%ld F=%ld (need 0 <= V, F < 2^31)", (long)V, (long)F);
  SVR_CHECK(C >= 0 && C <= V, SVR_E_BADSHAPE, "mesh_components_stats: C=%ld components of V=%ld vertices", (long)C, (long)V);
  if (C == 0) return SVR_OK;
  SVR_CHECK(verts && vertex_label && (F == 0 || face_label) && ws && root && vertex_count && face_count && marked_count && bbox_min &&
                bbox_max,
            SVR_E_BADARG, "mesh_components_stats: null pointer");
  WsCursor c(ws);
  uint32_t *rows = rows_layout(c, V);
  SVR_CHECK(ws_bytes >= c.bytes(), SVR_E_BADARG, "mesh_components_stats: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)c.bytes());
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mcc_rows_init_kernel, dim3(blocks(C * kRow)), dim3(kBlock), 0, s, rows, C);
  const int uniform = uniform_path != 0;
  hipLaunchKernelGGL(mcc_vertex_stats_kernel, dim3(blocks(cdiv(V, kPerThread))), dim3(kBlock), 0, s, verts, vertex_label, mark, V, C, rows, uniform);
  if (F > 0)
    hipLaunchKernelGGL(mcc_face_stats_kernel, dim3(blocks(cdiv(F, kPerThread))), dim3(kBlock), 0, s, face_label, F, C, rows, uniform);
  hipLaunchKernelGGL(mcc_rows_final_kernel, dim3(blocks(C)), dim3(kBlock), 0, s, rows, C, root, vertex_count, face_count, marked_count,
                     (uint32_t *)bbox_min, (uint32_t *)bbox_max);
  return launch_status("mesh_components_stats");
}

extern "C" int svr_mesh_filter_count(const int32_t *faces, int64_t F, int64_t V, const int32_t *vertex_label, const uint8_t *keep, int64_t C,
                                     void *ws, int64_t ws_bytes, int64_t *totals, void *stream) {
  SVR_CHECK(sizes_ok(V, F), SVR_E_BADSHAPE, "mesh_filter_count: V=%ld F=%ld (need 0 <= V, F < 2^31)", (long)V, (long)F);
  SVR_CHECK(C >= 0 && C <= V, SVR_E_BADSHAPE, "mesh_filter_count: C=%ld components of V=%ld vertices", (long)C, (long)V);
  SVR_CHECK(totals, SVR_E_BADARG, "mesh_filter_count: null totals");
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s);
  SVR_CHECK(e == hipSuccess, (int)e, "mesh_filter_count: memset failed: %s", hipGetErrorString(e));
  if (V == 0 || F == 0) return SVR_OK;  // no valid face: nothing is kept
  SVR_CHECK(faces && vertex_label && keep && ws, SVR_E_BADARG, "mesh_filter_count: null pointer");
  WsCursor c(ws);
  const FilterWs w = filter_layout(c, V, F);
  SVR_CHECK(ws_bytes >= c.bytes(), SVR_E_BADARG, "mesh_filter_count: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)c.bytes());
  e = hipMemsetAsync(w.vertex_keep, 0, (size_t)V * 4, s);
  SVR_CHECK(e == hipSuccess, (int)e, "mesh_filter_count: memset failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(mcc_keep_kernel, dim3(blocks(F)), dim3(kBlock), 0, s, faces, F, V, vertex_label, keep, C, w.vertex_keep, w.face_keep);
  if (int rc = launch_status("mesh_filter_keep")) return rc;
  e = scan_sum_excl_i32(w.tmp, w.vertex_tmp_bytes, w.vertex_keep, w.vertex_off, V, s);
  if (e == hipSuccess) e = scan_sum_excl_i32(w.tmp, w.face_tmp_bytes, w.face_keep, w.face_off, F, s);
  SVR_CHECK(e == hipSuccess, (int)e, "mesh_filter_count: scan failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(mcc_totals_kernel, dim3(1), dim3(1), 0, s, w.vertex_keep, w.vertex_off, V, w.face_keep, w.face_off, F,
                     (long long *)totals);
  return launch_status("mesh_filter_count");
}

extern "C" int svr_mesh_filter_emit(const float *verts, int64_t V, const int32_t *faces, int64_t F, void *ws, int64_t ws_bytes,
                                    float *out_verts, int32_t *out_faces, int32_t *vertex_index, void *stream) {
  SVR_CHECK(sizes_ok(V, F), SVR_E_BADSHAPE, "mesh_filter_emit: V=%ld F=%ld (need 0 <= V, F < 2^31)", (long)V, (long)F);
  if (V == 0 || F == 0) return SVR_OK;
  SVR_CHECK(verts && faces && ws && out_verts && out_faces && vertex_index, SVR_E_BADARG, "mesh_filter_emit: null pointer");
  WsCursor c(ws);
  const FilterWs w = filter_layout(c, V, F);
  SVR_CHECK(ws_bytes >= c.bytes(), SVR_E_BADARG, "mesh_filter_emit: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)c.bytes());
  hipLaunchKernelGGL(mcc_emit_kernel, dim3(blocks(std::max(V, F))), dim3(kBlock), 0, (hipStream_t)stream, (const uint32_t *)verts, V, faces,
                     F, w.vertex_keep, w.vertex_off, w.face_keep, w.face_off, (uint32_t *)out_verts, out_faces, vertex_index);
  return launch_status("mesh_filter_emit");
}
