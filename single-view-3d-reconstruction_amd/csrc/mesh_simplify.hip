// Vertex clustering (Rossignac-Borrel) of a triangle mesh on the device, gfx950.
//
// The rule is written down in include/svr_hip.h and restated in numpy by tests/mesh_simplify_oracle.py.
// Wherever threads meet, the values are integers: cells, slots, roots, flags, offsets, and the positions are summed as int64
// fixed point.  Floats are computed per item from that item's own words (the cell of a vertex, its fixed-point image) or from a
// finished integer sum (a cluster's vertex), so the order in which atomics land cannot change a bit of any output.
//   count  ms_fill_kernel          both hash sets "empty", the error word 0
//          ms_vertex_insert_kernel one thread per vertex: clusterable?  cell -> the vertex set; remembers its slot; counts `bad`
//          ms_vertex_root_kernel   root_of[i] = table[slot_of[i]]; a root zeroes its row of sums; used[i] = 0
//          ms_sums_kernel          int64 atomicAdd of s_x, s_y, s_z and n into the root's row, folded across the wave first
//                                  where its vertices share a root
//          ms_face_insert_kernel   one thread per face: valid?  roots, degenerate?  canonical triple -> the face set
//          ms_face_keep_kernel     keep[f] = table[slot_of[f]] == f; a kept face marks its three roots used
//          scan_sum_excl_i32 x 2   used -> the output vertex of a root, keep -> the output face (sort.hip, rocPRIM)
//          ms_totals_kernel        V', F' (bad was counted by the insert); SVR_E_INTERNAL in all three if the error word is set
//   emit   ms_emit_kernel          one grid over max(V, F): vertex_cluster, a used root's position and size, a kept face
// A cluster is named by its root, the smallest vertex index in its cell, all the way: roots order like the rule's cluster
// numbers (those ascend with the root), so the canonical rotation and the duplicate classes are the same, rows of sums and
// `used` flags are indexed by root, and the only numbering ever computed is the output's, by the scan over `used`.
//
// The hash set (HashSet below; one for the vertices, key = the cell, one for the faces, key = the canonical triple of roots).
// A slot is "empty" or holds an item index; the key is never stored, it is recomputed from the item the slot holds.
//   insert(i): probe linearly from hash(key(i)).  An empty slot: compare-and-swap empty -> i.  An occupied slot (a failed
//   compare-and-swap included; it returns the holder): if key(holder) == key(i), atomicMin(slot, i) and done, else next slot.
// Invariants: (1) a slot never returns to empty; (2) every value a slot ever holds has the key of its first value -- the only
// writes to an occupied slot are atomicMin's by items that compared equal -- so a slot's class is fixed for the launch;
// (3) a class owns at most one slot: its items all walk the same sequence from the same start, and the slots an item passed
// were occupied by other classes and stay so (1, 2), so a later item of the class reaches the class's slot before any slot
// that was empty when the first one claimed it.  Hence after the launch the class's slot holds its smallest item, whatever
// the interleaving.  Termination: the loop strictly advances one slot per turn and is bounded by the table size; it waits for
// nobody.  With 2^k >= 2 N slots and at most N classes an empty slot exists on every walk, so the bound is never reached; if
// it were, the item gives up (it is then treated as unclusterable / dropped, so every later launch stays inside its buffers)
// and sets the error word, which ms_totals_kernel turns into SVR_E_INTERNAL totals.
// Inside the insert launches slots are read with relaxed agent-scope atomic loads (served by L2, where the atomics go); the
// launch after reads them plainly: stream order is the barrier.
#include "common.h"
#include <algorithm>

using namespace svr;

namespace {

constexpr int kBlock = 256;
constexpr int kPerThread = 8;           // vertices per thread of the sums kernel
constexpr int32_t kEmpty = 0x7fffffff;  // no item: N < 2^31, so every index is below it
constexpr float kCoordLimit = 65536.0f;
constexpr double kFixed = 65536.0;      // fixed point of the sums: 16 fractional bits

__device__ __forceinline__ uint32_t mix(uint32_t h) {  // murmur3's finalizer
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}
struct Key {
  int32_t x, y, z;
};
__device__ __forceinline__ bool same(const Key &a, const Key &b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
__device__ __forceinline__ uint32_t hash(const Key &k) {
  return mix((uint32_t)k.x * 0x9e3779b1u ^ mix((uint32_t)k.y * 0x85ebca77u ^ mix((uint32_t)k.z * 0xc2b2ae3du)));
}

__device__ __forceinline__ bool clusterable(float x, float y, float z) {  // finite and below the limit (NaN fails the comparison)
  return fabsf(x) < kCoordLimit && fabsf(y) < kCoordLimit && fabsf(z) < kCoordLimit;
}
// the cell of a clusterable vertex: |v| < 2^16 and cell >= 2^-10, so |q| <= 2^26
__device__ __forceinline__ Key cell_of(const float *__restrict__ verts, int64_t i, double cell) {
  return Key{(int32_t)floor((double)verts[i * 3 + 0] / cell), (int32_t)floor((double)verts[i * 3 + 1] / cell),
             (int32_t)floor((double)verts[i * 3 + 2] / cell)};
}
struct VertexKeys {
  const float *verts;
  double cell;
  __device__ __forceinline__ Key operator()(int32_t i) const { return cell_of(verts, i, cell); }
};

// (a, b, c) rotated so that its smallest number comes first; the three differ
__device__ __forceinline__ Key canonical(int32_t a, int32_t b, int32_t c) {
  if (a < b && a < c) return Key{a, b, c};
  if (b < a && b < c) return Key{b, c, a};
  return Key{c, a, b};
}
// of a face that was inserted: valid and not degenerate, so its indices address root_of and its roots are no -1
struct FaceKeys {
  const int32_t *faces, *root_of;
  __device__ __forceinline__ Key operator()(int32_t f) const {
    return canonical(root_of[faces[(int64_t)f * 3 + 0]], root_of[faces[(int64_t)f * 3 + 1]], root_of[faces[(int64_t)f * 3 + 2]]);
  }
};

// -> the slot of i's class, or false after `slots` steps without an empty slot or an equal key (cannot happen: see above)
template <class Keys>
__device__ __forceinline__ bool insert(int32_t *table, uint32_t mask, int32_t i, const Key &mine, const Keys &key_of, uint32_t *slot_out) {
  uint32_t h = hash(mine) & mask;
  for (uint64_t step = 0; step <= (uint64_t)mask; ++step, h = (h + 1) & mask) {
    int32_t holder = __hip_atomic_load(table + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (holder == kEmpty) {
      holder = atomicCAS(table + h, kEmpty, i);
      if (holder == kEmpty) {
        *slot_out = h;
        return true;
      }
    }
    if (same(key_of(holder), mine)) {
      atomicMin(table + h, i);
      *slot_out = h;
      return true;
    }
  }
  return false;
}

__global__ __launch_bounds__(kBlock) void ms_fill_kernel(int32_t *__restrict__ vtable, int64_t vslots, int32_t *__restrict__ ftable,
                                                         int64_t fslots, int32_t *__restrict__ error) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < vslots) vtable[i] = kEmpty;
  if (i < fslots) ftable[i] = kEmpty;
  if (i == 0) *error = 0;
}

// the vertices that belong to no cluster; the wave adds its number once.  Every lane of the wave calls it.
__device__ __forceinline__ void count_bad(bool bad, unsigned long long *total) {
  const unsigned long long m = __ballot(bad);
  if (m != 0 && (threadIdx.x & 63) == 0) atomicAdd(total, (unsigned long long)__popcll(m));
}

// V == 0 or F == 0: nothing is clustered, `bad` is still counted
__global__ __launch_bounds__(kBlock) void ms_count_bad_kernel(const float *__restrict__ verts, int64_t V, unsigned long long *__restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  count_bad(i < V && !clusterable(verts[i * 3 + 0], verts[i * 3 + 1], verts[i * 3 + 2]), bad);
}

// root_of[i] = -1 marks a vertex of no cluster from here on (the root kernel replaces the 0 of the others)
__global__ __launch_bounds__(kBlock) void ms_vertex_insert_kernel(const float *__restrict__ verts, int64_t V, double cell, int32_t *table,
                                                                  uint32_t mask, uint32_t *__restrict__ slot_of, int32_t *__restrict__ root_of,
                                                                  unsigned long long *__restrict__ bad, int32_t *__restrict__ error) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool mine = i < V;
  const bool ok = mine && clusterable(verts[i * 3 + 0], verts[i * 3 + 1], verts[i * 3 + 2]);
  count_bad(mine && !ok, bad);
  if (!mine) return;
  bool placed = false;
  if (ok) {
    uint32_t slot = 0;
    placed = insert(table, mask, (int32_t)i, cell_of(verts, i, cell), VertexKeys{verts, cell}, &slot);
    if (placed) slot_of[i] = slot;
    else *error = 1;
  }
  root_of[i] = placed ? 0 : -1;
}

__global__ __launch_bounds__(kBlock) void ms_vertex_root_kernel(const int32_t *__restrict__ table, const uint32_t *__restrict__ slot_of, int64_t V,
                                                                int32_t *__restrict__ root_of, long long *__restrict__ sums,
                                                                int32_t *__restrict__ used) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= V) return;
  used[i] = 0;
  if (root_of[i] < 0) return;
  const int32_t r = table[slot_of[i]];
  root_of[i] = r;
  if (r == (int32_t)i) {
    sums[i * 4 + 0] = 0;
    sums[i * 4 + 1] = 0;
    sums[i * 4 + 2] = 0;
    sums[i * 4 + 3] = 0;
  }
}

// ---- sums ----------------------------------------------------------------------------------------------------------------
struct Sums {
  long long x, y, z, n;
};
__device__ __forceinline__ void publish(long long *row, const Sums &s) {
  atomicAdd((unsigned long long *)row + 0, (unsigned long long)s.x);  // two's complement: the signed sum, in any order
  atomicAdd((unsigned long long *)row + 1, (unsigned long long)s.y);
  atomicAdd((unsigned long long *)row + 2, (unsigned long long)s.z);
  atomicAdd((unsigned long long *)row + 3, (unsigned long long)s.n);
}
__device__ __forceinline__ long long shfl_xor64(long long v, int o) {
  const int lo = __shfl_xor((int)(uint32_t)(unsigned long long)v, o), hi = __shfl_xor((int)((unsigned long long)v >> 32), o);
  return (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
}
// the whole wave calls it: folds the lanes' sums, the first lane publishes them to the row of `root`, `s` is empty afterwards
__device__ __forceinline__ void flush(long long *sums, int32_t root, Sums &s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s.x += shfl_xor64(s.x, o);
    s.y += shfl_xor64(s.y, o);
    s.z += shfl_xor64(s.z, o);
    s.n += shfl_xor64(s.n, o);
  }
  if ((threadIdx.x & 63) == 0 && s.n) publish(sums + (int64_t)root * 4, s);
  s = Sums{0, 0, 0, 0};
}
// s_a = rint(v_a 2^16), ties to even; the product is exact (a power of two) and |s_a| < 2^32
__device__ __forceinline__ long long fixed(float v) { return (long long)rint((double)v * kFixed); }

// kPerThread vertices per thread, as mcc_vertex_stats_kernel sweeps them.  Marching cubes emits vertices in lattice order, so a
// wave's 64 consecutive vertices mostly lie in one cell: while every vertex the wave meets has the same root, each lane keeps
// its sums in registers; the wave folds them and its first lane issues the four atomics when the root changes and at the end.
// A sweep in which the wave's roots differ publishes per lane.  Integer sums: the same bits either way.
__global__ __launch_bounds__(kBlock) void ms_sums_kernel(const float *__restrict__ verts, const int32_t *__restrict__ root_of, int64_t V,
                                                         long long *__restrict__ sums, int uniform_path) {
  const int64_t base = (int64_t)blockIdx.x * (kBlock * kPerThread) + threadIdx.x;
  Sums acc{0, 0, 0, 0};
  int32_t acc_root = -1;  // the same in every lane of the wave; -1: acc is empty
  for (int j = 0; j < kPerThread; ++j) {
    const int64_t i = base + (int64_t)j * kBlock;
    int32_t r = -1;
    if (i < V) r = root_of[i];
    const bool live = r >= 0 && (int64_t)r < V;  // a root that is no row must not become an address
    Sums mine{0, 0, 0, 0};
    if (live) mine = Sums{fixed(verts[i * 3 + 0]), fixed(verts[i * 3 + 1]), fixed(verts[i * 3 + 2]), 1};
    const unsigned long long alive = __ballot(live);
    if (alive == 0) continue;  // the same for the whole wave
    const int32_t r0 = __shfl(r, __ffsll((long long)alive) - 1);
    if (uniform_path && __all(!live || r == r0)) {
      if (acc_root != r0) {
        if (acc_root >= 0) flush(sums, acc_root, acc);
        acc_root = r0;
      }
      acc.x += mine.x;
      acc.y += mine.y;
      acc.z += mine.z;
      acc.n += mine.n;
    } else {
      if (acc_root >= 0) flush(sums, acc_root, acc);
      acc_root = -1;
      if (live) publish(sums + (int64_t)r * 4, mine);
    }
  }
  if (acc_root >= 0) flush(sums, acc_root, acc);
}

// ---- faces ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool in_range(int32_t a, int32_t b, int32_t c, int64_t V) {
  return a >= 0 && b >= 0 && c >= 0 && (int64_t)a < V && (int64_t)b < V && (int64_t)c < V;
}
// the three roots of a valid face, or false; an index that is no vertex must not become an address
__device__ __forceinline__ bool face_roots(const int32_t *__restrict__ faces, int64_t f, int64_t V, const int32_t *__restrict__ root_of,
                                           int32_t *ra, int32_t *rb, int32_t *rc) {
  const int32_t a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  if (!in_range(a, b, c, V)) return false;
  *ra = root_of[a];
  *rb = root_of[b];
  *rc = root_of[c];
  return *ra >= 0 && *rb >= 0 && *rc >= 0;
}

// keep[f] = 0: invalid, degenerate (or given up); 1: inserted, ms_face_keep_kernel decides
__global__ __launch_bounds__(kBlock) void ms_face_insert_kernel(const int32_t *__restrict__ faces, int64_t F, int64_t V,
                                                                const int32_t *__restrict__ root_of, int32_t *table, uint32_t mask,
                                                                uint32_t *__restrict__ slot_of, int32_t *__restrict__ keep,
                                                                int32_t *__restrict__ error) {
  const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F) return;
  int32_t ra, rb, rc;
  bool placed = false;
  if (face_roots(faces, f, V, root_of, &ra, &rb, &rc) && ra != rb && rb != rc && rc != ra) {
    uint32_t slot = 0;
    placed = insert(table, mask, (int32_t)f, canonical(ra, rb, rc), FaceKeys{faces, root_of}, &slot);
    if (placed) slot_of[f] = slot;
    else *error = 1;
  }
  keep[f] = placed;
}

// the stores to `used` all write 1 (the root kernel zeroed it)
__global__ __launch_bounds__(kBlock) void ms_face_keep_kernel(const int32_t *__restrict__ faces, int64_t F, int64_t V,
                                                              const int32_t *__restrict__ root_of, const int32_t *__restrict__ table,
                                                              const uint32_t *__restrict__ slot_of, int32_t *__restrict__ keep,
                                                              int32_t *__restrict__ used) {
  const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (f >= F || !keep[f]) return;
  if (table[slot_of[f]] != (int32_t)f) {  // a duplicate of an earlier face
    keep[f] = 0;
    return;
  }
  int32_t ra, rb, rc;
  if (!face_roots(faces, f, V, root_of, &ra, &rb, &rc)) return;  // an inserted face is valid; the test is what bounds the stores
  used[ra] = 1;
  used[rb] = 1;
  used[rc] = 1;
}

__global__ void ms_totals_kernel(const int32_t *__restrict__ used, const int32_t *__restrict__ used_off, int64_t V,
                                 const int32_t *__restrict__ keep, const int32_t *__restrict__ keep_off, int64_t F,
                                 const int32_t *__restrict__ error, long long *__restrict__ totals) {
  if (*error) {
    totals[0] = totals[1] = totals[2] = SVR_E_INTERNAL;
    return;
  }
  totals[0] = (long long)used_off[V - 1] + used[V - 1];
  totals[1] = (long long)keep_off[F - 1] + keep[F - 1];
}

// one grid over max(V, F): thread i writes vertex_cluster[i], the output vertex of the cluster whose root i is, and face i
__global__ __launch_bounds__(kBlock) void ms_emit_kernel(const uint32_t *__restrict__ verts, int64_t V, const int32_t *__restrict__ faces,
                                                         int64_t F, const int32_t *__restrict__ root_of, const long long *__restrict__ sums,
                                                         const int32_t *__restrict__ used, const int32_t *__restrict__ used_off,
                                                         const int32_t *__restrict__ keep, const int32_t *__restrict__ keep_off,
                                                         const int32_t *__restrict__ error, uint32_t *__restrict__ out_verts,
                                                         int32_t *__restrict__ out_faces, int32_t *__restrict__ vertex_cluster,
                                                         int32_t *__restrict__ cluster_size) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool failed = *error != 0;  // the totals said so and sized no outputs: only vertex_cluster (V) is written
  if (i < V) {
    const int32_t r = root_of[i];
    const bool kept = !failed && r >= 0 && (int64_t)r < V && used[r];
    vertex_cluster[i] = kept ? used_off[r] : -1;
    if (kept && r == (int32_t)i) {
      const int64_t j = used_off[i];
      const long long n = sums[i * 4 + 3];
      cluster_size[j] = (int32_t)n;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        uint32_t word = verts[i * 3 + k];  // n == 1: the vertex's own words
        if (n != 1) word = __float_as_uint((float)(((double)sums[i * 4 + k] / (double)n) / kFixed));
        out_verts[j * 3 + k] = word;
      }
    }
  }
  if (i < F && !failed && keep[i]) {
    int32_t ra, rb, rc;
    if (!face_roots(faces, i, V, root_of, &ra, &rb, &rc)) return;  // a kept face is valid; the test is what bounds the loads
    const int64_t j = keep_off[i];
    out_faces[j * 3 + 0] = used_off[ra];
    out_faces[j * 3 + 1] = used_off[rb];
    out_faces[j * 3 + 2] = used_off[rc];
  }
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 0 && V < (1LL << 31) && F >= 0 && F < (1LL << 31); }
size_t scan_temp(int64_t n) { return n > 0 ? scan_sum_excl_i32_temp_bytes(n) : 0; }
// 2^k >= 2 n slots, at least 64: at most 2^32 for n < 2^31
int64_t slots_for(int64_t n) {
  int64_t s = 64;
  while (s < 2 * n) s <<= 1;
  return s;
}

// The one layout: count fills it, emit reads it.  Per vertex: its slot, its root (-1: no cluster), and by root index the `used`
// flag, its scan and the row of four int64 sums; per face: its slot, the keep flag and its scan; the two tables; one temp
// piece serves the vertex scan and the face scan; the error word has a line of its own.
struct SimplifyWs {
  long long *sums;
  uint32_t *vslot;
  int32_t *root_of, *used, *used_off;
  uint32_t *fslot;
  int32_t *keep, *keep_off, *vtable, *ftable;
  char *tmp;
  int32_t *error;
  int64_t vslots, fslots;
  size_t vertex_tmp_bytes, face_tmp_bytes;
};
SimplifyWs simplify_layout(WsCursor &c, int64_t V, int64_t F) {
  const int64_t vs = slots_for(V), fs = slots_for(F);
  const size_t tv = scan_temp(V), tf = scan_temp(F);
  return {c.take<long long>(4 * V), c.take<uint32_t>(V), c.take<int32_t>(V), c.take<int32_t>(V), c.take<int32_t>(V),
          c.take<uint32_t>(F),      c.take<int32_t>(F),  c.take<int32_t>(F), c.take<int32_t>(vs), c.take<int32_t>(fs),
          c.take<char>((int64_t)std::max(tv, tf)), c.take<int32_t>(1), vs, fs, tv, tf};
}

unsigned blocks(int64_t n) { return (unsigned)cdiv(n, kBlock); }

}  // namespace

extern "C" int64_t svr_mesh_simplify_workspace_bytes(int64_t V, int64_t F) {
  SVR_CHECK(sizes_ok(V, F), SVR_E_BADSHAPE, "mesh_simplify_workspace_bytes: V=%ld F=%ld (need 0 <= V, F < 2^31)", (long)V, (long)F);
  return ws_measure(simplify_layout, V, F);
}

extern "C" int svr_mesh_simplify_count(const float *verts, int64_t V, const int32_t *faces, int64_t F, float cell, void *ws, int64_t ws_bytes,
                                       int32_t uniform_path, int64_t *totals, void *stream) {
  SVR_CHECK(sizes_ok(V, F), SVR_E_BADSHAPE, "mesh_simplify_count: V=%ld F=%ld (need 0 <= V, F < 2^31)", (long)V, (long)F);
  // written so that a NaN fails it
  SVR_CHECK(cell >= 0.0009765625f && cell <= 65536.0f, SVR_E_BADARG, "mesh_simplify_count: cell=%g (need 2^-10 <= cell <= 2^16)", (double)cell);
  SVR_CHECK(totals, SVR_E_BADARG, "mesh_simplify_count: null totals");
  SVR_CHECK(V == 0 || verts, SVR_E_BADARG, "mesh_simplify_count: null verts");
  const bool empty = V == 0 || F == 0;  // no valid face: nothing is kept
  SimplifyWs w{};
  if (!empty) {
    SVR_CHECK(faces && ws, SVR_E_BADARG, "mesh_simplify_count: null pointer");
    WsCursor c(ws);
    w = simplify_layout(c, V, F);
    SVR_CHECK(ws_bytes >= c.bytes(), SVR_E_BADARG, "mesh_simplify_count: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)c.bytes());
  }
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(totals, 0, 3 * sizeof(int64_t), s);
  SVR_CHECK(e == hipSuccess, (int)e, "mesh_simplify_count: memset failed: %s", hipGetErrorString(e));
  unsigned long long *bad = (unsigned long long *)totals + 2;
  if (empty) {
    if (V > 0) hipLaunchKernelGGL(ms_count_bad_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, verts, V, bad);
    return launch_status("mesh_simplify_count");
  }
  const uint32_t vmask = (uint32_t)(w.vslots - 1), fmask = (uint32_t)(w.fslots - 1);
  hipLaunchKernelGGL(ms_fill_kernel, dim3(blocks(std::max(w.vslots, w.fslots))), dim3(kBlock), 0, s, w.vtable, w.vslots, w.ftable, w.fslots,
                     w.error);
  hipLaunchKernelGGL(ms_vertex_insert_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, verts, V, (double)cell, w.vtable, vmask, w.vslot, w.root_of,
                     bad, w.error);
  hipLaunchKernelGGL(ms_vertex_root_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, w.vtable, w.vslot, V, w.root_of, w.sums, w.used);
  hipLaunchKernelGGL(ms_sums_kernel, dim3(blocks(cdiv(V, kPerThread))), dim3(kBlock), 0, s, verts, w.root_of, V, w.sums,
                     (int)(uniform_path != 0));
  hipLaunchKernelGGL(ms_face_insert_kernel, dim3(blocks(F)), dim3(kBlock), 0, s, faces, F, V, w.root_of, w.ftable, fmask, w.fslot, w.keep,
                     w.error);
  hipLaunchKernelGGL(ms_face_keep_kernel, dim3(blocks(F)), dim3(kBlock), 0, s, faces, F, V, w.root_of, w.ftable, w.fslot, w.keep, w.used);
  if (int rc = launch_status("mesh_simplify_count")) return rc;
  e = scan_sum_excl_i32(w.tmp, w.vertex_tmp_bytes, w.used, w.used_off, V, s);
  if (e == hipSuccess) e = scan_sum_excl_i32(w.tmp, w.face_tmp_bytes, w.keep, w.keep_off, F, s);
  SVR_CHECK(e == hipSuccess, (int)e, "mesh_simplify_count: scan failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(ms_totals_kernel, dim3(1), dim3(1), 0, s, w.used, w.used_off, V, w.keep, w.keep_off, F, w.error, (long long *)totals);
  return launch_status("mesh_simplify_totals");
}

extern "C" int svr_mesh_simplify_emit(const float *verts, int64_t V, const int32_t *faces, int64_t F, void *ws, int64_t ws_bytes,
                                      float *out_verts, int32_t *out_faces, int32_t *vertex_cluster, int32_t *cluster_size, void *stream) {
  SVR_CHECK(sizes_ok(V, F), SVR_E_BADSHAPE, "mesh_simplify_emit: V=%ld F=%ld (need 0 <= V, F < 2^31)", (long)V, (long)F);
  if (V == 0) return SVR_OK;
  SVR_CHECK(vertex_cluster, SVR_E_BADARG, "mesh_simplify_emit: null vertex_cluster");
  const hipStream_t s = (hipStream_t)stream;
  if (F == 0) {  // nothing was clustered
    const hipError_t e = hipMemsetAsync(vertex_cluster, 0xff, (size_t)V * 4, s);
    SVR_CHECK(e == hipSuccess, (int)e, "mesh_simplify_emit: memset failed: %s", hipGetErrorString(e));
    return SVR_OK;
  }
  // out_verts / out_faces / cluster_size may be null when the totals were 0: nothing is written through them then
  SVR_CHECK(verts && faces && ws, SVR_E_BADARG, "mesh_simplify_emit: null pointer");
  WsCursor c(ws);
  const SimplifyWs w = simplify_layout(c, V, F);
  SVR_CHECK(ws_bytes >= c.bytes(), SVR_E_BADARG, "mesh_simplify_emit: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)c.bytes());
  hipLaunchKernelGGL(ms_emit_kernel, dim3(blocks(std::max(V, F))), dim3(kBlock), 0, s, (const uint32_t *)verts, V, faces, F, w.root_of, w.sums,
                     w.used, w.used_off, w.keep, w.keep_off, w.error, (uint32_t *)out_verts, out_faces, vertex_cluster, cluster_size);
  return launch_status("mesh_simplify_emit");
}
