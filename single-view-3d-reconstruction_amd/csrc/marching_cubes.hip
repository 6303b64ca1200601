// On-device marching cubes (gfx950): dense float32 field -> welded, indexed triangle mesh.
//
// Replaces the reference's marching_cubes.marching_cubes(sdf.astype(float), level) + export_obj in util/visualize.py:23-25,
// called by implicit_to_mesh (model/ifnet.py:232-234) and the trainers' validation / visualisation steps.  The reference
// copies the whole lattice to the host first; here only the mesh leaves the device.
//
// Semantics (pinned bit for bit by tests/test_gpu_marching_cubes.py against the numpy oracle of tests/mc_oracle.py):
//   - point inside iff (double)v < level (NaN: outside); cells (i, j, k) with i < X-1, j < Y-1, k < Z-1;
//   - one vertex per crossing lattice edge, owned by its lower endpoint p, placed at
//     (float)((double)p_axis + fmin(fmax((level - a) / (b - a), 0), 1)) in float64 (a at p, b at p + e_axis);
//   - vertices ordered by owner point (C order), then axis; faces by cell (C order of its minimum corner), then table order;
//   - case table from mc_table.h: normals point from inside to outside.
//
// Three steps: classify (one thread per point: owned crossing edges, cell case, packed count nv | nt << 32, exact totals by
// block atomics), one exclusive rocPRIM scan of the packed counts (sort.hip), emit (one thread per point: its vertices, its
// cell's triangles; a triangle's edge resolves to (owner point, axis) -> owner's vertex offset + popcount of its lower
// owned-edge bits).  The caller reads the two totals back (the only host synchronisation) to size the outputs.  While
// V < 2^31 and F < 2^31 neither 32-bit half of the scan can carry into the other.
#include "common.h"
#include "mc_table.h"
#include "reduce.h"
#include <algorithm>
#include <cmath>

using namespace svr;

namespace {

constexpr mc::CaseTable kHostTable = mc::build_case_table();
__constant__ mc::CaseTable kCaseTable = mc::build_case_table();

constexpr int kBlock = 256;
constexpr int kClassifyBlocks = 2048;  // grid-stride: one pair of totals atomics per block

struct Lattice {
  int32_t X, Y, Z;
  int64_t sx, sy;  // strides of axes 0 and 1 (axis 2: 1)
  int64_t n;
};

__device__ __forceinline__ void decompose(const Lattice &L, uint32_t p, uint32_t &i, uint32_t &j, uint32_t &k) {
  i = p / (uint32_t)L.sx;
  const uint32_t r = p - i * (uint32_t)L.sx;
  j = r / (uint32_t)L.Z;
  k = r - j * (uint32_t)L.Z;
}

__device__ __forceinline__ uint32_t inside(const float *__restrict__ f, int64_t q, double level) {
  return (double)f[q] < level ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void mc_classify_kernel(const float *__restrict__ field, Lattice L, double level,
                                                             uint64_t *__restrict__ counts, uint16_t *__restrict__ flags,
                                                             unsigned long long *__restrict__ totals) {
  uint32_t nv_sum = 0, nt_sum = 0;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < L.n; p += (int64_t)gridDim.x * kBlock) {
    uint32_t i, j, k;
    decompose(L, (uint32_t)p, i, j, k);
    const bool hx = (int32_t)i + 1 < L.X, hy = (int32_t)j + 1 < L.Y, hz = (int32_t)k + 1 < L.Z;
    uint32_t cs = inside(field, p, level);
    if (hx) cs |= inside(field, p + L.sx, level) << 1;
    if (hy) cs |= inside(field, p + L.sy, level) << 2;
    if (hz) cs |= inside(field, p + 1, level) << 4;
    const uint32_t b0 = cs & 1u;
    const uint32_t edges = (uint32_t)(hx && ((cs >> 1) & 1u) != b0) | (uint32_t)(hy && ((cs >> 2) & 1u) != b0) << 1 |
                           (uint32_t)(hz && ((cs >> 4) & 1u) != b0) << 2;
    uint32_t nt = 0;
    if (hx && hy && hz) {
      cs |= inside(field, p + L.sx + L.sy, level) << 3 | inside(field, p + L.sx + 1, level) << 5 |
            inside(field, p + L.sy + 1, level) << 6 | inside(field, p + L.sx + L.sy + 1, level) << 7;
      nt = (uint32_t)kCaseTable.ntri[cs];
    } else {
      cs = 0;  // not a cell's minimum corner: no triangles
    }
    const uint32_t nv = __popc(edges);
    counts[p] = (uint64_t)nv | (uint64_t)nt << 32;
    flags[p] = (uint16_t)(cs | edges << 8);
    nv_sum += nv;
    nt_sum += nt;
  }
  __shared__ uint64_t part[2][kBlock / 64];
  block_add_totals_u64<kBlock>(nv_sum, nt_sum, part, totals);
}

__global__ __launch_bounds__(kBlock) void mc_emit_kernel(const float *__restrict__ field, Lattice L, double level,
                                                         const uint64_t *__restrict__ offs, const uint16_t *__restrict__ flags,
                                                         float *__restrict__ verts, int32_t *__restrict__ faces) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= L.n) return;
  const uint32_t fl = flags[p];
  if (fl == 0) return;
  const uint64_t off = offs[p];
  const uint32_t edges = fl >> 8;
  if (edges) {
    uint32_t i, j, k;
    decompose(L, (uint32_t)p, i, j, k);
    const double a = (double)field[p];
    uint32_t vid = (uint32_t)off;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      if (!((edges >> ax) & 1u)) continue;
      const double b = (double)field[p + (ax == 0 ? L.sx : ax == 1 ? L.sy : 1)];
      const double t = fmin(fmax((level - a) / (b - a), 0.0), 1.0);  // NaN t -> 0
      float c[3] = {(float)i, (float)j, (float)k};
      c[ax] = (float)((double)(ax == 0 ? i : ax == 1 ? j : k) + t);
      float *o = verts + (int64_t)vid * 3;
      o[0] = c[0];
      o[1] = c[1];
      o[2] = c[2];
      ++vid;
    }
  }
  const uint32_t cs = fl & 0xffu;
  const int nt = kCaseTable.ntri[cs];
  int32_t *o = faces + (int64_t)(uint32_t)(off >> 32) * 3;
  for (int m = 0; m < nt * 3; ++m) {
    const int e = kCaseTable.edge[cs][m];
    const int ax = e >> 2;
    // the edge's offsets along the two other axes u < v pick its owner point inside the cell
    const int64_t su = ax == 0 ? L.sy : L.sx, sv = ax == 2 ? L.sy : 1;
    const int64_t q = p + (e & 1) * su + ((e >> 1) & 1) * sv;
    o[m] = (int32_t)((uint32_t)offs[q] + __popc(((uint32_t)flags[q] >> 8) & ((1u << ax) - 1u)));
  }
}


bool lattice(int32_t X, int32_t Y, int32_t Z, Lattice &L) {
  if (X < 0 || Y < 0 || Z < 0) return false;
  L.X = X;
  L.Y = Y;
  L.Z = Z;
  L.sy = Z;
  L.sx = (int64_t)Y * Z;
  L.n = (int64_t)X * Y * Z;
  return L.n < (1LL << 31);
}

bool empty(const Lattice &L) { return L.X < 2 || L.Y < 2 || L.Z < 2; }

struct Ws {
  uint64_t *counts, *offs;
  uint16_t *flags;
  void *tmp;
  size_t tmp_bytes;
};

Ws ws_layout(WsCursor &c, int64_t n) {   // the launchers have always used the caller's pointer as it is: base alignment 1
  const size_t tmp_bytes = scan_sum_excl_u64_temp_bytes(n);
  return {c.take<uint64_t>(n), c.take<uint64_t>(n), c.take<uint16_t>(n), c.take<char>((int64_t)tmp_bytes), tmp_bytes};
}

}  // namespace

extern "C" int64_t svr_mc_workspace_bytes(int32_t X, int32_t Y, int32_t Z) {
  Lattice L;
  if (!lattice(X, Y, Z, L)) {
    set_error("mc_workspace_bytes: bad lattice %d x %d x %d", X, Y, Z);
    return SVR_E_BADSHAPE;
  }
  if (empty(L)) return 256;
  return ws_measure(ws_layout, L.n);
}

extern "C" int svr_mc_count(const float *field, int32_t X, int32_t Y, int32_t Z, double level, void *ws, int64_t ws_bytes,
                            int64_t *totals, void *stream) {
  Lattice L;
  SVR_CHECK(lattice(X, Y, Z, L), SVR_E_BADSHAPE, "mc_count: bad lattice %d x %d x %d (fewer than 2^31 points)", X, Y, Z);
  SVR_CHECK(totals, SVR_E_BADARG, "mc_count: null totals");
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s);
  SVR_CHECK(e == hipSuccess, (int)e, "mc_count: memset failed: %s", hipGetErrorString(e));
  if (empty(L)) return SVR_OK;
  SVR_CHECK(field && ws, SVR_E_BADARG, "mc_count: null pointer");
  WsCursor c(ws, 1);
  const Ws w = ws_layout(c, L.n);
  SVR_CHECK(ws_bytes >= c.bytes(), SVR_E_BADARG, "mc_count: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)c.bytes());
  const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(L.n, kBlock), kClassifyBlocks);
  hipLaunchKernelGGL(mc_classify_kernel, dim3(blocks), dim3(kBlock), 0, s, field, L, level, w.counts, w.flags,
                     (unsigned long long *)totals);
  int rc = launch_status("mc_classify");
  if (rc) return rc;
  e = scan_sum_excl_u64(w.tmp, w.tmp_bytes, w.counts, w.offs, L.n, s);
  SVR_CHECK(e == hipSuccess, (int)e, "mc_count: scan failed: %s", hipGetErrorString(e));
  return launch_status("mc_scan");
}

extern "C" int svr_mc_emit(const float *field, int32_t X, int32_t Y, int32_t Z, double level, void *ws, float *verts,
                           int32_t *faces, void *stream) {
  Lattice L;
  SVR_CHECK(lattice(X, Y, Z, L), SVR_E_BADSHAPE, "mc_emit: bad lattice %d x %d x %d (fewer than 2^31 points)", X, Y, Z);
  if (empty(L)) return SVR_OK;
  SVR_CHECK(field && ws, SVR_E_BADARG, "mc_emit: null pointer");
  WsCursor c(ws, 1);
  const Ws w = ws_layout(c, L.n);
  hipLaunchKernelGGL(mc_emit_kernel, dim3((unsigned)cdiv(L.n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, field, L, level,
                     w.offs, w.flags, verts, faces);
  return launch_status("mc_emit");
}

extern "C" int svr_mc_case_table(int8_t *out) {
  SVR_CHECK(out, SVR_E_BADARG, "mc_case_table: null pointer");
  for (int c = 0; c < 256; ++c)
    for (int m = 0; m < 16; ++m) out[c * 16 + m] = kHostTable.edge[c][m];
  return SVR_OK;
}
