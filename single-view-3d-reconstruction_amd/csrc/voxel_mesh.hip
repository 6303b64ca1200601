// Stage visualisation of the scene trainer, device side (gfx950): the voxel-box mesher behind visualize_grid and the two
// image planes behind visualize_depthmap (the .png and point-list .obj writers are io_png.cpp and io_mesh.cpp).
//
// Replaces the reference's util/visualize.py:10-20,28-49 (to_point_list + trimesh.voxel.ops.multibox + Trimesh's vertex
// merge + export; numpy + PIL + pyexr for the depth map), called by SceneNetTrainer.visualize_intermediates
// (trainer/trainer_scene_net.py:170-188).  The reference copies the 139 x 104 x 112 grid to the host first; here only
// the mesh and the two image planes leave the device.
//
// Voxel-box mesher.  Semantics (pinned bit for bit by tests/test_gpu_voxel_mesh.py against tests/voxel_mesh_oracle.py):
//   - voxel (i, j, k) of the (X, Y, Z) lattice is occupied iff (double)v >= threshold (NaN: not occupied); it is the cube
//     [i-1/2, i+1/2] x [j-1/2, j+1/2] x [k-1/2, k+1/2] (pitch 1, x along axis 0: the index space of marching_cubes.hip);
//   - a cube face is emitted iff the voxel across it is unoccupied or outside the lattice: the boundary surface of the
//     union of the boxes.  (multibox emits all 12 triangles of every box; the faces shared by two boxes are dropped here);
//   - vertices are points (a, b, c) of the (X+1)(Y+1)(Z+1) corner lattice, at (a-1/2, b-1/2, c-1/2); a corner is emitted,
//     once, iff the 2 x 2 x 2 voxels around it (outside = empty) are neither all empty nor all occupied, which is exactly
//     "some emitted face touches it"; vertices are ordered by the corner's C-order index;
//   - faces are ordered by voxel (C order), then direction -x, +x, -y, +y, -z, +z.  Each is a quad q0 q1 q2 q3, counter-
//     clockwise seen from outside, split along q0-q2 into the triangles (q0, q1, q2), (q0, q2, q3).  With (d, u, v) the
//     cyclic axis triple of the face's axis d -- (x, y, z), (y, z, x), (z, x, y) -- and corner offsets in {0, 1} from the
//     voxel's minimum corner (i, j, k):
//         +d face: d = 1, (u, v) = (0,0) (1,0) (1,1) (0,1)        -d face: d = 0, (u, v) = (0,0) (0,1) (1,1) (1,0)
//     spelled out as (x y z) offsets:   -x: 000 001 011 010    +x: 100 110 111 101    -y: 000 100 101 001
//                                       +y: 010 011 111 110    -z: 000 010 110 100    +z: 001 101 111 011
//
// Three steps, the shape of marching_cubes.hip: classify (one thread per corner-lattice point p = (a, b, c): its vertex
// bit from a gather of the 8 voxels around it, and -- p being the minimum corner of voxel (a, b, c) when a < X, b < Y,
// c < Z -- that voxel's exposed-face mask; packed count nv | nt << 32 with nt = 2 triangles per face; exact totals by one
// atomic pair per block), one exclusive rocPRIM scan of the packed counts (sort.hip), emit (one thread per point: its
// vertex, its voxel's triangles; a quad corner resolves to the scanned vertex offset of its corner-lattice point).  The
// corner-lattice C order of the minimum corners is the voxels' C order, so one scan orders both outputs.  No flag races,
// no float atomics: the result is deterministic.  The caller reads the two totals back (the only host synchronisation).
//
// Depth-map planes: depth_minmax (min, max and a non-finite flag of the map: order-independent integer atomics on the
// order-preserving bit pattern) and depth_planes (one pass: the optionally column-flipped float32 plane and the uint8
// plane (255.0f / max * (d - min)) truncated toward zero, every float32 operation rounded on its own, the arithmetic
// numpy 2 applies to a float32 array).
#include "common.h"
#include "reduce.h"
#include <algorithm>

using namespace svr;

namespace {

constexpr int kBlock = 256;
constexpr int kClassifyBlocks = 2048;  // grid-stride: one pair of totals atomics per block

constexpr uint32_t kVertexBit = 1u << 6;

struct Lattice {
  int32_t X, Y, Z;
  int64_t sx, sy;    // voxel strides of axes 0 and 1 (axis 2: 1)
  int64_t cx, cy;    // corner-lattice strides of axes 0 and 1
  int64_t n;         // corner-lattice points
};

__device__ __forceinline__ uint32_t occupied(const float *__restrict__ f, const Lattice &L, int i, int j, int k, double threshold) {
  if (i < 0 || j < 0 || k < 0 || i >= L.X || j >= L.Y || k >= L.Z) return 0u;
  return (double)f[i * L.sx + j * L.sy + k] >= threshold ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void vm_classify_kernel(const float *__restrict__ field, Lattice L, double threshold,
                                                             uint64_t *__restrict__ counts, uint8_t *__restrict__ flags,
                                                             unsigned long long *__restrict__ totals) {
  uint32_t nv_sum = 0, nt_sum = 0;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < L.n; p += (int64_t)gridDim.x * kBlock) {
    const int a = (int)((uint32_t)p / (uint32_t)L.cx);
    const uint32_t r = (uint32_t)p - (uint32_t)a * (uint32_t)L.cx;
    const int b = (int)(r / (uint32_t)L.cy);
    const int c = (int)(r - (uint32_t)b * (uint32_t)L.cy);
    // the 8 voxels around the corner: bit (dx << 2 | dy << 1 | dz) = voxel (a-1+dx, b-1+dy, c-1+dz)
    uint32_t nb = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) nb |= occupied(field, L, a - 1 + (m >> 2), b - 1 + ((m >> 1) & 1), c - 1 + (m & 1), threshold) << m;
    uint32_t fl = (nb != 0 && nb != 0xffu) ? kVertexBit : 0u;
    if (nb >> 7) {  // voxel (a, b, c) itself is occupied (so a < X, b < Y, c < Z)
      fl |= (((nb >> 3) & 1u) ^ 1u) | (occupied(field, L, a + 1, b, c, threshold) ^ 1u) << 1 | (((nb >> 5) & 1u) ^ 1u) << 2 |
            (occupied(field, L, a, b + 1, c, threshold) ^ 1u) << 3 | (((nb >> 6) & 1u) ^ 1u) << 4 |
            (occupied(field, L, a, b, c + 1, threshold) ^ 1u) << 5;
    }
    const uint32_t nv = fl >> 6, nt = 2u * __popc(fl & 63u);
    counts[p] = (uint64_t)nv | (uint64_t)nt << 32;
    flags[p] = (uint8_t)fl;
    nv_sum += nv;
    nt_sum += nt;
  }
  __shared__ uint64_t part[2][kBlock / 64];
  block_add_totals_u64<kBlock>(nv_sum, nt_sum, part, totals);
}

__global__ __launch_bounds__(kBlock) void vm_emit_kernel(Lattice L, const uint64_t *__restrict__ offs, const uint8_t *__restrict__ flags,
                                                         float *__restrict__ verts, int32_t *__restrict__ faces) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= L.n) return;
  const uint32_t fl = flags[p];
  if (fl == 0) return;
  const uint64_t off = offs[p];
  if (fl & kVertexBit) {
    const uint32_t a = (uint32_t)p / (uint32_t)L.cx;
    const uint32_t r = (uint32_t)p - a * (uint32_t)L.cx;
    const uint32_t b = r / (uint32_t)L.cy;
    const uint32_t c = r - b * (uint32_t)L.cy;
    float *o = verts + (int64_t)(uint32_t)off * 3;
    o[0] = (float)a - 0.5f;
    o[1] = (float)b - 0.5f;
    o[2] = (float)c - 0.5f;
  }
  if ((fl & 63u) == 0) return;
  // an exposed face only exists on an occupied voxel (a < X, b < Y, c < Z): its 8 corners are inside the corner lattice
  int32_t id[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) id[m] = (int32_t)(uint32_t)offs[p + (m >> 2) * L.cx + ((m >> 1) & 1) * L.cy + (m & 1)];
  int32_t *o = faces + (int64_t)(uint32_t)(off >> 32) * 3;
  // quad corners per direction (-x, +x, -y, +y, -z, +z) as x << 2 | y << 1 | z offsets from the voxel's minimum corner
  // (compile-time indices after unrolling: id[] stays in registers)
  constexpr uint8_t kQuad[6][4] = {{0, 1, 3, 2}, {4, 6, 7, 5}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 2, 6, 4}, {1, 5, 7, 3}};
#pragma unroll
  for (int d = 0; d < 6; ++d) {
    if (!((fl >> d) & 1u)) continue;
    const int32_t q0 = id[kQuad[d][0]], q1 = id[kQuad[d][1]], q2 = id[kQuad[d][2]], q3 = id[kQuad[d][3]];
    o[0] = q0;
    o[1] = q1;
    o[2] = q2;
    o[3] = q0;
    o[4] = q2;
    o[5] = q3;
    o += 6;
  }
}


bool lattice(int32_t X, int32_t Y, int32_t Z, Lattice &L) {
  if (X < 0 || Y < 0 || Z < 0) return false;
  L.X = X;
  L.Y = Y;
  L.Z = Z;
  L.sy = Z;
  L.sx = (int64_t)Y * Z;
  L.cy = (int64_t)Z + 1;
  L.cx = ((int64_t)Y + 1) * L.cy;  // <= 2^62
  if (L.cx >= (1LL << 31)) return false;
  L.n = ((int64_t)X + 1) * L.cx;   // < 2^62
  return L.n < (1LL << 31);
}

bool empty(const Lattice &L) { return L.X == 0 || L.Y == 0 || L.Z == 0; }

struct Ws {
  uint64_t *counts, *offs;
  uint8_t *flags;
  void *tmp;
  size_t tmp_bytes;
};

Ws ws_layout(WsCursor &c, int64_t n) {   // the launchers have always used the caller's pointer as it is: base alignment 1
  const size_t tmp_bytes = scan_sum_excl_u64_temp_bytes(n);
  return {c.take<uint64_t>(n), c.take<uint64_t>(n), c.take<uint8_t>(n), c.take<char>((int64_t)tmp_bytes), tmp_bytes};
}

// ---- depth-map planes ---------------------------------------------------------------------------------------------
// float bits -> unsigned key with the floats' order (negative: all bits flipped, else the sign bit set)
__device__ __forceinline__ uint32_t order_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }

// stats[0] = ~key(min), stats[1] = key(max) (both raised by atomicMax from 0), stats[2] = 1 if any value is not finite
__global__ __launch_bounds__(kBlock) void depth_minmax_kernel(const float *__restrict__ map, int64_t n, uint32_t *__restrict__ stats) {
  uint32_t inv_lo = 0, hi = 0, bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const float v = map[i];
    if (!(fabsf(v) <= 3.402823466e+38f)) {  // NaN, +-inf
      bad = 1;
      continue;
    }
    const uint32_t k = order_key(v);
    inv_lo = max(inv_lo, ~k);
    hi = max(hi, k);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    inv_lo = max(inv_lo, (uint32_t)__shfl_xor((int)inv_lo, o));
    hi = max(hi, (uint32_t)__shfl_xor((int)hi, o));
    bad |= (uint32_t)__shfl_xor((int)bad, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (inv_lo) atomicMax(&stats[0], inv_lo);
    if (hi) atomicMax(&stats[1], hi);
    if (bad) atomicOr(&stats[2], 1u);
  }
}

__global__ __launch_bounds__(kBlock) void depth_planes_kernel(const float *__restrict__ map, int H, int W, int flip,
                                                              const uint32_t *__restrict__ stats, float *__restrict__ plane_f32,
                                                              uint8_t *__restrict__ plane_u8) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (int64_t)H * W) return;
  const int row = (int)(i / W), col = (int)(i - (int64_t)row * W);
  const float d = map[(int64_t)row * W + (flip ? W - 1 - col : col)];
  const float lo = key_value(~stats[0]), hi = key_value(stats[1]);
  const float scale = 255.0f / hi;
  const float r = scale * (d - lo);
  plane_f32[i] = d;
  // truncation toward zero; a value past 255 (a negative minimum) keeps its low 8 bits, like numpy's cast on x86-64
  plane_u8[i] = (uint8_t)((int32_t)r & 0xff);
}

}  // namespace

extern "C" int64_t svr_voxel_mesh_workspace_bytes(int32_t X, int32_t Y, int32_t Z) {
  Lattice L;
  if (!lattice(X, Y, Z, L)) {
    set_error("voxel_mesh_workspace_bytes: bad lattice %d x %d x %d (corner lattice of fewer than 2^31 points)", X, Y, Z);
    return SVR_E_BADSHAPE;
  }
  if (empty(L)) return 256;
  return ws_measure(ws_layout, L.n);
}

extern "C" int svr_voxel_mesh_count(const float *field, int32_t X, int32_t Y, int32_t Z, double threshold, void *ws, int64_t ws_bytes,
                                    int64_t *totals, void *stream) {
  Lattice L;
  SVR_CHECK(lattice(X, Y, Z, L), SVR_E_BADSHAPE, "voxel_mesh_count: bad lattice %d x %d x %d (corner lattice of fewer than 2^31 points)",
            X, Y, Z);
  SVR_CHECK(totals, SVR_E_BADARG, "voxel_mesh_count: null totals");
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s);
  SVR_CHECK(e == hipSuccess, (int)e, "voxel_mesh_count: memset failed: %s", hipGetErrorString(e));
  if (empty(L)) return SVR_OK;
  SVR_CHECK(field && ws, SVR_E_BADARG, "voxel_mesh_count: null pointer");
  WsCursor c(ws, 1);
  const Ws w = ws_layout(c, L.n);
  SVR_CHECK(ws_bytes >= c.bytes(), SVR_E_BADARG, "voxel_mesh_count: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)c.bytes());
  const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(L.n, kBlock), kClassifyBlocks);
  hipLaunchKernelGGL(vm_classify_kernel, dim3(blocks), dim3(kBlock), 0, s, field, L, threshold, w.counts, w.flags,
                     (unsigned long long *)totals);
  int rc = launch_status("vm_classify");
  if (rc) return rc;
  e = scan_sum_excl_u64(w.tmp, w.tmp_bytes, w.counts, w.offs, L.n, s);
  SVR_CHECK(e == hipSuccess, (int)e, "voxel_mesh_count: scan failed: %s", hipGetErrorString(e));
  return launch_status("vm_scan");
}

extern "C" int svr_voxel_mesh_emit(const float *field, int32_t X, int32_t Y, int32_t Z, double threshold, void *ws, float *verts,
                                   int32_t *faces, void *stream) {
  (void)field;      // the flags of svr_voxel_mesh_count hold everything emit needs; kept for the svr_mc_emit calling shape
  (void)threshold;
  Lattice L;
  SVR_CHECK(lattice(X, Y, Z, L), SVR_E_BADSHAPE, "voxel_mesh_emit: bad lattice %d x %d x %d (corner lattice of fewer than 2^31 points)",
            X, Y, Z);
  if (empty(L)) return SVR_OK;
  SVR_CHECK(ws && verts && faces, SVR_E_BADARG, "voxel_mesh_emit: null pointer");
  WsCursor c(ws, 1);
  const Ws w = ws_layout(c, L.n);
  hipLaunchKernelGGL(vm_emit_kernel, dim3((unsigned)cdiv(L.n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, L, w.offs, w.flags, verts,
                     faces);
  return launch_status("vm_emit");
}

extern "C" int svr_depth_minmax(const float *map, int64_t n, uint32_t *stats, void *stream) {
  SVR_CHECK(map && stats, SVR_E_BADARG, "depth_minmax: null pointer");
  SVR_CHECK(n > 0 && n < (1LL << 31), SVR_E_BADSHAPE, "depth_minmax: %ld values", (long)n);
  const hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(stats, 0, 4 * sizeof(uint32_t), s);
  SVR_CHECK(e == hipSuccess, (int)e, "depth_minmax: memset failed: %s", hipGetErrorString(e));
  const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(n, kBlock), 1024);
  hipLaunchKernelGGL(depth_minmax_kernel, dim3(blocks), dim3(kBlock), 0, s, map, n, stats);
  return launch_status("depth_minmax");
}

extern "C" int svr_depth_planes(const float *map, int32_t H, int32_t W, int32_t flip, const uint32_t *stats, float *plane_f32,
                                uint8_t *plane_u8, void *stream) {
  SVR_CHECK(map && stats && plane_f32 && plane_u8, SVR_E_BADARG, "depth_planes: null pointer");
  SVR_CHECK(H > 0 && W > 0 && (int64_t)H * W < (1LL << 31), SVR_E_BADSHAPE, "depth_planes: map %d x %d", H, W);
  hipLaunchKernelGGL(depth_planes_kernel, dim3((unsigned)cdiv((int64_t)H * W, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, map, H, W,
                     flip ? 1 : 0, stats, plane_f32, plane_u8);
  return launch_status("depth_planes");
}
