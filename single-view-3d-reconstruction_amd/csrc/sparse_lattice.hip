// Block-sparse evaluation of an occupancy lattice (gfx950): the bookkeeping around the network queries.
//
// Not a reference op.  implicit_to_mesh evaluates the IF-Net at every lattice point although only points next to the
// iso-surface can influence the mesh.  Here the lattice is cut into blocks of s cells per axis; a coarse sub-lattice (the
// block corners) is evaluated first, all fine points only in blocks whose corners lie on both sides of the level, and the
// surface is then followed into neighbouring blocks until it no longer leaves the evaluated region (util/sparse_grid.py
// drives the rounds; the exact rule is in include/svr_hip.h and DESIGN.md section 15, restated in numpy by
// tests/sparse_lattice_oracle.py).  The (X, Y, Z) field stays dense and goes to svr_mc_count / svr_mc_emit unchanged.
//
// The kernels never compute a coordinate: they copy entries of the three axis tables (the linspace tensors make_3d_grid
// builds), so a listed point has the bits of make_3d_grid's row.  Points, scatter and leak check run one workgroup per
// listed block, z fastest: stores and loads are contiguous runs of a block's z extent.  The leak check only walks the
// six faces of a block (an edge between two different owner blocks lies on a face of both) and issues one atomic per
// workgroup.  The block list comes from one exclusive rocPRIM scan (sort.hip) of packed per-block counts
// (owned points | selected << 32): fewer than 2^31 lattice points, so the low half never carries into the high half.
#include "common.h"
#include <algorithm>

using namespace svr;

namespace {

constexpr int kBlock = 256;
constexpr int kFillBlocks = 2048;  // grid-stride fill

struct Grid {
  int32_t n[3];   // lattice points per axis
  int32_t nb[3];  // blocks per axis
  int32_t s;      // block edge in cells
  int64_t sx, sy;  // lattice strides of axes 0 and 1 (axis 2: 1)
  int64_t np;      // lattice points
  int64_t nblk;    // blocks
  int64_t nc;      // coarse points
};

// first owned lattice index of block b along an axis, and the number of owned indices (the last block also owns n-1)
__device__ __forceinline__ int32_t lo_of(const Grid &G, int32_t b) { return b * G.s; }
__device__ __forceinline__ int32_t cnt_of(const Grid &G, int a, int32_t b) {
  return b == G.nb[a] - 1 ? G.n[a] - b * G.s : G.s;
}
__device__ __forceinline__ int32_t owner_of(const Grid &G, int a, int32_t i) { return min(i / G.s, G.nb[a] - 1); }
__device__ __forceinline__ int32_t coarse_of(const Grid &G, int a, int32_t c) { return min(c * G.s, G.n[a] - 1); }

__device__ __forceinline__ void block_coords(const Grid &G, int32_t b, int32_t bc[3]) {
  const int32_t yz = G.nb[1] * G.nb[2];
  bc[0] = b / yz;
  const int32_t r = b - bc[0] * yz;
  bc[1] = r / G.nb[2];
  bc[2] = r - bc[1] * G.nb[2];
}

__device__ __forceinline__ bool inside(float v, double level) { return (double)v < level; }

__global__ __launch_bounds__(kBlock) void sl_coarse_points_kernel(const float *__restrict__ tx, const float *__restrict__ ty,
                                                                  const float *__restrict__ tz, Grid G,
                                                                  float *__restrict__ pts) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= G.nc) return;
  const int32_t cy = G.nb[1] + 1, cz = G.nb[2] + 1;
  const int32_t i = (int32_t)(c / (cy * cz));
  const int32_t r = (int32_t)(c - (int64_t)i * (cy * cz));
  const int32_t j = r / cz, k = r - j * cz;
  float *o = pts + c * 3;
  o[0] = tx[coarse_of(G, 0, i)];
  o[1] = ty[coarse_of(G, 1, j)];
  o[2] = tz[coarse_of(G, 2, k)];
}

// every lattice point takes the coarse value at the minimum corner of its owner block
__global__ __launch_bounds__(kBlock) void sl_fill_kernel(const float *__restrict__ coarse, Grid G, float *__restrict__ field) {
  const int32_t cy = G.nb[1] + 1, cz = G.nb[2] + 1;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < G.np; p += (int64_t)gridDim.x * kBlock) {
    const int32_t i = (int32_t)(p / G.sx);
    const int32_t r = (int32_t)(p - (int64_t)i * G.sx);
    const int32_t j = r / G.n[2], k = r - j * G.n[2];
    field[p] = coarse[((int64_t)owner_of(G, 0, i) * cy + owner_of(G, 1, j)) * cz + owner_of(G, 2, k)];
  }
}

// round 1: a block is selected iff its 8 corner flags are not all equal; every state starts at 0
__global__ __launch_bounds__(kBlock) void sl_seed_kernel(const float *__restrict__ coarse, Grid G, double level,
                                                         uint8_t *__restrict__ sel, uint8_t *__restrict__ state) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= G.nblk) return;
  int32_t bc[3];
  block_coords(G, (int32_t)b, bc);
  const int32_t cy = G.nb[1] + 1, cz = G.nb[2] + 1;
  int in = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c)
    in += inside(coarse[((int64_t)(bc[0] + (c & 1)) * cy + bc[1] + ((c >> 1) & 1)) * cz + bc[2] + ((c >> 2) & 1)], level) ? 1 : 0;
  sel[b] = (in != 0 && in != 8) ? 1 : 0;
  state[b] = 0;
}

__global__ __launch_bounds__(kBlock) void sl_count_kernel(Grid G, int all, const uint8_t *__restrict__ state,
                                                          const uint8_t *__restrict__ sel, uint64_t *__restrict__ counts) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= G.nblk) return;
  const bool take = all ? state[b] == 0 : sel[b] != 0;
  uint64_t c = 0;
  if (take) {
    int32_t bc[3];
    block_coords(G, (int32_t)b, bc);
    c = (uint64_t)((int64_t)cnt_of(G, 0, bc[0]) * cnt_of(G, 1, bc[1]) * cnt_of(G, 2, bc[2])) | 1ull << 32;
  }
  counts[b] = c;
}

// list[rank] = block, start[rank] = first row of the block in the round's point list; the selection flags are consumed
__global__ __launch_bounds__(kBlock) void sl_compact_kernel(Grid G, const uint64_t *__restrict__ counts,
                                                            const uint64_t *__restrict__ offs, uint8_t *__restrict__ sel,
                                                            int32_t *__restrict__ list, int32_t *__restrict__ start,
                                                            long long *__restrict__ totals) {
  const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (b >= G.nblk) return;
  const uint64_t c = counts[b], o = offs[b];
  sel[b] = 0;
  if (c) {
    list[(uint32_t)(o >> 32)] = (int32_t)b;
    start[(uint32_t)(o >> 32)] = (int32_t)(uint32_t)o;
  }
  if (b == G.nblk - 1) {
    const uint64_t t = o + c;
    totals[0] = (long long)(t >> 32);
    totals[1] = (long long)(uint32_t)t;
  }
}

// the owned box of a listed block: lattice origin, extents
struct Box {
  int32_t lo[3], cnt[3];
};
__device__ __forceinline__ Box box_of(const Grid &G, int32_t b) {
  int32_t bc[3];
  block_coords(G, b, bc);
  Box B;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    B.lo[a] = lo_of(G, bc[a]);
    B.cnt[a] = cnt_of(G, a, bc[a]);
  }
  return B;
}

__global__ __launch_bounds__(kBlock) void sl_block_points_kernel(const float *__restrict__ tx, const float *__restrict__ ty,
                                                                 const float *__restrict__ tz, Grid G,
                                                                 const int32_t *__restrict__ list,
                                                                 const int32_t *__restrict__ start, float *__restrict__ pts) {
  const Box B = box_of(G, list[blockIdx.x]);
  const int64_t row0 = start[blockIdx.x];
  const int32_t yz = B.cnt[1] * B.cnt[2], total = B.cnt[0] * yz;
  for (int32_t t = threadIdx.x; t < total; t += kBlock) {
    const int32_t li = t / yz, r = t - li * yz;
    const int32_t lj = r / B.cnt[2], lk = r - lj * B.cnt[2];
    float *o = pts + (row0 + t) * 3;
    o[0] = tx[B.lo[0] + li];
    o[1] = ty[B.lo[1] + lj];
    o[2] = tz[B.lo[2] + lk];
  }
}

__global__ __launch_bounds__(kBlock) void sl_scatter_kernel(const float *__restrict__ vals, Grid G,
                                                            const int32_t *__restrict__ list,
                                                            const int32_t *__restrict__ start, int round,
                                                            float *__restrict__ field, uint8_t *__restrict__ state) {
  const int32_t b = list[blockIdx.x];
  const Box B = box_of(G, b);
  const int64_t row0 = start[blockIdx.x];
  const int32_t yz = B.cnt[1] * B.cnt[2], total = B.cnt[0] * yz;
  for (int32_t t = threadIdx.x; t < total; t += kBlock) {
    const int32_t li = t / yz, r = t - li * yz;
    const int32_t lj = r / B.cnt[2], lk = r - lj * B.cnt[2];
    field[(int64_t)(B.lo[0] + li) * G.sx + (int64_t)(B.lo[1] + lj) * G.sy + B.lo[2] + lk] = vals[row0 + t];
  }
  if (threadIdx.x == 0) state[b] = (uint8_t)round;
}

// Edges (p, q) along an axis with p owned by this (just evaluated) block and q by a block never evaluated lie on the block's
// faces.  A face whose neighbour has been evaluated, or does not exist, is skipped by the whole workgroup.
__global__ __launch_bounds__(kBlock) void sl_leak_kernel(const float *__restrict__ field, Grid G, double level,
                                                         const int32_t *__restrict__ list, const uint8_t *__restrict__ state,
                                                         uint8_t *__restrict__ sel, unsigned long long *__restrict__ leaks) {
  const int32_t b = list[blockIdx.x];
  int32_t bc[3];
  block_coords(G, b, bc);
  const Box B = box_of(G, b);
  const int64_t stride[3] = {G.sx, G.sy, 1};
  const int64_t bstride[3] = {(int64_t)G.nb[1] * G.nb[2], G.nb[2], 1};
  uint32_t n = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int u = a == 0 ? 1 : 0, v = a == 2 ? 1 : 2;  // the two other axes, u < v
#pragma unroll
    for (int d = -1; d <= 1; d += 2) {
      const int32_t nbc = bc[a] + d;
      if (nbc < 0 || nbc >= G.nb[a]) continue;
      const int64_t nbr = (int64_t)b + d * bstride[a];
      if (state[nbr] != 0) continue;
      const int32_t pa = d < 0 ? B.lo[a] : B.lo[a] + B.cnt[a] - 1;  // the neighbour exists: pa + d is a lattice index
      const int32_t total = B.cnt[u] * B.cnt[v];
      uint32_t m = 0;
      for (int32_t t = threadIdx.x; t < total; t += kBlock) {
        const int32_t lu = t / B.cnt[v], lv = t - lu * B.cnt[v];
        const int64_t p = (int64_t)pa * stride[a] + (int64_t)(B.lo[u] + lu) * stride[u] + (int64_t)(B.lo[v] + lv) * stride[v];
        m += inside(field[p], level) != inside(field[p + d * stride[a]], level) ? 1u : 0u;
      }
      if (m) sel[nbr] = 1;  // every writer stores the same value
      n += m;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
  __shared__ uint32_t part[kBlock / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (int q = 0; q < kBlock / 64; ++q) sum += part[q];
    if (sum) atomicAdd(leaks, (unsigned long long)sum);
  }
}


bool grid(int32_t X, int32_t Y, int32_t Z, int32_t s, Grid &G) {
  if (X < 2 || Y < 2 || Z < 2 || s < 2) return false;
  const int32_t n[3] = {X, Y, Z};
  G.s = s;
  G.nblk = 1;
  G.nc = 1;
  for (int a = 0; a < 3; ++a) {
    G.n[a] = n[a];
    G.nb[a] = (int32_t)cdiv((int64_t)n[a] - 1, s);
    G.nblk *= G.nb[a];
    G.nc *= G.nb[a] + 1;
  }
  G.sy = Z;
  G.sx = (int64_t)Y * Z;
  G.np = (int64_t)X * Y * Z;
  return G.np < (1LL << 31);
}

struct Ws {
  uint64_t *counts, *offs;
  int32_t *list, *start;
  uint8_t *sel;
  void *tmp;
  size_t tmp_bytes;
};

Ws ws_layout(WsCursor &c, int64_t nblk) {   // the launchers have always used the caller's pointer as it is: base alignment 1
  const size_t tmp_bytes = scan_sum_excl_u64_temp_bytes(nblk);
  return {c.take<uint64_t>(nblk), c.take<uint64_t>(nblk), c.take<int32_t>(nblk), c.take<int32_t>(nblk), c.take<uint8_t>(nblk),
          c.take<char>((int64_t)tmp_bytes), tmp_bytes};
}

#define SL_GRID(name)                                                                                                      \
  Grid G;                                                                                                                  \
  SVR_CHECK(grid(X, Y, Z, s, G), SVR_E_BADSHAPE,                                                                           \
            name ": bad lattice %d x %d x %d, block %d (extents >= 2, block >= 2, fewer than 2^31 points)", X, Y, Z, s)

}  // namespace

extern "C" int64_t svr_sl_workspace_bytes(int32_t X, int32_t Y, int32_t Z, int32_t s) {
  Grid G;
  if (!grid(X, Y, Z, s, G)) {
    set_error("sl_workspace_bytes: bad lattice %d x %d x %d, block %d", X, Y, Z, s);
    return SVR_E_BADSHAPE;
  }
  return ws_measure(ws_layout, G.nblk);
}

extern "C" int svr_sl_coarse_points(const float *tx, const float *ty, const float *tz, int32_t X, int32_t Y, int32_t Z,
                                    int32_t s, float *pts, void *stream) {
  SL_GRID("sl_coarse_points");
  SVR_CHECK(tx && ty && tz && pts, SVR_E_BADARG, "sl_coarse_points: null pointer");
  hipLaunchKernelGGL(sl_coarse_points_kernel, dim3((unsigned)cdiv(G.nc, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, tx,
                     ty, tz, G, pts);
  return launch_status("sl_coarse_points");
}

extern "C" int svr_sl_fill_seed(const float *coarse, int32_t X, int32_t Y, int32_t Z, int32_t s, double level, float *field,
                                uint8_t *state, void *ws, int64_t ws_bytes, void *stream) {
  SL_GRID("sl_fill_seed");
  SVR_CHECK(coarse && field && state && ws, SVR_E_BADARG, "sl_fill_seed: null pointer");
  WsCursor c(ws, 1);
  const Ws w = ws_layout(c, G.nblk);
  SVR_CHECK(ws_bytes >= c.bytes(), SVR_E_BADARG, "sl_fill_seed: workspace of %ld bytes, need %ld", (long)ws_bytes, (long)c.bytes());
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sl_fill_kernel, dim3((unsigned)std::min<int64_t>(cdiv(G.np, kBlock), kFillBlocks)), dim3(kBlock), 0, st,
                     coarse, G, field);
  int rc = launch_status("sl_fill");
  if (rc) return rc;
  hipLaunchKernelGGL(sl_seed_kernel, dim3((unsigned)cdiv(G.nblk, kBlock)), dim3(kBlock), 0, st, coarse, G, level, w.sel, state);
  return launch_status("sl_seed");
}

extern "C" int svr_sl_select(int32_t X, int32_t Y, int32_t Z, int32_t s, int32_t all, const uint8_t *state, void *ws,
                             int64_t *totals, void *stream) {
  SL_GRID("sl_select");
  SVR_CHECK(state && ws && totals, SVR_E_BADARG, "sl_select: null pointer");
  WsCursor c(ws, 1);
  const Ws w = ws_layout(c, G.nblk);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 blocks((unsigned)cdiv(G.nblk, kBlock));
  hipLaunchKernelGGL(sl_count_kernel, blocks, dim3(kBlock), 0, st, G, (int)(all != 0), state, w.sel, w.counts);
  int rc = launch_status("sl_count");
  if (rc) return rc;
  hipError_t e = scan_sum_excl_u64(w.tmp, w.tmp_bytes, w.counts, w.offs, G.nblk, st);
  SVR_CHECK(e == hipSuccess, (int)e, "sl_select: scan failed: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(sl_compact_kernel, blocks, dim3(kBlock), 0, st, G, w.counts, w.offs, w.sel, w.list, w.start,
                     (long long *)totals);
  return launch_status("sl_compact");
}

extern "C" int svr_sl_block_points(const float *tx, const float *ty, const float *tz, int32_t X, int32_t Y, int32_t Z,
                                   int32_t s, const void *ws, int64_t n_blocks, float *pts, void *stream) {
  SL_GRID("sl_block_points");
  SVR_CHECK(n_blocks >= 0 && n_blocks <= G.nblk, SVR_E_BADSHAPE, "sl_block_points: %ld listed blocks of %ld", (long)n_blocks,
            (long)G.nblk);
  if (n_blocks == 0) return SVR_OK;
  SVR_CHECK(tx && ty && tz && ws && pts, SVR_E_BADARG, "sl_block_points: null pointer");
  WsCursor c(ws, 1);
  const Ws w = ws_layout(c, G.nblk);
  hipLaunchKernelGGL(sl_block_points_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)stream, tx, ty, tz, G,
                     w.list, w.start, pts);
  return launch_status("sl_block_points");
}

extern "C" int svr_sl_scatter(const float *vals, int32_t X, int32_t Y, int32_t Z, int32_t s, const void *ws, int64_t n_blocks,
                              int32_t round, float *field, uint8_t *state, void *stream) {
  SL_GRID("sl_scatter");
  SVR_CHECK(n_blocks >= 0 && n_blocks <= G.nblk, SVR_E_BADSHAPE, "sl_scatter: %ld listed blocks of %ld", (long)n_blocks,
            (long)G.nblk);
  SVR_CHECK(round >= 1 && round <= 255, SVR_E_BADARG, "sl_scatter: round %d outside [1, 255]", round);
  if (n_blocks == 0) return SVR_OK;
  SVR_CHECK(vals && ws && field && state, SVR_E_BADARG, "sl_scatter: null pointer");
  WsCursor c(ws, 1);
  const Ws w = ws_layout(c, G.nblk);
  hipLaunchKernelGGL(sl_scatter_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, (hipStream_t)stream, vals, G, w.list,
                     w.start, (int)round, field, state);
  return launch_status("sl_scatter");
}

extern "C" int svr_sl_leak_check(const float *field, int32_t X, int32_t Y, int32_t Z, int32_t s, double level,
                                 const uint8_t *state, void *ws, int64_t n_blocks, int64_t *totals, void *stream) {
  SL_GRID("sl_leak_check");
  SVR_CHECK(n_blocks >= 0 && n_blocks <= G.nblk, SVR_E_BADSHAPE, "sl_leak_check: %ld listed blocks of %ld", (long)n_blocks,
            (long)G.nblk);
  SVR_CHECK(totals, SVR_E_BADARG, "sl_leak_check: null totals");
  const hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(totals + 2, 0, sizeof(int64_t), st);
  SVR_CHECK(e == hipSuccess, (int)e, "sl_leak_check: memset failed: %s", hipGetErrorString(e));
  if (n_blocks == 0) return SVR_OK;
  SVR_CHECK(field && state && ws, SVR_E_BADARG, "sl_leak_check: null pointer");
  WsCursor c(ws, 1);
  const Ws w = ws_layout(c, G.nblk);
  hipLaunchKernelGGL(sl_leak_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, st, field, G, level, w.list, state, w.sel,
                     (unsigned long long *)(totals + 2));
  return launch_status("sl_leak");
}
