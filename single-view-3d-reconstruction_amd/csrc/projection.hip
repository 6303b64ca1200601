// Depth map -> camera points -> grid space -> trilinear splat -> separable Gaussian blur, gfx950.
//
// Replaces the reference's `project` module (model/projection.py):
//   unproject  : depth_to_camera :199-206 + the 4x4 camera->frustum affine :160-161 (+ the
//                grid-space normalisation :124-132), one elementwise pass;
//   splat      : pc_voxels :39-80 (validity test, integer base voxel, 8 weighted index_put_
//                accumulations) with f32 atomics;  the x8 aliasing quirk and the clamp are
//                svr_scale_clamp01 (scale 8);  svr_voxelize_splat_fwd_ordered is the atomic-free form in a fixed
//                summation order (sort by base cell + pull kernel) that ifnet.DETERMINISTIC selects;
//   blur       : voxels_smooth :100-117, one pass per axis, taps from the learnable sigma.
// All are HBM / atomic bound elementwise kernels (no MFMA).  Compiled with -ffp-contract=off
// so the base-voxel arithmetic ((p+0.5)*(dims-1), floor) rounds exactly like torch's separate ops
// and the integer voxel indices are bit-exact.
#include "common.h"
#include "unproject.h"
#include "reduce.h"

using namespace svr;

namespace {

__global__ void unproject_fwd_kernel(const float *__restrict__ depth, float *__restrict__ pc, int64_t total, int Hi,
                                     int Wi, UnprojConsts c, int normalize) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int u = (int)(i % Wi), v = (int)((i / Wi) % Hi);
  float gx, gy, gz;
  unproject_point(depth[i], u, v, c, gx, gy, gz);
  if (normalize) {
    gx = (gx - c.d0 / 2.f) / c.d0;
    gy = (gy - c.d1 / 2.f) / c.d1;
    gz = (gz - c.d2 / 2.f) / c.d2;
  }
  pc[i * 3 + 0] = gx;
  pc[i * 3 + 1] = gy;
  pc[i * 3 + 2] = gz;
}

__global__ void unproject_bwd_kernel(const float *__restrict__ gpc, float *__restrict__ gdepth, int64_t total, int Hi,
                                     int Wi, UnprojConsts c, int normalize) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int u = (int)(i % Wi), v = (int)((i / Wi) % Hi);
  float a0 = c.s00 * (((float)u - c.cx) / c.f);
  float a1 = -c.s11 * (((float)v - c.cy) / c.f);
  float a2 = c.s22;
  if (normalize) { a0 /= c.d0; a1 /= c.d1; a2 /= c.d2; }
  gdepth[i] = gpc[i * 3] * a0 + gpc[i * 3 + 1] * a1 + gpc[i * 3 + 2] * a2;
}

struct Splat {
  bool valid;
  int i0, i1, i2;
  float r0, r1, r2;
};

__device__ __forceinline__ Splat splat_of(const float *__restrict__ p, int D0, int D1, int D2) {
  const float hi = (float)(0.5 - 1e-6), lo = (float)(-0.5 + 1e-6);  // torch compares in float32
  Splat s;
  float a = p[0], b = p[1], c = p[2];
  s.valid = (a < hi && a > lo) && (b < hi && b > lo) && (c < hi && c > lo);
  float g0 = (a + 0.5f) * (float)(D0 - 1), g1 = (b + 0.5f) * (float)(D1 - 1), g2 = (c + 0.5f) * (float)(D2 - 1);
  float f0 = floorf(g0), f1 = floorf(g1), f2 = floorf(g2);
  s.r0 = g0 - f0; s.r1 = g1 - f1; s.r2 = g2 - f2;
  float cl = 2.0e9f;
  s.i0 = (int)fminf(fmaxf(f0, -cl), cl);
  s.i1 = (int)fminf(fmaxf(f1, -cl), cl);
  s.i2 = (int)fminf(fmaxf(f2, -cl), cl);
  if (a != a || b != b || c != c) { s.valid = false; s.i0 = s.i1 = s.i2 = 0; }
  return s;
}

__global__ void splat_fwd_kernel(const float *__restrict__ pts, float *__restrict__ acc, int32_t *__restrict__ base,
                                 uint8_t *__restrict__ valid, int64_t total, int N, int D0, int D1, int D2) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  Splat s = splat_of(pts + i * 3, D0, D1, D2);
  if (base) { base[i * 3] = s.i0; base[i * 3 + 1] = s.i1; base[i * 3 + 2] = s.i2; }
  if (valid) valid[i] = s.valid ? 1 : 0;
  if (!s.valid) return;
  int64_t b = i / N;
  float w0[2] = {1.f - s.r0, s.r0}, w1[2] = {1.f - s.r1, s.r1}, w2[2] = {1.f - s.r2, s.r2};
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int l = 0; l < 2; ++l) {
        int z = s.i0 + k, y = s.i1 + j, x = s.i2 + l;
        if (z >= 0 && z < D0 && y >= 0 && y < D1 && x >= 0 && x < D2)
          atomicAdd(acc + ((b * D0 + z) * D1 + y) * (int64_t)D2 + x, (w0[k] * w1[j]) * w2[l]);
      }
}

__global__ void splat_bwd_kernel(const float *__restrict__ pts, const float *__restrict__ gacc,
                                 float *__restrict__ gpts, int64_t total, int N, int D0, int D1, int D2) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  Splat s = splat_of(pts + i * 3, D0, D1, D2);
  float g0 = 0.f, g1 = 0.f, g2 = 0.f;
  if (s.valid) {
    int64_t b = i / N;
    float w0[2] = {1.f - s.r0, s.r0}, w1[2] = {1.f - s.r1, s.r1}, w2[2] = {1.f - s.r2, s.r2};
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int l = 0; l < 2; ++l) {
          int z = s.i0 + k, y = s.i1 + j, x = s.i2 + l;
          if (z >= 0 && z < D0 && y >= 0 && y < D1 && x >= 0 && x < D2) {
            float g = gacc[((b * D0 + z) * D1 + y) * (int64_t)D2 + x];
            g0 += (k ? g : -g) * w1[j] * w2[l];
            g1 += (j ? g : -g) * w0[k] * w2[l];
            g2 += (l ? g : -g) * w0[k] * w1[j];
          }
        }
    g0 *= (float)(D0 - 1); g1 *= (float)(D1 - 1); g2 *= (float)(D2 - 1);
  }
  gpts[i * 3] = g0; gpts[i * 3 + 1] = g1; gpts[i * 3 + 2] = g2;
}

// clamp(scale * v, 0, 1) like torch.clamp: NaN stays NaN (fminf / fmaxf alone return the other operand, which turned a NaN
// grid into a clean all-zero occupancy with zero gradients); every other value as fminf(fmaxf(., 0), 1)
__device__ __forceinline__ float scale_clamp01(float v, float scale) {
  const float s = v * scale;
  return s != s ? s : fminf(fmaxf(s, 0.f), 1.f);
}

__global__ void scale_clamp_fwd_kernel(const float *__restrict__ in, float *__restrict__ out, int64_t n, float scale) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = scale_clamp01(in[i], scale);
}

__global__ void scale_clamp_bwd_kernel(const float *__restrict__ in, const float *__restrict__ gout,
                                       float *__restrict__ gin, int64_t n, float scale) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = in[i] * scale;
  gin[i] = (v >= 0.f && v <= 1.f) ? gout[i] * scale : 0.f;
}

constexpr int KMAX = 15;

// out[i] = sum_t in[i + (t - K/2)*stride_axis] * taps[t]   (ADJ: gin = sum_t gout[i - (t-K/2)] taps[t])
template <bool ADJ>
__global__ void blur_axis_kernel(const float *__restrict__ in, const float *__restrict__ taps, float *__restrict__ out,
                                 int64_t total, int len, int64_t stride, int K) {
  __shared__ float tp[KMAX];
  if ((int)threadIdx.x < K) tp[threadIdx.x] = taps[threadIdx.x];
  __syncthreads();
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int pos = (int)((i / stride) % len);
  float s = 0.f;
  for (int t = 0; t < K; ++t) {
    int o = ADJ ? (K / 2 - t) : (t - K / 2);
    int p = pos + o;
    if (p >= 0 && p < len) s += in[i + (int64_t)o * stride] * tp[t];
  }
  out[i] = s;
}

// gtaps[t] += sum_i gout[i] * in[i + (t-K/2)]
__global__ __launch_bounds__(256) void blur_taps_grad_kernel(const float *__restrict__ in,
                                                             const float *__restrict__ gout, double *__restrict__ gtaps,
                                                             int64_t total, int len, int64_t stride, int K) {
  float s[KMAX];
#pragma unroll
  for (int t = 0; t < KMAX; ++t) s[t] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int pos = (int)((i / stride) % len);
    float g = gout[i];
#pragma unroll
    for (int t = 0; t < KMAX; ++t) {
      if (t < K) {
        int p = pos + t - K / 2;
        if (p >= 0 && p < len) s[t] += g * in[i + (int64_t)(t - K / 2) * stride];
      }
    }
  }
  __shared__ double red[256];
  for (int t = 0; t < K; ++t) {
    block_sum_f64((double)s[t], red);
    if (threadIdx.x == 0) atomicAdd(gtaps + t, red[0]);
    __syncthreads();
  }
}

// blur_taps_grad_kernel with the block sums stored (part[block][K]) instead of added atomically; the same per-thread
// float32 partials and the same float64 tree
__global__ __launch_bounds__(256) void blur_taps_grad_parts_kernel(const float *__restrict__ in,
                                                                   const float *__restrict__ gout, double *__restrict__ part,
                                                                   int64_t total, int len, int64_t stride, int K) {
  float s[KMAX];
#pragma unroll
  for (int t = 0; t < KMAX; ++t) s[t] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int pos = (int)((i / stride) % len);
    float g = gout[i];
#pragma unroll
    for (int t = 0; t < KMAX; ++t) {
      if (t < K) {
        int p = pos + t - K / 2;
        if (p >= 0 && p < len) s[t] += g * in[i + (int64_t)(t - K / 2) * stride];
      }
    }
  }
  __shared__ double red[256];
  for (int t = 0; t < K; ++t) {
    block_sum_f64((double)s[t], red);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.x * K + t] = red[0];
    __syncthreads();
  }
}

// gtaps[t] from part[.][t], one 64-thread workgroup per tap, in a fixed order (depth_head.hip's loss pattern): lane i adds
// blocks i, i + 64, i + 128, ... in ascending order, then the 64 lane sums go through a fixed tree.  (One thread walking
// all 1024 block sums: 100 us per axis at 128^3 -- a chain of dependent loads.)
__global__ __launch_bounds__(64) void blur_taps_final_kernel(const double *__restrict__ part, double *__restrict__ gtaps,
                                                             int blocks, int K) {
  const int t = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 64) s += part[(int64_t)b * K + t];
  __shared__ double red[64];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 32; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) gtaps[t] = red[0];
}

int64_t taps_grad_blocks(int64_t total) {
  int64_t blocks = cdiv(total, 256 * 8);
  return blocks > 1024 ? 1024 : (blocks < 1 ? 1 : blocks);
}

int axis_geometry(int D0, int D1, int D2, int axis, int *len, int64_t *stride) {
  SVR_CHECK(axis >= 0 && axis <= 2, SVR_E_BADARG, "blur: axis %d", axis);
  *len = axis == 0 ? D0 : (axis == 1 ? D1 : D2);
  *stride = axis == 0 ? (int64_t)D1 * D2 : (axis == 1 ? D2 : 1);
  return SVR_OK;
}

// ---------------------------------------------------------------------------------------------
// Ordered splat (svr_voxelize_splat_fwd_ordered; summation order: include/svr_hip.h).  The plan of gather.hip's pull
// scatter on the points themselves: key = row-major index of the cell (b, i0 + 1, i1 + 1, i2 + 1) in a
// (D0+1) x (D1+1) x (D2+1) lattice, stable radix sort (ascending point index inside a cell), one 16-byte record per
// sorted point, cs[c] = number of points with a key below c.  A voxel's partial P[k][j][l] only ever receives from ONE
// cell, (z - k, y - j, x - l), so the order in which a thread visits its cells does not enter the result.
// ---------------------------------------------------------------------------------------------
struct SplatRec {
  float r0, r1, r2;
  int32_t cx;  // x cell coordinate i2 + 1
};

constexpr int SPLAT_XS = 4;  // x voxels per thread

__device__ __forceinline__ bool splat_cell(const Splat &s, int64_t b, int D0, int D1, int D2, uint32_t &key) {
  if (!s.valid) return false;
  if (!(s.i0 >= -1 && s.i0 < D0 && s.i1 >= -1 && s.i1 < D1 && s.i2 >= -1 && s.i2 < D2)) return false;  // touches no voxel
  key = (uint32_t)(((b * (D0 + 1) + s.i0 + 1) * (D1 + 1) + s.i1 + 1) * (D2 + 1) + s.i2 + 1);
  return true;
}

__global__ __launch_bounds__(256) void splat_key_kernel(const float *__restrict__ pts, uint32_t *__restrict__ keys,
                                                        int32_t *__restrict__ vals, int32_t *__restrict__ base,
                                                        uint8_t *__restrict__ valid, int64_t total, int N, int D0, int D1,
                                                        int D2, uint32_t sentinel) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const Splat s = splat_of(pts + i * 3, D0, D1, D2);
  if (base) { base[i * 3] = s.i0; base[i * 3 + 1] = s.i1; base[i * 3 + 2] = s.i2; }
  if (valid) valid[i] = s.valid ? 1 : 0;
  uint32_t key;
  const bool ok = splat_cell(s, i / N, D0, D1, D2, key);
  keys[i] = ok ? key : sentinel;
  vals[i] = (int32_t)i;
}

// sorted point -> record; the last point of a cell writes the cell's end (ends[0] stays 0)
__global__ __launch_bounds__(256) void splat_record_kernel(const float *__restrict__ pts, const uint32_t *__restrict__ keys,
                                                           const int32_t *__restrict__ items, SplatRec *__restrict__ recs,
                                                           int32_t *__restrict__ ends, int64_t total, int D0, int D1, int D2,
                                                           uint32_t sentinel) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const uint32_t k = keys[idx];
  if (k >= sentinel) return;
  const int64_t pn = items[idx];
  const Splat s = splat_of(pts + pn * 3, D0, D1, D2);
  SplatRec r;
  r.r0 = s.r0; r.r1 = s.r1; r.r2 = s.r2;
  r.cx = s.i2 + 1;
  recs[idx] = r;
  if (idx == total - 1 || keys[idx + 1] != k) ends[k + 1] = (int32_t)idx + 1;
}

// one thread = SPLAT_XS consecutive x voxels of one (b, z, y) row; its four (k, j) cell rows are four contiguous CSR ranges
__global__ __launch_bounds__(256) void splat_pull_kernel(float *__restrict__ acc, float *__restrict__ vox,
                                                         const SplatRec *__restrict__ recs, const int32_t *__restrict__ cs,
                                                         int n_items, int64_t strips, int D0, int D1, int D2) {
  constexpr int XS = SPLAT_XS;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= strips) return;
  const int nsx = (D2 + XS - 1) / XS;
  const int x0 = (int)(t % nsx) * XS;
  int64_t q = t / nsx;
  const int y = (int)(q % D1); q /= D1;
  const int z = (int)(q % D0);
  const int64_t b = q / D0;
  const int ncell = min(XS, D2 - x0) + 1;  // cell coordinates x0 .. x0 + ncell - 1 (they end at D2)
  int lo[4], hi[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int k = w >> 1, j = w & 1;  // base voxel (z - k, y - j): cell coordinates (z + 1 - k, y + 1 - j)
    const int64_t kb = ((b * (D0 + 1) + z + 1 - k) * (D1 + 1) + y + 1 - j) * (D2 + 1) + x0;
    lo[w] = cs[kb];
    hi[w] = cs[kb + ncell];
  }
  float P[XS][8];  // [voxel][k*4 + j*2 + l]
#pragma unroll
  for (int i = 0; i < XS; ++i)
#pragma unroll
    for (int c = 0; c < 8; ++c) P[i][c] = 0.f;
  const int last = n_items > 0 ? n_items - 1 : 0;
  while (lo[0] < hi[0] || lo[1] < hi[1] || lo[2] < hi[2] || lo[3] < hi[3]) {
    SplatRec r[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) r[w] = recs[min(lo[w], last)];  // unconditional, clamped: all four loads in flight together
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int k = w >> 1, j = w & 1;
      if (lo[w] < hi[w]) {
        const int o = r[w].cx - x0;  // cell x0 + o = base voxel x0 + o - 1: corner l = 1 is voxel x0 + o, l = 0 voxel x0 + o - 1
        const float wkj = (k ? r[w].r0 : 1.f - r[w].r0) * (j ? r[w].r1 : 1.f - r[w].r1);
        const float wl1 = wkj * r[w].r2, wl0 = wkj * (1.f - r[w].r2);
#pragma unroll
        for (int i = 0; i < XS; ++i) {
          if (o == i) P[i][w * 2 + 1] += wl1;
          if (o == i + 1) P[i][w * 2] += wl0;
        }
        ++lo[w];
      }
    }
  }
  const int64_t out = ((b * D0 + z) * D1 + y) * (int64_t)D2 + x0;
#pragma unroll
  for (int i = 0; i < XS; ++i)
    if (x0 + i < D2) {
      const float v = ((P[i][0] + P[i][1]) + (P[i][2] + P[i][3])) + ((P[i][4] + P[i][5]) + (P[i][6] + P[i][7]));
      acc[out + i] = v;
      if (vox) vox[out + i] = scale_clamp01(v, 8.f);
    }
}

int64_t splat_cells(int B, int D0, int D1, int D2) { return (int64_t)B * (D0 + 1) * (D1 + 1) * (D2 + 1); }
int splat_key_bits(int64_t cells) {  // the sentinel (= cells) must fit
  int nb = 1;
  while ((1LL << nb) <= cells) ++nb;
  return nb;
}
bool splat_ordered_fits(int B, int N, int D0, int D1, int D2) {
  // (dims up to 2^20 per axis keep the cell product inside int64)
  return B >= 0 && N >= 0 && D0 > 0 && D1 > 0 && D2 > 0 && D0 < (1 << 20) && D1 < (1 << 20) && D2 < (1 << 20) &&
         (int64_t)(D0 + 1) * (D1 + 1) < (1LL << 31) && ((int64_t)(D0 + 1) * (D1 + 1)) * (D2 + 1) < (1LL << 31) &&
         splat_cells(B, D0, D1, D2) < (1LL << 31) - 1 && (int64_t)B * N < (1LL << 31);
}

}  // namespace

extern "C" int svr_unproject_fwd(const float *depth, float *pc, int32_t B, int32_t Hi, int32_t Wi, const float *consts,
                                 int normalize, void *stream) {
  SVR_CHECK(depth && pc && consts, SVR_E_BADARG, "unproject_fwd: null pointer");
  int64_t total = (int64_t)B * Hi * Wi;
  if (total <= 0) return SVR_OK;
  hipLaunchKernelGGL(unproject_fwd_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, depth, pc,
                     total, Hi, Wi, unproj_consts(consts), normalize);
  return launch_status("unproject_fwd");
}

extern "C" int svr_unproject_bwd(const float *depth, const float *gpc, float *gdepth, int32_t B, int32_t Hi, int32_t Wi,
                                 const float *consts, int normalize, void *stream) {
  (void)depth;
  SVR_CHECK(gpc && gdepth && consts, SVR_E_BADARG, "unproject_bwd: null pointer");
  int64_t total = (int64_t)B * Hi * Wi;
  if (total <= 0) return SVR_OK;
  hipLaunchKernelGGL(unproject_bwd_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, gpc,
                     gdepth, total, Hi, Wi, unproj_consts(consts), normalize);
  return launch_status("unproject_bwd");
}

extern "C" int svr_voxelize_splat_fwd(const float *pts, float *acc, int32_t *base, uint8_t *valid, int32_t B, int32_t N,
                                      int32_t D0, int32_t D1, int32_t D2, void *stream) {
  int64_t total = (int64_t)B * N;
  if (total <= 0) return SVR_OK;  // empty point cloud: nothing to add
  SVR_CHECK(pts && acc, SVR_E_BADARG, "splat_fwd: null pointer");
  SVR_CHECK(D0 > 0 && D1 > 0 && D2 > 0, SVR_E_BADSHAPE, "splat_fwd: dims %dx%dx%d", D0, D1, D2);
  hipLaunchKernelGGL(splat_fwd_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, pts, acc, base,
                     valid, total, N, D0, D1, D2);
  return launch_status("splat_fwd");
}

namespace {
struct SplatWs {
  int32_t *ends, *cs;
  char *scan_tmp;
  size_t scan_bytes;
  uint32_t *keys_in = nullptr, *keys = nullptr;   // the item pieces exist only for T > 0
  int32_t *vals_in = nullptr, *items = nullptr;
  SplatRec *recs = nullptr;
  char *sort_tmp = nullptr;
};
SplatWs splat_ordered_layout(WsCursor &c, int64_t cells, int64_t T) {
  SplatWs w;
  w.ends = c.take<int32_t>(cells + 1);
  w.cs = c.take<int32_t>(cells + 1);
  w.scan_bytes = svr::scan_max_i32_temp_bytes(cells + 1);
  w.scan_tmp = c.take<char>((int64_t)w.scan_bytes);
  if (T > 0) {
    w.keys_in = c.take<uint32_t>(T);
    w.vals_in = c.take<int32_t>(T);
    w.keys = c.take<uint32_t>(T);
    w.items = c.take<int32_t>(T);
    w.recs = c.take<SplatRec>(T);
    w.sort_tmp = c.take<char>((int64_t)svr::sort_pairs_u32_temp_bytes(T, 32));   // for the widest key; sorted with fewer bits
  }
  c.take<char>(256);   // pad: unused, the size has always carried it
  return w;
}
}  // namespace

extern "C" int64_t svr_voxelize_splat_ordered_workspace(int32_t B, int32_t N, int32_t D0, int32_t D1, int32_t D2) {
  if (!splat_ordered_fits(B, N, D0, D1, D2)) return SVR_E_UNSUPPORTED;
  return ws_measure(splat_ordered_layout, splat_cells(B, D0, D1, D2), (int64_t)B * N);
}

extern "C" int svr_voxelize_splat_fwd_ordered(const float *pts, float *acc, float *vox, int32_t *base, uint8_t *valid,
                                              int32_t B, int32_t N, int32_t D0, int32_t D1, int32_t D2, void *workspace,
                                              void *stream) {
  SVR_CHECK(B >= 0 && N >= 0 && D0 > 0 && D1 > 0 && D2 > 0, SVR_E_BADSHAPE, "splat_fwd_ordered: B=%d N=%d dims %dx%dx%d", B, N,
            D0, D1, D2);
  SVR_CHECK(splat_ordered_fits(B, N, D0, D1, D2), SVR_E_UNSUPPORTED,
            "splat_fwd_ordered: %ld x (%d+1)(%d+1)(%d+1) cells / %ld points exceed the 32-bit keys of the ordered splat "
            "(cells < 2^31 - 1, points < 2^31)", (long)B, D0, D1, D2, (long)((int64_t)B * N));
  if (B == 0) return SVR_OK;
  SVR_CHECK(acc && workspace, SVR_E_BADARG, "splat_fwd_ordered: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int64_t cells = splat_cells(B, D0, D1, D2), T = (int64_t)B * N;
  WsCursor c(workspace);
  const SplatWs w = splat_ordered_layout(c, cells, T);
  hipError_t e = hipMemsetAsync(w.ends, 0, (size_t)(cells + 1) * sizeof(int32_t), s);
  SVR_CHECK(e == hipSuccess, (int)e, "splat_fwd_ordered: memset failed: %s", hipGetErrorString(e));
  if (T > 0) {
    SVR_CHECK(pts, SVR_E_BADARG, "splat_fwd_ordered: null points");
    const uint32_t sentinel = (uint32_t)cells;
    const int bits = splat_key_bits(cells);
    hipLaunchKernelGGL(splat_key_kernel, dim3((unsigned)cdiv(T, 256)), dim3(256), 0, s, pts, w.keys_in, w.vals_in, base, valid, T, N,
                       D0, D1, D2, sentinel);
    e = svr::sort_pairs_u32(w.sort_tmp, svr::sort_pairs_u32_temp_bytes(T, bits), w.keys_in, w.keys, w.vals_in, w.items, T, bits, s);
    SVR_CHECK(e == hipSuccess, (int)e, "splat_fwd_ordered: radix sort failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(splat_record_kernel, dim3((unsigned)cdiv(T, 256)), dim3(256), 0, s, pts, (const uint32_t *)w.keys,
                       (const int32_t *)w.items, w.recs, w.ends, T, D0, D1, D2, sentinel);
  }
  e = svr::scan_max_i32(w.scan_tmp, w.scan_bytes, w.ends, w.cs, cells + 1, s);
  SVR_CHECK(e == hipSuccess, (int)e, "splat_fwd_ordered: scan failed: %s", hipGetErrorString(e));
  const int64_t strips = (int64_t)B * D0 * D1 * cdiv(D2, SPLAT_XS);  // < cells < 2^31
  hipLaunchKernelGGL(splat_pull_kernel, dim3((unsigned)cdiv(strips, 256)), dim3(256), 0, s, acc, vox, (const SplatRec *)w.recs, (const int32_t *)w.cs,
                     (int)T, strips, D0, D1, D2);
  return launch_status("splat_fwd_ordered");
}

extern "C" int svr_voxelize_splat_bwd(const float *pts, const float *gacc, float *gpts, int32_t B, int32_t N, int32_t D0,
                                      int32_t D1, int32_t D2, void *stream) {
  int64_t total = (int64_t)B * N;
  if (total <= 0) return SVR_OK;
  SVR_CHECK(pts && gacc && gpts, SVR_E_BADARG, "splat_bwd: null pointer");
  hipLaunchKernelGGL(splat_bwd_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, pts, gacc, gpts,
                     total, N, D0, D1, D2);
  return launch_status("splat_bwd");
}

extern "C" int svr_scale_clamp01_fwd(const float *in, float *out, int64_t n, float scale, void *stream) {
  SVR_CHECK(in && out, SVR_E_BADARG, "scale_clamp01_fwd: null pointer");
  if (n <= 0) return SVR_OK;
  hipLaunchKernelGGL(scale_clamp_fwd_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, in, out, n, scale);
  return launch_status("scale_clamp01_fwd");
}

extern "C" int svr_scale_clamp01_bwd(const float *in, const float *gout, float *gin, int64_t n, float scale, void *stream) {
  SVR_CHECK(in && gout && gin, SVR_E_BADARG, "scale_clamp01_bwd: null pointer");
  if (n <= 0) return SVR_OK;
  hipLaunchKernelGGL(scale_clamp_bwd_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, in, gout, gin, n, scale);
  return launch_status("scale_clamp01_bwd");
}

extern "C" int svr_blur_axis_fwd(const float *in, const float *taps, float *out, int32_t B, int32_t D0, int32_t D1,
                                 int32_t D2, int32_t axis, int32_t K, void *stream) {
  SVR_CHECK(in && taps && out, SVR_E_BADARG, "blur_fwd: null pointer");
  SVR_CHECK(K >= 1 && K <= KMAX && (K & 1), SVR_E_UNSUPPORTED, "blur_fwd: K=%d (odd, <= %d)", K, KMAX);
  int len;
  int64_t stride;
  if (int rc = axis_geometry(D0, D1, D2, axis, &len, &stride)) return rc;
  int64_t total = (int64_t)B * D0 * D1 * D2;
  if (total <= 0) return SVR_OK;
  hipLaunchKernelGGL(blur_axis_kernel<false>, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, in, taps,
                     out, total, len, stride, K);
  return launch_status("blur_fwd");
}

extern "C" int svr_blur_axis_bwd(const float *in, const float *taps, const float *gout, float *gin, double *gtaps,
                                 int32_t B, int32_t D0, int32_t D1, int32_t D2, int32_t axis, int32_t K, void *stream) {
  SVR_CHECK(in && taps && gout, SVR_E_BADARG, "blur_bwd: null pointer");
  SVR_CHECK(K >= 1 && K <= KMAX && (K & 1), SVR_E_UNSUPPORTED, "blur_bwd: K=%d (odd, <= %d)", K, KMAX);
  int len;
  int64_t stride;
  if (int rc = axis_geometry(D0, D1, D2, axis, &len, &stride)) return rc;
  int64_t total = (int64_t)B * D0 * D1 * D2;
  if (total <= 0) return SVR_OK;
  hipStream_t s = (hipStream_t)stream;
  if (gin)
    hipLaunchKernelGGL(blur_axis_kernel<true>, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, gout, taps, gin, total,
                       len, stride, K);
  if (gtaps) {
    int64_t blocks = cdiv(total, 256 * 8);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(blur_taps_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, gout, gtaps, total, len, stride, K);
  }
  return launch_status("blur_bwd");
}

extern "C" int64_t svr_blur_axis_bwd_ordered_workspace(int32_t B, int32_t D0, int32_t D1, int32_t D2, int32_t K) {
  if (B <= 0 || D0 <= 0 || D1 <= 0 || D2 <= 0 || K <= 0) return (int64_t)sizeof(double);
  return taps_grad_blocks((int64_t)B * D0 * D1 * D2) * K * (int64_t)sizeof(double);
}

extern "C" int svr_blur_axis_bwd_ordered(const float *in, const float *taps, const float *gout, float *gin, double *gtaps,
                                         int32_t B, int32_t D0, int32_t D1, int32_t D2, int32_t axis, int32_t K,
                                         void *workspace, void *stream) {
  SVR_CHECK(in && taps && gout, SVR_E_BADARG, "blur_bwd_ordered: null pointer");
  SVR_CHECK(!gtaps || workspace, SVR_E_BADARG, "blur_bwd_ordered: the tap gradient needs a workspace");
  SVR_CHECK(K >= 1 && K <= KMAX && (K & 1), SVR_E_UNSUPPORTED, "blur_bwd_ordered: K=%d (odd, <= %d)", K, KMAX);
  int len;
  int64_t stride;
  if (int rc = axis_geometry(D0, D1, D2, axis, &len, &stride)) return rc;
  int64_t total = (int64_t)B * D0 * D1 * D2;
  if (total <= 0) return SVR_OK;
  hipStream_t s = (hipStream_t)stream;
  if (gin)
    hipLaunchKernelGGL(blur_axis_kernel<true>, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, gout, taps, gin, total,
                       len, stride, K);
  if (gtaps) {
    const int64_t blocks = taps_grad_blocks(total);
    hipLaunchKernelGGL(blur_taps_grad_parts_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, gout, (double *)workspace, total,
                       len, stride, K);
    hipLaunchKernelGGL(blur_taps_final_kernel, dim3((unsigned)K), dim3(64), 0, s, (const double *)workspace, gtaps, (int)blocks, K);
  }
  return launch_status("blur_bwd_ordered");
}
