// Raw view -> what the trainers eat, device side (gfx950): the distance -> depth rule and the depth-grid marking of the
// reference's data_processing/distance_to_depth.py:11-27 and process_sample.py:17-21.
//
//   distance_to_depth : depth = sqrt(d*d / ((r*r + c*c) / (f*f) + 1)), r = row - H/2, c = col - W/2 (integer halves: the
//                       reference centres on the integers, not on cx / cy).  r*r + c*c is an integer sum converted to
//                       float32; each float32 operation is rounded on its own, in that order (-ffp-contract=off; hipcc's
//                       default division and sqrtf are correctly rounded), like torch's separate CPU ops.
//   depth_grid_mark   : (distance ->) depth -> grid-space coordinate (unproject_point of unproject.h, the function behind
//                       svr_unproject_fwd) -> rintf (round half to even = np.round) -> grid[i0][i1][i2] = 1.
// The marking writes plain byte stores of the constant 1: two pixels on one voxel race, and either order leaves the same
// byte.  A pixel whose rounded index leaves [0, dim) on any axis -- NaN / inf included, and the [-dim, 0) range numpy's
// indexing would wrap -- is not written; such pixels are counted (one integer atomic per wavefront that saw any).
// Elementwise, HBM bound: 76 800 pixels of a 320 x 240 view, one pass.
#include "common.h"
#include "unproject.h"

using namespace svr;

namespace {

__device__ __forceinline__ float distance_to_depth(float d, int row, int col, int H, int W, float f) {
  const int r = row - H / 2, c = col - W / 2;
  const float rc = (float)(r * r + c * c);
  return sqrtf(d * d / (rc / (f * f) + 1.f));
}

__global__ __launch_bounds__(256) void distance_to_depth_kernel(const float *__restrict__ distance, float *__restrict__ depth, int64_t total,
                                                                int H, int W, float f) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  depth[i] = distance_to_depth(distance[i], (int)((i / W) % H), (int)(i % W), H, W, f);
}

// rounded coordinate -> index, or -1 when it leaves [0, D) (NaN fails both comparisons)
__device__ __forceinline__ int voxel_index(float g, int D) {
  const float r = rintf(g);
  return (r >= 0.f && r <= (float)(D - 1)) ? (int)r : -1;
}

__global__ __launch_bounds__(256) void depth_grid_mark_kernel(const float *__restrict__ map, int is_distance, float focal, int H, int W,
                                                              UnprojConsts c, uint8_t *__restrict__ grid, int D0, int D1, int D2,
                                                              int32_t *__restrict__ out_of_range, float *__restrict__ coords) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < H * W;
  bool out = false;
  if (live) {
    const int row = i / W, col = i % W;
    float z = map[i];
    if (is_distance) z = distance_to_depth(z, row, col, H, W, focal);
    float gx, gy, gz;
    unproject_point(z, col, row, c, gx, gy, gz);
    if (coords) {
      coords[(int64_t)i * 3 + 0] = gx;
      coords[(int64_t)i * 3 + 1] = gy;
      coords[(int64_t)i * 3 + 2] = gz;
    }
    const int i0 = voxel_index(gx, D0), i1 = voxel_index(gy, D1), i2 = voxel_index(gz, D2);
    out = i0 < 0 || i1 < 0 || i2 < 0;
    if (!out) grid[((int64_t)i0 * D1 + i1) * D2 + i2] = 1;
  }
  const unsigned long long m = __ballot(out);
  if (m != 0 && (threadIdx.x & 63) == 0) atomicAdd(out_of_range, (int32_t)__popcll(m));
}

}  // namespace

extern "C" int svr_distance_to_depth(const float *distance, float *depth, int32_t B, int32_t H, int32_t W, float focal, void *stream) {
  SVR_CHECK(B >= 0 && H >= 0 && W >= 0, SVR_E_BADSHAPE, "distance_to_depth: %d x %d x %d", B, H, W);
  const int64_t total = (int64_t)B * H * W;
  if (total == 0) return SVR_OK;
  SVR_CHECK(distance && depth, SVR_E_BADARG, "distance_to_depth: null pointer");
  SVR_CHECK(H <= 32768 && W <= 32768 && cdiv(total, 256) < (1LL << 31), SVR_E_BADSHAPE, "distance_to_depth: %d x %d x %d", B, H, W);
  hipLaunchKernelGGL(distance_to_depth_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, distance, depth,
                     total, H, W, focal);
  return launch_status("distance_to_depth");
}

extern "C" int svr_depth_grid_mark(const float *map, int32_t is_distance, float focal, int32_t H, int32_t W, const float *consts,
                                   uint8_t *grid, int32_t D0, int32_t D1, int32_t D2, int32_t *out_of_range, float *coords,
                                   void *stream) {
  SVR_CHECK(map && consts && grid && out_of_range, SVR_E_BADARG, "depth_grid_mark: null pointer");
  SVR_CHECK(H > 0 && W > 0 && H <= 32768 && W <= 32768 && (int64_t)H * W < (1LL << 30), SVR_E_BADSHAPE, "depth_grid_mark: map %d x %d", H, W);
  SVR_CHECK(D0 > 0 && D1 > 0 && D2 > 0 && D0 < (1 << 20) && D1 < (1 << 20) && D2 < (1 << 20), SVR_E_BADSHAPE,
            "depth_grid_mark: grid %d x %d x %d", D0, D1, D2);
  hipLaunchKernelGGL(depth_grid_mark_kernel, dim3((unsigned)cdiv((int64_t)H * W, 256)), dim3(256), 0, (hipStream_t)stream, map,
                     is_distance, focal, H, W, unproj_consts(consts), grid, D0, D1, D2, out_of_range, coords);
  return launch_status("depth_grid_mark");
}
