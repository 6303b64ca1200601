// Depth -> grid-space point: the one device function behind svr_unproject_fwd (projection.hip) and the depth-grid marking
// of a raw sample (raw_sample.hip).  Include only from sources compiled with -ffp-contract=off: every float32 operation
// below is rounded on its own, in this order, like the reference's separate torch ops (model/projection.py:150-163,199-206).
#pragma once
#include <hip/hip_runtime.h>

namespace svr {

// f, cx, cy of the intrinsic; the diagonal and the offsets of camera2frustum; the grid dims (used by the normalisation only)
struct UnprojConsts {
  float f, cx, cy, s00, t0, s11, t1, s22, t2, d0, d1, d2;
};

// pixel (u = column, v = row) at depth z -> un-normalised grid-space coordinates
__device__ __forceinline__ void unproject_point(float z, int u, int v, const UnprojConsts &c, float &gx, float &gy, float &gz) {
  float X = ((float)u * z - c.cx * z) / c.f;
  float Y = -(((float)v * z - c.cy * z) / c.f);
  gx = c.s00 * X + c.t0;
  gy = c.s11 * Y + c.t1;
  gz = c.s22 * z + c.t2;
}

inline UnprojConsts unproj_consts(const float *k) {
  return UnprojConsts{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8], k[9], k[10], k[11]};
}

}  // namespace svr
