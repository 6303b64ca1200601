// The ray caster's pair routine: one ray against one triangle (include/svr_hip.h, svr_raycast_*, line by line).  Plain
// C++ with no HIP type in its interface, so the same function compiles for the device (every kernel of raycast.hip
// calls it) and for the host (tests/test_raycast_cpu.py builds a stand-alone program around it with g++).  Include only
// from sources compiled with -ffp-contract=off: every float64 operation below is rounded on its own, in this order.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SVR_RAY_HD __host__ __device__ inline
#else
#define SVR_RAY_HD inline
#endif

namespace svr {

SVR_RAY_HD double ray_dot3(double ux, double uy, double uz, double vx, double vy, double vz) { return (ux * vx + uy * vy) + uz * vz; }

// Direction per unit depth of the ray through pixel (u = column, v = row); k: the 12 constants, widened by the caller
SVR_RAY_HD void ray_direction(int u, int v, double f, double cx, double cy, double s00, double s11, double s22, double *d) {
  d[0] = s00 * (((double)u - cx) / f);
  d[1] = -(s11 * (((double)v - cy) / f));
  d[2] = s22;
}

// Moeller-Trumbore, two-sided.  o: origin, d: direction per unit depth, t: a, b, c of the face (9 values).
// true: the ray hits the face at depth *z with near < z <= far; false: *z is not written.  Every comparison is false
// for NaN, so a NaN anywhere rejects the pair.
SVR_RAY_HD bool ray_triangle(const double *o, const double *d, const double *t, double near, double far, double *z) {
  const double e1x = t[3] - t[0], e1y = t[4] - t[1], e1z = t[5] - t[2];
  const double e2x = t[6] - t[0], e2y = t[7] - t[1], e2z = t[8] - t[2];
  const double px = d[1] * e2z - d[2] * e2y, py = d[2] * e2x - d[0] * e2z, pz = d[0] * e2y - d[1] * e2x;
  const double det = ray_dot3(e1x, e1y, e1z, px, py, pz);
  if (det == 0.0) return false;  // edge-on, zero area
  const double inv = 1.0 / det;
  const double sx = o[0] - t[0], sy = o[1] - t[1], sz = o[2] - t[2];
  const double bu = ray_dot3(sx, sy, sz, px, py, pz) * inv;
  if (!(bu >= 0.0 && bu <= 1.0)) return false;
  const double qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
  const double bv = ray_dot3(d[0], d[1], d[2], qx, qy, qz) * inv;
  if (!(bv >= 0.0 && bu + bv <= 1.0)) return false;
  const double zz = ray_dot3(e2x, e2y, e2z, qx, qy, qz) * inv;
  if (!(near < zz && zz <= far)) return false;
  *z = zz;
  return true;
}

// Unit normal of the face turned against the ray: m = (e1 x e2) / |e1 x e2| per component, negated when m . d > 0
SVR_RAY_HD void ray_facing_normal(const double *d, const double *t, double *m) {
  const double e1x = t[3] - t[0], e1y = t[4] - t[1], e1z = t[5] - t[2];
  const double e2x = t[6] - t[0], e2y = t[7] - t[1], e2z = t[8] - t[2];
  const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const double len = sqrt(ray_dot3(nx, ny, nz, nx, ny, nz));
  m[0] = nx / len, m[1] = ny / len, m[2] = nz / len;
  if (ray_dot3(m[0], m[1], m[2], d[0], d[1], d[2]) > 0.0) m[0] = -m[0], m[1] = -m[1], m[2] = -m[2];
}

}  // namespace svr
