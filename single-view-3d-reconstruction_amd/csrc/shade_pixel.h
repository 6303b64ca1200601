// The mesh shader's pixel routine: one pixel of the ray caster's face map -> three bytes (include/svr_hip.h, svr_mesh_shade,
// line by line).  Like raycast_pair.h, which it builds on: plain C++ with no HIP type in its interface, so the same function
// compiles for the device (mesh_shade.hip calls it, one thread per pixel) and for the host (tests/test_mesh_render_cpu.py
// builds a stand-alone program around it with g++).  Include only from sources compiled with -ffp-contract=off: every float64
// operation below is rounded on its own, in this order.
#pragma once
#include "raycast_pair.h"
#include <cstdint>

namespace svr {

// rint(x), half to even, clamped to [0, 255]; NaN gives 0
SVR_RAY_HD uint8_t shade_byte(double x) {
  const double r = rint(x);
  if (!(r >= 0.0)) return 0;
  return (uint8_t)(r > 255.0 ? 255.0 : r);
}

// k: f, cx, cy, s00, t0, s11, t1, s22, t2 widened to float64.  tri (F, 9), faces (F, 3) (read only with normals or colors),
// normals (V, 3) or null, colors (V, 3) or null; albedo, background: 3 bytes each.  Writes rgb[0..2].
SVR_RAY_HD void shade_pixel(int u, int v, int32_t face, const double *tri, const int32_t *faces, int64_t F, int64_t V, const float *normals,
                            const uint8_t *colors, const double *k, const uint8_t *albedo, const uint8_t *background, double ambient,
                            uint8_t *rgb) {
  rgb[0] = background[0], rgb[1] = background[1], rgb[2] = background[2];
  if (face < 0 || (int64_t)face >= F) return;      // a miss, or no face of this mesh: never turned into an address
  double d[3];
  ray_direction(u, v, k[0], k[1], k[2], k[3], k[5], k[7], d);
  const double *t = tri + (int64_t)face * 9;
  // bu, bv by the very expressions of ray_triangle
  const double e1x = t[3] - t[0], e1y = t[4] - t[1], e1z = t[5] - t[2];
  const double e2x = t[6] - t[0], e2y = t[7] - t[1], e2z = t[8] - t[2];
  const double px = d[1] * e2z - d[2] * e2y, py = d[2] * e2x - d[0] * e2z, pz = d[0] * e2y - d[1] * e2x;
  const double det = ray_dot3(e1x, e1y, e1z, px, py, pz);
  if (det == 0.0) return;                          // cannot be a face the caster accepted
  const double inv = 1.0 / det;
  const double sx = k[4] - t[0], sy = k[6] - t[1], sz = k[8] - t[2];
  const double bu = ray_dot3(sx, sy, sz, px, py, pz) * inv;
  const double qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
  const double bv = ray_dot3(d[0], d[1], d[2], qx, qy, qz) * inv;
  const double w0 = (1.0 - bu) - bv;
  // the three vertices, when an attribute needs them; an index that is no vertex must not become an address
  int64_t i0 = 0, i1 = 0, i2 = 0;
  bool corners = false;
  if (normals || colors) {
    i0 = faces[(int64_t)face * 3 + 0], i1 = faces[(int64_t)face * 3 + 1], i2 = faces[(int64_t)face * 3 + 2];
    corners = i0 >= 0 && i1 >= 0 && i2 >= 0 && i0 < V && i1 < V && i2 < V;
  }
  double n[3];
  bool smooth = false;
  if (normals && corners) {
    const float *n0 = normals + i0 * 3, *n1 = normals + i1 * 3, *n2 = normals + i2 * 3;
    for (int a = 0; a < 3; ++a) n[a] = (w0 * (double)n0[a] + bu * (double)n1[a]) + bv * (double)n2[a];
    const double len = sqrt(ray_dot3(n[0], n[1], n[2], n[0], n[1], n[2]));
    if (len > 0.0) {                               // false for NaN
      n[0] = n[0] / len, n[1] = n[1] / len, n[2] = n[2] / len;
      smooth = true;
    }
  }
  if (!smooth) ray_facing_normal(d, t, n);
  // head light, two-sided
  const double c = fabs(ray_dot3(n[0], n[1], n[2], d[0], d[1], d[2])) / sqrt(ray_dot3(d[0], d[1], d[2], d[0], d[1], d[2]));
  const double I = ambient + (1.0 - ambient) * c;
  for (int a = 0; a < 3; ++a) {
    double base = (double)albedo[a];
    if (colors && corners) base = (w0 * (double)colors[i0 * 3 + a] + bu * (double)colors[i1 * 3 + a]) + bv * (double)colors[i2 * 3 + a];
    rgb[a] = shade_byte(base * I);
  }
}

}  // namespace svr
