// Mesh file writers (plain C++): the indexed .obj behind implicit_to_mesh / visualize_sdf (the reference's export_obj,
// util/visualize.py:23-25) and its form with `vn` lines, the point-list .obj of visualize_point_list (:14-20) and the binary PLY
// with vertex colours.
// Built with -ffp-contract=off: svr_write_obj_points adds 0.5 in float32, one rounding per operation.
#include "io_bytes.h"
#include <charconv>
#include <vector>

using namespace svr;

// `v` lines, with `normals` one `vn` line per vertex after them, then the faces: `f a b c`, or `f a//a b//b c//c` with normals
static int write_obj(const char *what, const char *path, const float *verts, const float *normals, int64_t nv, const int32_t *faces,
                     int64_t nf) {
  OutFile out(path);
  SVR_CHECK(out.f, SVR_E_IO, "%s: cannot open %s", what, path);
  std::vector<char> buf(1 << 20);
  size_t used = 0;
  auto flush = [&]() { out.write(buf.data(), 1, used); used = 0; };
  // %.9g: every float32 reads back exactly, also through a float64 parse and a cast
  auto rows = [&](const float *data, const char *tag) {
    for (int64_t i = 0; i < nv; ++i) {
      if (used + 64 > buf.size()) flush();
      char *c = buf.data() + used;
      char *end = buf.data() + buf.size();
      for (const char *t = tag; *t; ++t) *c++ = *t;
      for (int a = 0; a < 3; ++a) {
        *c++ = ' ';
        c = std::to_chars(c, end, data[i * 3 + a], std::chars_format::general, 9).ptr;
      }
      *c++ = '\n';
      used = c - buf.data();
    }
  };
  rows(verts, "v");
  if (normals) rows(normals, "vn");
  for (int64_t i = 0; i < nf; ++i) {
    if (used + 96 > buf.size()) flush();
    char *c = buf.data() + used;
    char *end = buf.data() + buf.size();
    *c++ = 'f';
    for (int a = 0; a < 3; ++a) {
      *c++ = ' ';
      c = std::to_chars(c, end, (int64_t)faces[i * 3 + a] + 1).ptr;
      if (normals) {
        *c++ = '/';
        *c++ = '/';
        c = std::to_chars(c, end, (int64_t)faces[i * 3 + a] + 1).ptr;
      }
    }
    *c++ = '\n';
    used = c - buf.data();
  }
  flush();
  SVR_CHECK(out.close(), SVR_E_IO, "%s: write to %s failed", what, path);
  return SVR_OK;
}

extern "C" int svr_write_obj(const char *path, const float *verts, int64_t nv, const int32_t *faces, int64_t nf) {
  SVR_CHECK(path && nv >= 0 && nf >= 0 && (verts || nv == 0) && (faces || nf == 0), SVR_E_BADARG, "write_obj: bad argument");
  return write_obj("write_obj", path, verts, nullptr, nv, faces, nf);
}

extern "C" int svr_write_obj_normals(const char *path, const float *verts, const float *normals, int64_t nv, const int32_t *faces,
                                     int64_t nf) {
  SVR_CHECK(path && nv >= 0 && nf >= 0 && ((verts && normals) || nv == 0) && (faces || nf == 0), SVR_E_BADARG,
            "write_obj_normals: bad argument");
  static const float none = 0.0f;                  // nv == 0: a non-null pointer that is never read selects the `//` form
  return write_obj("write_obj_normals", path, verts, normals ? normals : &none, nv, faces, nf);
}

extern "C" int svr_write_obj_points(const char *path, const float *pts, int64_t n) {
  SVR_CHECK(path && n >= 0 && (pts || n == 0), SVR_E_BADARG, "write_obj_points: bad argument");
  OutFile out(path);
  SVR_CHECK(out.f, SVR_E_IO, "write_obj_points: cannot open %s", path);
  for (int64_t i = 0; i < n && out.ok; ++i) {
    // + 0.5 in float32, widened for %f: the reference's '%f' % (x + 0.5) on a float32 coordinate
    const float x = pts[i * 3] + 0.5f, y = pts[i * 3 + 1] + 0.5f, z = pts[i * 3 + 2] + 0.5f;
    out.ok = fprintf(out.f, "v %f %f %f %f %f %f\n", (double)x, (double)y, (double)z, 1.0, 1.0, 1.0) > 0;
  }
  SVR_CHECK(out.close(), SVR_E_IO, "write_obj_points: write to %s failed", path);
  return SVR_OK;
}

extern "C" int svr_write_ply(const char *path, const float *verts, const uint8_t *colors, int64_t nv, const int32_t *faces, int64_t nf) {
  SVR_CHECK(path && nv >= 0 && nf >= 0 && ((verts && colors) || nv == 0) && (faces || nf == 0), SVR_E_BADARG, "write_ply: bad argument");
  OutFile out(path);
  SVR_CHECK(out.f, SVR_E_IO, "write_ply: cannot open %s", path);
  char header[512];
  const int hn = snprintf(header, sizeof(header),
                          "ply\nformat binary_little_endian 1.0\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\n"
                          "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %lld\n"
                          "property list uchar int vertex_indices\nend_header\n",
                          (long long)nv, (long long)nf);
  out.write(header, 1, (size_t)hn);
  // the host is little-endian x86-64: floats and ints go out as they lie in memory
  std::vector<unsigned char> buf;
  constexpr int64_t kChunk = 1 << 16;
  buf.resize((size_t)kChunk * 15);
  for (int64_t i0 = 0; out.ok && i0 < nv; i0 += kChunk) {
    const int64_t n = nv - i0 < kChunk ? nv - i0 : kChunk;
    for (int64_t i = 0; i < n; ++i) {
      memcpy(&buf[(size_t)i * 15], verts + (i0 + i) * 3, 12);
      memcpy(&buf[(size_t)i * 15 + 12], colors + (i0 + i) * 3, 3);
    }
    out.write(buf.data(), 15, (size_t)n);
  }
  for (int64_t i0 = 0; out.ok && i0 < nf; i0 += kChunk) {
    const int64_t n = nf - i0 < kChunk ? nf - i0 : kChunk;
    for (int64_t i = 0; i < n; ++i) {
      buf[(size_t)i * 13] = 3;
      memcpy(&buf[(size_t)i * 13 + 1], faces + (i0 + i) * 3, 12);
    }
    out.write(buf.data(), 13, (size_t)n);
  }
  SVR_CHECK(out.close(), SVR_E_IO, "write_ply: %s: write failed", path);
  return SVR_OK;
}
