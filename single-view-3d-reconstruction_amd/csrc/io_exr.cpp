// OpenEXR subset reader / writer (plain C++ + zlib), next to the .df / .npz readers (io_df.cpp, io_npz.cpp).
//
// The reference opens a view's distance.exr through pyexr (data_processing/distance_to_depth.py:84, dataset/
// scene_net_data.py:77).  Read here: single-part scanline files, compression NONE / ZIPS / ZIP, pixel types HALF / FLOAT /
// UINT, any number of channels, lineOrder 0 and 1, any data-window origin.  Everything else (tiled, multi-part, deep,
// subsampled channels, RLE / PIZ / PXR24 / B44 / DWA) is refused by name.  The file is read into memory once and every
// access is checked against its size: a truncated file or a wild offset is an error, never a read outside the buffer.
//
// Layout: magic, version word (low byte 2; bit 9 tiled, bit 11 deep, bit 12 multi-part), attributes (name\0 type\0 int32
// size, payload) up to an empty name, one uint64 offset per scanline block, blocks (int32 y, int32 packed size, payload).
// A block holds 1 (NONE, ZIPS) or 16 (ZIP) scanlines; within a block the bytes go scanline by scanline, and within a
// scanline channel by channel in the file's (alphabetical) order.  A ZIP(S) payload is zlib-deflated after the bytes were
// split into even / odd halves and delta coded (t[i] = t[i-1] + d[i] - 128); a block that deflate did not shrink is
// stored raw (packed size == raw size).
#include "io_bytes.h"
#include <zlib.h>
#include <algorithm>
#include <string>
#include <vector>

using namespace svr;

namespace {

enum { PT_UINT = 0, PT_HALF = 1, PT_FLOAT = 2 };
const char *kCompression[] = {"NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB"};

float half_to_float(uint32_t h) {
  const uint32_t s = (h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 0x1fu, m = h & 0x3ffu, bits;
  if (e == 0) {
    if (m == 0) {
      bits = s;
    } else {  // subnormal half: m * 2^-24, normalised
      int sh = 0;
      while (!(m & 0x400u)) { m <<= 1; ++sh; }
      bits = s | ((uint32_t)(113 - sh) << 23) | ((m & 0x3ffu) << 13);
    }
  } else if (e == 31) {
    bits = s | 0x7f800000u | (m << 13);  // inf / NaN (payload kept)
  } else {
    bits = s | ((e + 112u) << 23) | (m << 13);
  }
  float f;
  memcpy(&f, &bits, 4);
  return f;
}

struct Channel {
  std::string name;
  int type = 0, xs = 1, ys = 1;
};

struct Exr {
  std::vector<unsigned char> b;
  int x0 = 0, y0 = 0, W = 0, H = 0, comp = 0, line_order = 0, lines = 1;
  std::vector<Channel> ch;
  size_t table = 0;
  int64_t nblocks = 0;
  bool has(size_t p, uint64_t n) const { return p <= b.size() && n <= b.size() - p; }
};

// a NUL-terminated string at p, not running past `end`: -> position behind the NUL, or 0
size_t cstring(const Exr &x, size_t p, size_t end, std::string &out) {
  size_t q = p;
  while (q < end && x.b[q] != 0) ++q;
  if (q >= end) return 0;
  out.assign((const char *)&x.b[p], q - p);
  return q + 1;
}

int exr_open(const char *path, Exr &x, const char *what) {
  SVR_CHECK(path, SVR_E_BADARG, "%s: null path", what);
  File fh(path);
  FILE *const f = fh.f;
  SVR_CHECK(f != nullptr, SVR_E_IO, "%s: cannot open %s", what, path);
  bool ok = fseek(f, 0, SEEK_END) == 0;
  const long size = ok ? ftell(f) : -1;
  ok = ok && size >= 0 && fseek(f, 0, SEEK_SET) == 0;
  if (ok) {
    x.b.resize((size_t)size);
    ok = fread(x.b.data(), 1, (size_t)size, f) == (size_t)size;
  }
  SVR_CHECK(ok, SVR_E_IO, "%s: cannot read %s", what, path);
  SVR_CHECK(x.b.size() >= 8 && rd32(&x.b[0]) == 20000630u, SVR_E_IO, "%s: %s: not an OpenEXR file (bad magic)", what, path);
  const uint32_t ver = rd32(&x.b[4]);
  SVR_CHECK(!(ver & 0x200u), SVR_E_UNSUPPORTED, "%s: %s: tiled files are not supported", what, path);
  SVR_CHECK(!(ver & 0x1000u), SVR_E_UNSUPPORTED, "%s: %s: multi-part files are not supported", what, path);
  SVR_CHECK(!(ver & 0x800u), SVR_E_UNSUPPORTED, "%s: %s: deep files are not supported", what, path);
  SVR_CHECK((ver & 0xffu) == 2, SVR_E_UNSUPPORTED, "%s: %s: file format version %u is not supported", what, path, ver & 0xffu);
  size_t p = 8;
  bool got_ch = false, got_comp = false, got_dw = false;
  for (;;) {
    SVR_CHECK(x.has(p, 1), SVR_E_IO, "%s: %s: truncated header", what, path);
    if (x.b[p] == 0) { ++p; break; }
    std::string name, type;
    p = cstring(x, p, x.b.size(), name);
    if (p) p = cstring(x, p, x.b.size(), type);
    SVR_CHECK(p && x.has(p, 4), SVR_E_IO, "%s: %s: truncated header", what, path);
    const int32_t sz = (int32_t)rd32(&x.b[p]);
    p += 4;
    SVR_CHECK(sz >= 0 && x.has(p, (uint64_t)sz), SVR_E_IO, "%s: %s: truncated header (attribute '%s')", what, path, name.c_str());
    const unsigned char *a = &x.b[p];
    if (name == "channels") {
      size_t q = p;
      const size_t end = p + (size_t)sz;
      for (;;) {
        SVR_CHECK(q < end, SVR_E_IO, "%s: %s: malformed channel list", what, path);
        if (x.b[q] == 0) break;
        Channel c;
        q = cstring(x, q, end, c.name);
        SVR_CHECK(q && q + 16 <= end, SVR_E_IO, "%s: %s: malformed channel list", what, path);
        c.type = (int32_t)rd32(&x.b[q]);
        c.xs = (int32_t)rd32(&x.b[q + 8]);
        c.ys = (int32_t)rd32(&x.b[q + 12]);
        q += 16;
        x.ch.push_back(c);
      }
      got_ch = true;
    } else if (name == "compression") {
      SVR_CHECK(sz == 1, SVR_E_IO, "%s: %s: malformed attribute 'compression'", what, path);
      x.comp = a[0];
      got_comp = true;
    } else if (name == "dataWindow") {
      SVR_CHECK(sz == 16, SVR_E_IO, "%s: %s: malformed attribute 'dataWindow'", what, path);
      const int64_t x0 = (int32_t)rd32(a), y0 = (int32_t)rd32(a + 4), x1 = (int32_t)rd32(a + 8), y1 = (int32_t)rd32(a + 12);
      SVR_CHECK(x1 >= x0 && y1 >= y0 && x1 - x0 < 65536 && y1 - y0 < 65536, SVR_E_IO, "%s: %s: implausible dataWindow (%ld,%ld)-(%ld,%ld)",
                what, path, (long)x0, (long)y0, (long)x1, (long)y1);
      x.x0 = (int)x0;
      x.y0 = (int)y0;
      x.W = (int)(x1 - x0 + 1);
      x.H = (int)(y1 - y0 + 1);
      got_dw = true;
    } else if (name == "lineOrder") {
      SVR_CHECK(sz == 1, SVR_E_IO, "%s: %s: malformed attribute 'lineOrder'", what, path);
      x.line_order = a[0];
    }
    p += (size_t)sz;
  }
  SVR_CHECK(got_ch && got_comp && got_dw, SVR_E_IO, "%s: %s: header lacks %s", what, path,
            !got_ch ? "'channels'" : (!got_comp ? "'compression'" : "'dataWindow'"));
  SVR_CHECK(!x.ch.empty() && x.ch.size() <= 1024, SVR_E_IO, "%s: %s: %zu channels", what, path, x.ch.size());
  SVR_CHECK(x.comp == 0 || x.comp == 2 || x.comp == 3, SVR_E_UNSUPPORTED, "%s: %s: compression %d (%s) is not supported", what, path,
            x.comp, x.comp < 10 ? kCompression[x.comp] : "unknown");
  SVR_CHECK(x.line_order == 0 || x.line_order == 1, SVR_E_UNSUPPORTED, "%s: %s: lineOrder %d is not supported", what, path, x.line_order);
  for (const Channel &c : x.ch) {
    SVR_CHECK(c.xs == 1 && c.ys == 1, SVR_E_UNSUPPORTED, "%s: %s: channel '%s' is subsampled (%d x %d): not supported", what, path,
              c.name.c_str(), c.xs, c.ys);
    SVR_CHECK(c.type >= 0 && c.type <= 2, SVR_E_UNSUPPORTED, "%s: %s: channel '%s' has unknown pixel type %d", what, path, c.name.c_str(),
              c.type);
  }
  x.lines = x.comp == 3 ? 16 : 1;
  x.nblocks = (x.H + x.lines - 1) / x.lines;
  x.table = p;
  SVR_CHECK(x.has(p, 8 * (uint64_t)x.nblocks), SVR_E_IO, "%s: %s: truncated offset table (%ld blocks)", what, path, (long)x.nblocks);
  return SVR_OK;
}

int exr_info_impl(const char *path, int32_t *width, int32_t *height, int32_t *origin, int32_t *n_channels, char *names,
                  int64_t names_bytes, int32_t *pixel_types, int32_t max_channels, int32_t *compression, int32_t *line_order) {
  Exr x;
  if (int rc = exr_open(path, x, "exr_info")) return rc;
  SVR_CHECK(width && height && origin && n_channels && compression && line_order, SVR_E_BADARG, "exr_info: null output");
  *width = x.W;
  *height = x.H;
  origin[0] = x.x0;
  origin[1] = x.y0;
  *n_channels = (int32_t)x.ch.size();
  *compression = x.comp;
  *line_order = x.line_order;
  if (names || pixel_types) {
    int64_t used = 0;
    SVR_CHECK((int64_t)x.ch.size() <= max_channels, SVR_E_BADSHAPE, "exr_info: %s has %zu channels, caller sized for %d", path,
              x.ch.size(), max_channels);
    for (size_t i = 0; i < x.ch.size(); ++i) {
      if (pixel_types) pixel_types[i] = x.ch[i].type;
      if (names) {
        const int64_t n = (int64_t)x.ch[i].name.size() + 1;
        SVR_CHECK(used + n <= names_bytes, SVR_E_BADSHAPE, "exr_info: %s: channel names need more than %ld bytes", path, (long)names_bytes);
        memcpy(names + used, x.ch[i].name.c_str(), (size_t)n);
        used += n;
      }
    }
  }
  return SVR_OK;
}

int exr_read_channel_impl(const char *path, const char *name, float *out, int64_t n) {
  Exr x;
  if (int rc = exr_open(path, x, "exr_read_channel")) return rc;
  SVR_CHECK(name && out, SVR_E_BADARG, "exr_read_channel: null argument");
  static const int kBytes[3] = {4, 2, 4};
  int ci = -1;
  int64_t line_bytes = 0, chan_off = 0;
  for (size_t i = 0; i < x.ch.size(); ++i) {
    if (ci < 0 && x.ch[i].name == name) {
      ci = (int)i;
      chan_off = line_bytes;
    }
    line_bytes += (int64_t)x.W * kBytes[x.ch[i].type];
  }
  SVR_CHECK(ci >= 0, SVR_E_NOTFOUND, "exr_read_channel: %s has no channel '%s'", path, name);
  SVR_CHECK(n == (int64_t)x.W * x.H, SVR_E_BADSHAPE, "exr_read_channel: %s holds %ld pixels, caller sized for %ld", path,
            (long)((int64_t)x.W * x.H), (long)n);
  const int type = x.ch[ci].type;
  std::vector<unsigned char> tmp, blk;
  std::vector<char> seen((size_t)x.nblocks, 0);
  for (int64_t k = 0; k < x.nblocks; ++k) {
    const uint64_t off = rd64(&x.b[x.table + 8 * (size_t)k]);
    SVR_CHECK(off <= x.b.size() && x.has((size_t)off, 8), SVR_E_IO, "exr_read_channel: %s: block %ld: offset %llu lies beyond the file (%zu bytes)",
              path, (long)k, (unsigned long long)off, x.b.size());
    const int64_t y = (int32_t)rd32(&x.b[off]), sz = (int32_t)rd32(&x.b[off + 4]);
    const int64_t rel = y - x.y0;
    SVR_CHECK(rel >= 0 && rel < x.H && rel % x.lines == 0, SVR_E_IO, "exr_read_channel: %s: block %ld: scanline %ld is no block start of the data window",
              path, (long)k, (long)y);
    SVR_CHECK(!seen[(size_t)(rel / x.lines)], SVR_E_IO, "exr_read_channel: %s: the block at scanline %ld appears twice", path, (long)y);
    seen[(size_t)(rel / x.lines)] = 1;
    const int64_t nl = std::min<int64_t>(x.lines, x.H - rel), raw = nl * line_bytes;
    SVR_CHECK(sz >= 0 && x.has((size_t)off + 8, (uint64_t)sz), SVR_E_IO, "exr_read_channel: %s: the block at scanline %ld is truncated (%ld bytes packed)",
              path, (long)y, (long)sz);
    SVR_CHECK(sz <= raw && (x.comp != 0 || sz == raw), SVR_E_IO, "exr_read_channel: %s: the block at scanline %ld packs %ld bytes, its raw size is %ld",
              path, (long)y, (long)sz, (long)raw);
    const unsigned char *src = &x.b[(size_t)off + 8];
    if (sz != raw) {
      tmp.resize((size_t)raw);
      blk.resize((size_t)raw);
      uLongf got = (uLongf)raw;
      const int zrc = uncompress(tmp.data(), &got, src, (uLong)sz);
      SVR_CHECK(zrc == Z_OK || zrc == Z_BUF_ERROR, SVR_E_IO, "exr_read_channel: %s: the block at scanline %ld: corrupt deflate stream", path, (long)y);
      SVR_CHECK(zrc == Z_OK && (int64_t)got == raw, SVR_E_IO, "exr_read_channel: %s: the block at scanline %ld: wrong inflated size (expected %ld bytes)",
                path, (long)y, (long)raw);
      for (int64_t i = 1; i < raw; ++i) tmp[(size_t)i] = (unsigned char)(tmp[(size_t)i - 1] + tmp[(size_t)i] - 128);
      const int64_t half = (raw + 1) / 2;
      for (int64_t i = 0; i < raw; ++i) blk[(size_t)i] = (i & 1) ? tmp[(size_t)(half + i / 2)] : tmp[(size_t)(i / 2)];
      src = blk.data();
    }
    for (int64_t l = 0; l < nl; ++l) {
      const unsigned char *p = src + l * line_bytes + chan_off;
      float *o = out + (rel + l) * x.W;
      if (type == PT_FLOAT) {
        memcpy(o, p, (size_t)x.W * 4);
      } else if (type == PT_HALF) {
        for (int i = 0; i < x.W; ++i) o[i] = half_to_float(rd16(p + 2 * i));
      } else {
        for (int i = 0; i < x.W; ++i) o[i] = (float)rd32(p + 4 * i);
      }
    }
  }
  return SVR_OK;
}

void put32(std::vector<unsigned char> &b, uint32_t v) { b.resize(b.size() + 4); wr_le32(&b[b.size() - 4], v); }
void put64(std::vector<unsigned char> &b, uint64_t v) { b.resize(b.size() + 8); wr_le64(&b[b.size() - 8], v); }
void put_str(std::vector<unsigned char> &b, const char *s) { b.insert(b.end(), s, s + strlen(s) + 1); }
void put_attr(std::vector<unsigned char> &b, const char *name, const char *type, const std::vector<unsigned char> &payload) {
  put_str(b, name);
  put_str(b, type);
  put32(b, (uint32_t)payload.size());
  b.insert(b.end(), payload.begin(), payload.end());
}
void put_f32(std::vector<unsigned char> &b, float f) { uint32_t u; memcpy(&u, &f, 4); put32(b, u); }

int exr_write_impl(const char *path, const float *data, int32_t H, int32_t W, const char *names, int32_t n_channels) {
  SVR_CHECK(path && data && names, SVR_E_BADARG, "exr_write: null argument");
  SVR_CHECK(H > 0 && W > 0 && H <= 65536 && W <= 65536 && n_channels > 0 && n_channels <= 1024, SVR_E_BADSHAPE,
            "exr_write: %d x %d pixels, %d channels", H, W, n_channels);
  std::vector<std::pair<std::string, int>> ch;  // (name, plane index), written in alphabetical order
  const char *s = names;
  for (int i = 0; i < n_channels; ++i) {
    const size_t len = strlen(s);
    SVR_CHECK(len > 0 && len < 256, SVR_E_BADARG, "exr_write: channel %d: a name has 1 to 255 characters", i);
    ch.emplace_back(std::string(s), i);
    s += len + 1;
  }
  std::sort(ch.begin(), ch.end());
  for (size_t i = 1; i < ch.size(); ++i)
    SVR_CHECK(ch[i].first != ch[i - 1].first, SVR_E_BADARG, "exr_write: channel '%s' given twice", ch[i].first.c_str());
  bool long_names = false;
  for (auto &c : ch) long_names = long_names || c.first.size() > 31;
  std::vector<unsigned char> b, a;
  put32(b, 20000630u);
  put32(b, 2u | (long_names ? 0x400u : 0u));
  for (auto &c : ch) {
    put_str(a, c.first.c_str());
    put32(a, PT_FLOAT);
    put32(a, 0);  // pLinear + 3 reserved bytes
    put32(a, 1);
    put32(a, 1);
  }
  a.push_back(0);
  put_attr(b, "channels", "chlist", a);
  put_attr(b, "compression", "compression", {0});
  a.clear();
  put32(a, 0); put32(a, 0); put32(a, (uint32_t)(W - 1)); put32(a, (uint32_t)(H - 1));
  put_attr(b, "dataWindow", "box2i", a);
  put_attr(b, "displayWindow", "box2i", a);
  put_attr(b, "lineOrder", "lineOrder", {0});
  a.clear();
  put_f32(a, 1.f);
  put_attr(b, "pixelAspectRatio", "float", a);
  put_attr(b, "screenWindowWidth", "float", a);
  a.clear();
  put_f32(a, 0.f); put_f32(a, 0.f);
  put_attr(b, "screenWindowCenter", "v2f", a);
  b.push_back(0);
  const uint64_t line = (uint64_t)W * 4 * ch.size(), first = b.size() + 8 * (uint64_t)H;
  for (int y = 0; y < H; ++y) put64(b, first + (uint64_t)y * (8 + line));
  OutFile out(path);
  SVR_CHECK(out.f != nullptr, SVR_E_IO, "exr_write: cannot open %s", path);
  out.write(b.data(), 1, b.size());
  for (int y = 0; y < H && out.ok; ++y) {
    b.clear();
    put32(b, (uint32_t)y);
    put32(b, (uint32_t)line);
    out.write(b.data(), 1, 8);
    for (size_t c = 0; c < ch.size(); ++c) out.write(data + ((int64_t)ch[c].second * H + y) * W, 4, (size_t)W);
  }
  SVR_CHECK(out.close(), SVR_E_IO, "exr_write: %s: write failed", path);
  return SVR_OK;
}

}  // namespace

extern "C" int svr_exr_info(const char *path, int32_t *width, int32_t *height, int32_t *origin, int32_t *n_channels, char *names,
                            int64_t names_bytes, int32_t *pixel_types, int32_t max_channels, int32_t *compression, int32_t *line_order) {
  return io_guard("exr_info", [&] {
    return exr_info_impl(path, width, height, origin, n_channels, names, names_bytes, pixel_types, max_channels, compression, line_order);
  });
}

extern "C" int svr_exr_read_channel(const char *path, const char *name, float *out, int64_t n) {
  return io_guard("exr_read_channel", [&] { return exr_read_channel_impl(path, name, out, n); });
}

extern "C" int svr_exr_write(const char *path, const float *data, int32_t H, int32_t W, const char *names, int32_t n_channels) {
  return io_guard("exr_write", [&] { return exr_write_impl(path, data, H, W, names, n_channels); });
}
