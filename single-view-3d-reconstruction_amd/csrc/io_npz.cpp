// .npz member reader (plain C++ + zlib): zip central directory, stored or deflated members, zip64 local headers as numpy
// writes them, and the .npy header, straight into a caller buffer (the reference's np.load calls: sample_io's header).
#include "io_bytes.h"
#include <zlib.h>
#include <cstdlib>
#include <string>
#include <vector>

using namespace svr;

namespace {

struct ZipEntry {
  int method = -1;
  uint64_t comp = 0, uncomp = 0, local = 0;
};

// locate `name` in the zip's central directory (zip64 end record / extra fields handled)
int zip_find(FILE *f, const std::string &name, ZipEntry &e) {
  if (fseek(f, 0, SEEK_END)) return -1;
  const long size = ftell(f);
  const long tail = size < 65557 ? size : 65557;
  std::vector<unsigned char> buf((size_t)tail);
  if (fseek(f, size - tail, SEEK_SET) || fread(buf.data(), 1, (size_t)tail, f) != (size_t)tail) return -1;
  long eocd = -1;
  for (long i = tail - 22; i >= 0; --i)
    if (rd32(&buf[i]) == 0x06054b50u) { eocd = i; break; }
  if (eocd < 0) return -1;
  uint64_t n = rd16(&buf[eocd + 10]), cd_off = rd32(&buf[eocd + 16]), cd_size = rd32(&buf[eocd + 12]);
  if ((n == 0xFFFF || cd_off == 0xFFFFFFFFu || cd_size == 0xFFFFFFFFu) && eocd >= 20 && rd32(&buf[eocd - 20]) == 0x07064b50u) {
    const uint64_t z64 = rd64(&buf[eocd - 20 + 8]);  // zip64 end-of-central-directory record
    unsigned char r[56];
    if (fseek(f, (long)z64, SEEK_SET) || fread(r, 1, 56, f) != 56 || rd32(r) != 0x06064b50u) return -1;
    n = rd64(r + 32);
    cd_size = rd64(r + 40);
    cd_off = rd64(r + 48);
  }
  // a truncated or garbage file must not size an allocation or a seek: the directory lies inside the file
  if (cd_off > (uint64_t)size || cd_size > (uint64_t)size - cd_off) return -1;
  std::vector<unsigned char> cd((size_t)cd_size);
  if (fseek(f, (long)cd_off, SEEK_SET) || fread(cd.data(), 1, cd.size(), f) != cd.size()) return -1;
  size_t p = 0;
  for (uint64_t i = 0; i < n && p + 46 <= cd.size(); ++i) {
    if (rd32(&cd[p]) != 0x02014b50u) return -1;
    const int method = rd16(&cd[p + 10]);
    uint64_t comp = rd32(&cd[p + 20]), uncomp = rd32(&cd[p + 24]), local = rd32(&cd[p + 42]);
    const size_t nl = rd16(&cd[p + 28]), xl = rd16(&cd[p + 30]), cl = rd16(&cd[p + 32]);
    if (p + 46 + nl + xl + cl > cd.size()) return -1;  // entry runs past the directory
    const std::string fn((const char *)&cd[p + 46], nl);
    size_t x = p + 46 + nl;
    const size_t xend = x + xl;
    while (x + 4 <= xend) {  // zip64 extended information: only the fields that overflowed, in this order
      const int id = rd16(&cd[x]), sz = rd16(&cd[x + 2]);
      if (id == 1) {
        size_t q = x + 4;
        const size_t fend = x + 4 + (size_t)sz < xend ? x + 4 + (size_t)sz : xend;
        if (uncomp == 0xFFFFFFFFu) { if (q + 8 > fend) return -1; uncomp = rd64(&cd[q]); q += 8; }
        if (comp == 0xFFFFFFFFu) { if (q + 8 > fend) return -1; comp = rd64(&cd[q]); q += 8; }
        if (local == 0xFFFFFFFFu) { if (q + 8 > fend) return -1; local = rd64(&cd[q]); q += 8; }
      }
      x += 4 + (size_t)sz;
    }
    if (fn == name) {
      e.method = method;
      e.comp = comp;
      e.uncomp = uncomp;
      e.local = local;
      return 0;
    }
    p += 46 + nl + xl + cl;
  }
  return 1;  // not found
}

// read the member's bytes [skip, skip + want) of its UNCOMPRESSED stream into out
int zip_read(FILE *f, const ZipEntry &e, uint64_t skip, void *out, uint64_t want) {
  unsigned char lh[30];
  if (fseek(f, (long)e.local, SEEK_SET) || fread(lh, 1, 30, f) != 30 || rd32(lh) != 0x04034b50u) return -1;
  const long data = (long)e.local + 30 + rd16(lh + 26) + rd16(lh + 28);
  if (skip + want > e.uncomp) return -1;
  if (e.method == 0) {
    if (fseek(f, data + (long)skip, SEEK_SET) || fread(out, 1, (size_t)want, f) != (size_t)want) return -1;
    return 0;
  }
  if (e.method != 8) return -2;
  if (fseek(f, data, SEEK_SET)) return -1;
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (inflateInit2(&zs, -MAX_WBITS) != Z_OK) return -1;
  std::vector<unsigned char> in(1 << 16), scratch(1 << 16);
  uint64_t left_in = e.comp, produced = 0;
  int rc = Z_OK;
  while (produced < skip + want && rc != Z_STREAM_END) {
    if (zs.avail_in == 0 && left_in > 0) {
      const size_t take = (size_t)(left_in < in.size() ? left_in : in.size());
      if (fread(in.data(), 1, take, f) != take) { inflateEnd(&zs); return -1; }
      zs.next_in = in.data();
      zs.avail_in = (uInt)take;
      left_in -= take;
    }
    if (produced < skip) {  // header bytes in front of the payload: inflate into a scratch buffer
      const uint64_t room = skip - produced;
      zs.next_out = scratch.data();
      zs.avail_out = (uInt)(room < scratch.size() ? room : scratch.size());
    } else {
      const uint64_t room = skip + want - produced;
      zs.next_out = (unsigned char *)out + (produced - skip);
      zs.avail_out = (uInt)(room < (1u << 30) ? room : (1u << 30));
    }
    const uInt before = zs.avail_out;
    rc = inflate(&zs, Z_NO_FLUSH);
    if (rc != Z_OK && rc != Z_STREAM_END) { inflateEnd(&zs); return -1; }
    produced += before - zs.avail_out;
    if (before == zs.avail_out && zs.avail_in == 0 && left_in == 0) break;
  }
  inflateEnd(&zs);
  return produced >= skip + want ? 0 : -1;
}

struct NpyInfo {
  int dtype = -1;  // SVR_DT_*
  int ndim = 0, fortran = 0;
  int64_t shape[8] = {0};
  uint64_t header_bytes = 0;
};

int dtype_code(const std::string &descr) {
  if (descr == "<f4" || descr == "=f4") return SVR_DT_F32;
  if (descr == "<f8" || descr == "=f8") return SVR_DT_F64;
  if (descr == "|b1") return SVR_DT_BOOL;
  if (descr == "|u1") return SVR_DT_U8;
  if (descr == "<i4" || descr == "=i4") return SVR_DT_I32;
  if (descr == "<i8" || descr == "=i8") return SVR_DT_I64;
  return -1;
}

int dtype_size(int code) {
  switch (code) {
    case SVR_DT_F32: case SVR_DT_I32: return 4;
    case SVR_DT_F64: case SVR_DT_I64: return 8;
    case SVR_DT_BOOL: case SVR_DT_U8: return 1;
  }
  return 0;
}

// .npy header: magic, version, little-endian header length, python dict literal
int npy_parse(FILE *f, const ZipEntry &e, NpyInfo &info) {
  unsigned char h[12];
  const uint64_t first = e.uncomp < 12 ? e.uncomp : 12;
  if (first < 10 || zip_read(f, e, 0, h, first)) return -1;
  if (memcmp(h, "\x93NUMPY", 6) != 0) return -1;
  uint64_t hlen, pre;
  if (h[6] == 1) { hlen = rd16(h + 8); pre = 10; } else { if (first < 12) return -1; hlen = rd32(h + 8); pre = 12; }
  if (pre + hlen > e.uncomp || hlen > (1u << 20)) return -1;  // (numpy headers are a few hundred bytes)
  std::string d((size_t)hlen, '\0');
  if (zip_read(f, e, pre, &d[0], hlen)) return -1;
  info.header_bytes = pre + hlen;
  auto value_after = [&](const char *key) -> size_t {
    size_t k = d.find(key);
    if (k == std::string::npos) return k;
    k = d.find(':', k);
    return k == std::string::npos ? k : k + 1;
  };
  size_t p = value_after("'descr'");
  if (p == std::string::npos) return -1;
  size_t q0 = d.find('\'', p), q1 = q0 == std::string::npos ? q0 : d.find('\'', q0 + 1);
  if (q1 == std::string::npos) return -1;
  info.dtype = dtype_code(d.substr(q0 + 1, q1 - q0 - 1));
  p = value_after("'fortran_order'");
  if (p == std::string::npos) return -1;
  const size_t fo = d.find_first_not_of(' ', p);
  if (fo == std::string::npos) return -1;
  info.fortran = d.compare(fo, 4, "True") == 0;
  p = value_after("'shape'");
  if (p == std::string::npos) return -1;
  size_t a = d.find('(', p), b = d.find(')', a);
  if (a == std::string::npos || b == std::string::npos) return -1;
  info.ndim = 0;
  const char *s = d.c_str() + a + 1, *end = d.c_str() + b;
  while (s < end && info.ndim < 8) {
    while (s < end && (*s == ' ' || *s == ',')) ++s;
    if (s >= end) break;
    char *nx;
    info.shape[info.ndim++] = strtoll(s, &nx, 10);
    if (nx == s) return -1;
    s = nx;
  }
  return 0;
}

int open_member(const char *path, const char *member, File &fh, ZipEntry &e, NpyInfo &info, const char *what) {
  SVR_CHECK(path && member, SVR_E_BADARG, "%s: null argument", what);
  SVR_CHECK(fh.f != nullptr, SVR_E_IO, "%s: cannot open %s", what, path);
  int rc = zip_find(fh.f, std::string(member) + ".npy", e);
  SVR_CHECK(rc == 0, rc > 0 ? SVR_E_NOTFOUND : SVR_E_IO, "%s: %s has no member '%s'", what, path, member);
  SVR_CHECK(npy_parse(fh.f, e, info) == 0, SVR_E_IO, "%s: %s[%s]: malformed .npy header", what, path, member);
  SVR_CHECK(info.dtype >= 0, SVR_E_UNSUPPORTED, "%s: %s[%s]: unsupported dtype", what, path, member);
  return SVR_OK;
}

int npz_member_info_impl(const char *path, const char *member, int32_t *dtype, int32_t *ndim, int64_t *shape, int32_t *fortran_order) {
  File fh(path);
  ZipEntry e;
  NpyInfo info;
  if (int rc = open_member(path, member, fh, e, info, "npz_member_info")) return rc;
  SVR_CHECK(dtype && ndim && shape && fortran_order, SVR_E_BADARG, "npz_member_info: null output");
  *dtype = info.dtype;
  *ndim = info.ndim;
  *fortran_order = info.fortran;
  for (int i = 0; i < 8; ++i) shape[i] = i < info.ndim ? info.shape[i] : 0;
  return SVR_OK;
}

int npz_member_read_impl(const char *path, const char *member, void *out, int64_t nbytes) {
  File fh(path);
  ZipEntry e;
  NpyInfo info;
  if (int rc = open_member(path, member, fh, e, info, "npz_member_read")) return rc;
  int64_t count = 1;
  for (int i = 0; i < info.ndim; ++i) {
    SVR_CHECK(info.shape[i] >= 0 && (info.shape[i] == 0 || count <= (int64_t)(1LL << 56) / info.shape[i]), SVR_E_IO,
              "npz_member_read: %s[%s]: implausible shape", path, member);
    count *= info.shape[i];
  }
  SVR_CHECK(out && nbytes == count * dtype_size(info.dtype), SVR_E_BADSHAPE, "npz_member_read: %s[%s] holds %ld bytes, caller sized for %ld",
            path, member, (long)(count * dtype_size(info.dtype)), (long)nbytes);
  int rc = zip_read(fh.f, e, info.header_bytes, out, (uint64_t)nbytes);
  SVR_CHECK(rc == 0, rc == -2 ? SVR_E_UNSUPPORTED : SVR_E_IO, "npz_member_read: %s[%s]: %s", path, member,
            rc == -2 ? "unsupported zip compression method" : "read / inflate failed");
  return SVR_OK;
}

}  // namespace

extern "C" int svr_npz_member_info(const char *path, const char *member, int32_t *dtype, int32_t *ndim, int64_t *shape,
                                   int32_t *fortran_order) {
  return io_guard("npz_member_info", [&] { return npz_member_info_impl(path, member, dtype, ndim, shape, fortran_order); });
}

extern "C" int svr_npz_member_read(const char *path, const char *member, void *out, int64_t nbytes) {
  return io_guard("npz_member_read", [&] { return npz_member_read_impl(path, member, out, nbytes); });
}
