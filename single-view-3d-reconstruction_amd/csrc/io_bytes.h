// What the file-format units (io_*.cpp) share: byte-order readers and writers, the FILE holders and the exception guard of
// the C ABI.  Plain C++17; every entry point built on it takes host pointers only and needs no GPU.
#pragma once
#include "error.h"
#include <cstdio>
#include <cstring>
#include <exception>

namespace svr {

// little-endian reads; little- and big-endian writes
inline uint32_t rd16(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t rd32(const unsigned char *p) { return rd16(p) | (rd16(p + 2) << 16); }
inline uint64_t rd64(const unsigned char *p) { return (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32); }
inline void wr_le32(unsigned char *p, uint32_t v) { for (int i = 0; i < 4; ++i) p[i] = (unsigned char)(v >> (8 * i)); }
inline void wr_le64(unsigned char *p, uint64_t v) { for (int i = 0; i < 8; ++i) p[i] = (unsigned char)(v >> (8 * i)); }
inline void wr_be32(unsigned char *p, uint32_t v) { for (int i = 0; i < 4; ++i) p[i] = (unsigned char)(v >> (24 - 8 * i)); }

// a file opened for reading, closed on every way out (a null path opens nothing: the caller's null check names it)
struct File {
  FILE *f = nullptr;
  explicit File(const char *path) { f = path ? fopen(path, "rb") : nullptr; }
  ~File() { if (f) fclose(f); }
};

// a file being written: write() remembers the first failed fwrite, close() folds fclose's result in
struct OutFile {
  FILE *f = nullptr;
  bool ok = true;
  explicit OutFile(const char *path) { f = fopen(path, "wb"); }
  ~OutFile() { if (f) fclose(f); }
  void write(const void *p, size_t size, size_t n) { ok = ok && fwrite(p, size, n, f) == n; }
  bool close() { ok = (fclose(f) == 0) && ok; f = nullptr; return ok; }
};

// nothing throws across the ABI: std::bad_alloc / std::length_error / std::out_of_range from a malformed file are SVR_E_IO
template <typename F>
int io_guard(const char *what, F &&body) {
  try {
    return body();
  } catch (const std::exception &ex) {
    SVR_CHECK(false, SVR_E_IO, "%s: malformed file (%s)", what, ex.what());
  } catch (...) {
    SVR_CHECK(false, SVR_E_IO, "%s: malformed file", what);
  }
  return SVR_E_IO;
}

}  // namespace svr
