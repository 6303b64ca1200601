// .df reader and writer (plain C++): 3 x uint64 dims + float32 payload, x fastest (the reference's read_df, data_processing/
// volume_reader.py:36-45); the header is checked and the payload goes into a caller buffer (pinned memory) with one fread.
#include "io_bytes.h"

using namespace svr;

extern "C" int svr_df_dims(const char *path, int64_t *dims) {
  SVR_CHECK(path && dims, SVR_E_BADARG, "df_dims: null argument");
  File fh(path);
  SVR_CHECK(fh.f != nullptr, SVR_E_IO, "df_dims: cannot open %s", path);
  unsigned char h[24];
  SVR_CHECK(fread(h, 1, 24, fh.f) == 24, SVR_E_IO, "df_dims: %s: short header", path);
  for (int a = 0; a < 3; ++a) dims[a] = (int64_t)rd64(h + 8 * a);
  SVR_CHECK(dims[0] > 0 && dims[1] > 0 && dims[2] > 0 && dims[0] < (1 << 20) && dims[1] < (1 << 20) && dims[2] < (1 << 20), SVR_E_IO,
            "df_dims: %s: implausible dims %ld x %ld x %ld", path, (long)dims[0], (long)dims[1], (long)dims[2]);
  return SVR_OK;
}

extern "C" int svr_df_read(const char *path, float *payload, int64_t n) {
  int64_t dims[3];
  if (int rc = svr_df_dims(path, dims)) return rc;
  SVR_CHECK(payload && n == dims[0] * dims[1] * dims[2], SVR_E_BADSHAPE, "df_read: %s holds %ld values, caller sized for %ld", path,
            (long)(dims[0] * dims[1] * dims[2]), (long)n);
  File fh(path);
  SVR_CHECK(fh.f != nullptr && fseek(fh.f, 24, SEEK_SET) == 0, SVR_E_IO, "df_read: cannot open %s", path);
  SVR_CHECK(fread(payload, sizeof(float), (size_t)n, fh.f) == (size_t)n, SVR_E_IO, "df_read: %s: truncated payload", path);  // like the reference's `raise Exception`
  return SVR_OK;
}

extern "C" int svr_df_write(const char *path, const float *payload, int64_t X, int64_t Y, int64_t Z) {
  SVR_CHECK(path && payload, SVR_E_BADARG, "df_write: null argument");
  SVR_CHECK(X > 0 && Y > 0 && Z > 0 && X < (1 << 20) && Y < (1 << 20) && Z < (1 << 20), SVR_E_BADARG,
            "df_write: dims %ld x %ld x %ld (svr_df_dims reads extents in [1, 2^20))", (long)X, (long)Y, (long)Z);
  OutFile out(path);
  SVR_CHECK(out.f != nullptr, SVR_E_IO, "df_write: cannot open %s", path);
  unsigned char h[24];
  wr_le64(h, (uint64_t)X), wr_le64(h + 8, (uint64_t)Y), wr_le64(h + 16, (uint64_t)Z);
  out.write(h, 1, 24);
  out.write(payload, sizeof(float), (size_t)(X * Y * Z));
  SVR_CHECK(out.close(), SVR_E_IO, "df_write: %s: write failed", path);
  return SVR_OK;
}
