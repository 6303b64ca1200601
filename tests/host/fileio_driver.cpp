// Stand-alone driver of the file-format entry points (csrc/io_*.cpp + csrc/capi.cpp), built by tests/test_fileio_host.py with
// g++ -- plain, and with -fsanitize=address,undefined.  argv[1] is a manifest, one tab-separated job per line:
//   exr <class> <path>                          svr_exr_info, then svr_exr_read_channel for every channel it reports
//   npz <class> <path> <member>...              svr_npz_member_info / svr_npz_member_read for every named member
//   df  <class> <path>                          svr_df_dims / svr_df_read
//     <class>: ok  = intact: every call returns SVR_OK and the line `sum <path> <what> <crc32> <bytes>` is printed;
//              bad = damaged: no call that reads data (read_channel, member_read, df_read) may return SVR_OK;
//              any = may or may not still be readable.  Whatever the class, every return value is SVR_OK or one of the
//              library's negative codes.
//   obj / pts / ply / png / dfw / exrw <out> <inputs...>    one writer call each from raw little-endian input files
//   badargs <dir>                               the refusals the ctypes tests pin, printed as `arg <label> <rc>`
// Exit status 0: every rule held; 1: a rule was broken (the reason on stderr); 2: the manifest itself is wrong.
#include <zlib.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "svr_hip.h"

namespace {

int g_broken = 0;

void broken(const std::string &job, const char *what, int rc) {
  fprintf(stderr, "%s: %s (rc %d: %s)\n", job.c_str(), what, rc, svr_last_error());
  ++g_broken;
}

bool is_code(int rc) { return rc <= 0 && rc >= SVR_E_NOTFOUND; }

// one call's verdict against the file's class; `reads` = the call delivers data
void judge(const std::string &job, const std::string &cls, const char *call, int rc, bool reads) {
  if (!is_code(rc)) broken(job, (std::string(call) + " returned no code of the library").c_str(), rc);
  else if (cls == "ok" && rc != SVR_OK) broken(job, (std::string(call) + " failed on an intact file").c_str(), rc);
  else if (cls == "bad" && reads && rc == SVR_OK) broken(job, (std::string(call) + " accepted a damaged file").c_str(), rc);
}

void sum(const std::string &path, const std::string &what, const void *p, size_t bytes) {
  printf("sum\t%s\t%s\t%08lx\t%zu\n", path.c_str(), what.c_str(), crc32(0L, (const Bytef *)p, (uInt)bytes), bytes);
}

template <typename T>
std::vector<T> slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  std::string s((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(s.size() / sizeof(T));
  if (!v.empty()) memcpy(v.data(), s.data(), v.size() * sizeof(T));
  return v;
}

constexpr int64_t kMost = 1 << 26;  // values per read: far above every file of the sweep

void exr_job(const std::string &job, const std::string &cls, const std::string &path) {
  int32_t w = 0, h = 0, origin[2], nch = 0, comp = 0, order = 0;
  int rc = svr_exr_info(path.c_str(), &w, &h, origin, &nch, nullptr, 0, nullptr, 0, &comp, &order);
  judge(job, cls, "exr_info", rc, false);
  float one = 0.f;
  if (rc != SVR_OK) {  // the reader opens the file anew: it refuses it too
    rc = svr_exr_read_channel(path.c_str(), "R", &one, 1);
    judge(job, "bad", "exr_read_channel after a failed exr_info", rc, true);
    return;
  }
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  std::vector<char> names((size_t)f.tellg() + (size_t)nch + 1);  // the names lie in the file
  std::vector<int32_t> types((size_t)nch);
  rc = svr_exr_info(path.c_str(), &w, &h, origin, &nch, names.data(), (int64_t)names.size(), types.data(), nch, &comp, &order);
  judge(job, cls, "exr_info with names", rc, false);
  if (rc != SVR_OK) return;
  const int64_t n = (int64_t)w * h;
  if (n > kMost) return broken(job, "a data window larger than any file of the sweep", 0);
  std::vector<float> out((size_t)n);
  const char *name = names.data();
  for (int c = 0; c < nch; ++c, name += strlen(name) + 1) {
    rc = svr_exr_read_channel(path.c_str(), name, out.data(), n);
    judge(job, cls, "exr_read_channel", rc, true);
    if (cls == "ok" && rc == SVR_OK) sum(path, name, out.data(), out.size() * 4);
  }
}

void npz_job(const std::string &job, const std::string &cls, const std::vector<std::string> &a) {
  static const int kSize[6] = {4, 8, 1, 1, 4, 8};  // SVR_DT_*
  for (size_t m = 3; m < a.size(); ++m) {
    int32_t dtype = -1, ndim = 0, fortran = 0;
    int64_t shape[8];
    int rc = svr_npz_member_info(a[2].c_str(), a[m].c_str(), &dtype, &ndim, shape, &fortran);
    judge(job, cls, "npz_member_info", rc, false);
    int64_t count = 1;
    bool sized = rc == SVR_OK && dtype >= 0 && dtype < 6;
    for (int i = 0; sized && i < ndim; ++i) {
      sized = shape[i] >= 0 && (shape[i] == 0 || count <= kMost / shape[i]);
      if (sized) count *= shape[i];
    }
    if (!sized) {  // info refused the member, or it is larger than any file of the sweep: one byte is the wrong size for it
      char one = 0;
      rc = svr_npz_member_read(a[2].c_str(), a[m].c_str(), &one, 1);
      judge(job, "bad", "npz_member_read of an unsized member", rc, true);
      continue;
    }
    std::vector<char> out((size_t)(count * kSize[dtype]) + 1);  // + 1: never a null pointer for an empty member
    rc = svr_npz_member_read(a[2].c_str(), a[m].c_str(), out.data(), count * kSize[dtype]);
    judge(job, cls, "npz_member_read", rc, true);
    if (cls == "ok" && rc == SVR_OK) sum(a[2], a[m], out.data(), out.size() - 1);
  }
}

void df_job(const std::string &job, const std::string &cls, const std::string &path) {
  int64_t dims[3] = {0, 0, 0};
  int rc = svr_df_dims(path.c_str(), dims);
  judge(job, cls, "df_dims", rc, false);
  float one = 0.f;
  if (rc != SVR_OK || dims[0] * dims[1] * dims[2] > kMost) {  // (dims are below 2^20 each when df_dims accepts them)
    rc = svr_df_read(path.c_str(), &one, 1);
    judge(job, "bad", "df_read of an unsized file", rc, true);
    return;
  }
  std::vector<float> out((size_t)(dims[0] * dims[1] * dims[2]));
  rc = svr_df_read(path.c_str(), out.data(), (int64_t)out.size());
  judge(job, cls, "df_read", rc, true);
  if (cls == "ok" && rc == SVR_OK) sum(path, "payload", out.data(), out.size() * 4);
}

void arg(const char *label, int rc) { printf("arg\t%s\t%d\n", label, rc); }

// the refusals tests/test_*_cpu.py pin through ctypes, in the same words (tests/test_fileio_host.py: BAD_ARGS)
void badargs(const std::string &dir) {
  const std::string in_missing = dir + "/no_such_dir/x", ok_path = dir + "/badargs.out", absent = dir + "/absent.file";
  const char *gone = in_missing.c_str(), *ok = ok_path.c_str();
  const float v[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
  const int32_t f[3] = {0, 1, 2};
  const uint8_t c[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
  float out[4];
  int32_t i32[8];
  int64_t i64[8];
  arg("obj_missing_dir", svr_write_obj(gone, nullptr, 0, nullptr, 0));
  arg("obj_null_path", svr_write_obj(nullptr, v, 3, f, 1));
  arg("obj_null_verts", svr_write_obj(ok, nullptr, 3, f, 1));
  arg("obj_negative", svr_write_obj(ok, v, -1, f, 1));
  arg("pts_empty", svr_write_obj_points(ok, nullptr, 0));
  arg("pts_missing_dir", svr_write_obj_points(gone, nullptr, 0));
  arg("pts_null", svr_write_obj_points(ok, nullptr, 3));
  arg("pts_negative", svr_write_obj_points(ok, v, -1));
  arg("ply_missing_dir", svr_write_ply(gone, v, c, 3, f, 1));
  arg("ply_null_colors", svr_write_ply(ok, v, nullptr, 3, f, 1));
  arg("ply_null_path", svr_write_ply(nullptr, v, c, 3, f, 1));
  arg("png_zero_height", svr_write_png_gray8(ok, c, 0, 2));
  arg("png_negative_width", svr_write_png_gray8(ok, c, 2, -2));
  arg("png_null_data", svr_write_png_gray8(ok, nullptr, 2, 2));
  arg("png_missing_dir", svr_write_png_gray8(gone, c, 2, 2));
  arg("dfw_missing_dir", svr_df_write(gone, v, 1, 3, 3));
  arg("dfw_null_payload", svr_df_write(ok, nullptr, 1, 3, 3));
  arg("dfw_zero_extent", svr_df_write(ok, v, 0, 3, 3));
  arg("dfw_negative_extent", svr_df_write(ok, v, 3, -1, 3));
  arg("exrw_missing_dir", svr_exr_write(gone, v, 3, 3, "Z", 1));
  arg("exrw_null_data", svr_exr_write(ok, nullptr, 3, 3, "Z", 1));
  arg("exrw_zero_height", svr_exr_write(ok, v, 0, 3, "Z", 1));
  arg("exrw_no_channels", svr_exr_write(ok, v, 3, 3, "Z", 0));
  arg("exrw_name_twice", svr_exr_write(ok, v, 1, 1, "Z\0Z", 2));
  arg("exr_info_absent", svr_exr_info(absent.c_str(), i32, i32 + 1, i32 + 2, i32 + 4, nullptr, 0, nullptr, 0, i32 + 5, i32 + 6));
  arg("exr_info_null_path", svr_exr_info(nullptr, i32, i32 + 1, i32 + 2, i32 + 4, nullptr, 0, nullptr, 0, i32 + 5, i32 + 6));
  arg("exr_read_absent", svr_exr_read_channel(absent.c_str(), "R", out, 4));
  arg("exr_read_null_path", svr_exr_read_channel(nullptr, "R", out, 4));
  arg("npz_info_absent", svr_npz_member_info(absent.c_str(), "a", i32, i32 + 1, i64, i32 + 2));
  arg("npz_info_null_path", svr_npz_member_info(nullptr, "a", i32, i32 + 1, i64, i32 + 2));
  arg("npz_info_null_member", svr_npz_member_info(absent.c_str(), nullptr, i32, i32 + 1, i64, i32 + 2));
  arg("npz_read_absent", svr_npz_member_read(absent.c_str(), "a", out, 16));
  arg("npz_read_null_path", svr_npz_member_read(nullptr, "a", out, 16));
  arg("df_dims_absent", svr_df_dims(absent.c_str(), i64));
  arg("df_dims_null_path", svr_df_dims(nullptr, i64));
  arg("df_dims_null_dims", svr_df_dims(absent.c_str(), nullptr));
  arg("df_read_absent", svr_df_read(absent.c_str(), out, 4));
  arg("df_read_null_path", svr_df_read(nullptr, out, 4));
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream manifest(argv[1]);
  if (!manifest) return 2;
  std::string line;
  while (std::getline(manifest, line)) {
    std::vector<std::string> a;
    std::stringstream ss(line);
    for (std::string field; std::getline(ss, field, '\t');) a.push_back(field);
    if (a.empty()) continue;
    const std::string &k = a[0];
    auto num = [&](size_t i) { return strtoll(a[i].c_str(), nullptr, 10); };
    int rc = SVR_OK;
    if (k == "exr" && a.size() == 3) exr_job(line, a[1], a[2]);
    else if (k == "npz" && a.size() >= 4) npz_job(line, a[1], a);
    else if (k == "df" && a.size() == 3) df_job(line, a[1], a[2]);
    else if (k == "badargs" && a.size() == 2) badargs(a[1]);
    else if (k == "obj" && a.size() == 6) rc = svr_write_obj(a[1].c_str(), slurp<float>(a[2]).data(), num(3), slurp<int32_t>(a[4]).data(), num(5));
    else if (k == "pts" && a.size() == 4) rc = svr_write_obj_points(a[1].c_str(), slurp<float>(a[2]).data(), num(3));
    else if (k == "ply" && a.size() == 7)
      rc = svr_write_ply(a[1].c_str(), slurp<float>(a[2]).data(), slurp<uint8_t>(a[3]).data(), num(4), slurp<int32_t>(a[5]).data(), num(6));
    else if (k == "png" && a.size() == 5) rc = svr_write_png_gray8(a[1].c_str(), slurp<uint8_t>(a[2]).data(), (int32_t)num(3), (int32_t)num(4));
    else if (k == "dfw" && a.size() == 6) rc = svr_df_write(a[1].c_str(), slurp<float>(a[2]).data(), num(3), num(4), num(5));
    else if (k == "exrw" && a.size() == 7) {
      std::string names = a[5];  // comma separated in the manifest, NUL separated for the library
      for (char &ch : names) ch = ch == ',' ? '\0' : ch;
      rc = svr_exr_write(a[1].c_str(), slurp<float>(a[2]).data(), (int32_t)num(3), (int32_t)num(4), names.c_str(), (int32_t)num(6));
    } else {
      fprintf(stderr, "bad manifest line: %s\n", line.c_str());
      return 2;
    }
    if (rc != SVR_OK) broken(line, "the writer failed", rc);
  }
  return g_broken ? 1 : 0;
}
