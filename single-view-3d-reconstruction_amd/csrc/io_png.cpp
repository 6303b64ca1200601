// 8-bit .png writers (plain C++ + zlib): grayscale behind visualize_depthmap (the reference goes through PIL,
// util/visualize.py:28-49) and RGB behind the mesh previews (util/mesh_render.py): signature, IHDR, one deflated IDAT with
// filter type 0 on every scanline, IEND.
#include "io_bytes.h"
#include <zlib.h>
#include <vector>

using namespace svr;

// length, type, payload, CRC-32 over type + payload
static void write_chunk(OutFile &out, const char *type, const unsigned char *data, uint32_t len) {
  unsigned char head[8], tail[4];
  wr_be32(head, len);
  memcpy(head + 4, type, 4);
  uLong crc = crc32(0L, head + 4, 4);
  if (len) crc = crc32(crc, data, len);
  wr_be32(tail, (uint32_t)crc);
  out.write(head, 1, 8);
  if (len) out.write(data, 1, len);
  out.write(tail, 1, 4);
}

// `channels` bytes per pixel: 1 = colour type 0 (grayscale), 3 = colour type 2 (RGB); `what` names the entry point in messages
static int write_png8(const char *what, const char *path, const uint8_t *data, int32_t H, int32_t W, int channels) {
  SVR_CHECK(path && data, SVR_E_BADARG, "%s: null pointer", what);
  SVR_CHECK(H > 0 && W > 0 && ((int64_t)W * channels + 1) * H < (1LL << 30), SVR_E_BADSHAPE, "%s: image %d x %d", what, H, W);
  // scanlines, each behind its filter-type byte 0 (None)
  const size_t line = (size_t)W * channels;
  std::vector<unsigned char> raw((line + 1) * H);
  for (int r = 0; r < H; ++r) {
    raw[(size_t)r * (line + 1)] = 0;
    memcpy(&raw[(size_t)r * (line + 1) + 1], data + (size_t)r * line, line);
  }
  uLongf zlen = compressBound((uLong)raw.size());
  std::vector<unsigned char> z(zlen);
  SVR_CHECK(compress2(z.data(), &zlen, raw.data(), (uLong)raw.size(), 6) == Z_OK, SVR_E_IO, "%s: deflate failed", what);
  OutFile out(path);
  SVR_CHECK(out.f, SVR_E_IO, "%s: cannot open %s", what, path);
  static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  unsigned char ihdr[13];
  wr_be32(ihdr, (uint32_t)W);
  wr_be32(ihdr + 4, (uint32_t)H);
  ihdr[8] = 8;                        // bit depth
  ihdr[9] = channels == 3 ? 2 : 0;    // colour type: RGB or grayscale
  ihdr[10] = 0;                       // compression: deflate
  ihdr[11] = 0;                       // filter method 0
  ihdr[12] = 0;                       // no interlace
  out.write(sig, 1, 8);
  write_chunk(out, "IHDR", ihdr, 13);
  write_chunk(out, "IDAT", z.data(), (uint32_t)zlen);
  write_chunk(out, "IEND", nullptr, 0);
  SVR_CHECK(out.close(), SVR_E_IO, "%s: write to %s failed", what, path);
  return SVR_OK;
}

extern "C" int svr_write_png_gray8(const char *path, const uint8_t *data, int32_t H, int32_t W) {
  return write_png8("write_png_gray8", path, data, H, W, 1);
}

extern "C" int svr_write_png_rgb8(const char *path, const uint8_t *data, int32_t H, int32_t W) {
  return write_png8("write_png_rgb8", path, data, H, W, 3);
}
