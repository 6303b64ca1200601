// Stand-alone check of csrc/mlp_tail_layout.h (the workspace of the fused point-MLP tail): measure it, carve it out of a heap
// block of exactly the measured size at several misalignments, and write every piece over its whole length.  Plain C++,
// nothing from ROCm.  Prints "ok <bytes> <carvings>"; tests/test_mlp_tail_cpu.py compares <bytes> with the library's size query.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mlp_tail_layout.h"

int main() {
  const int64_t hidden = svr::kMlpTailHidden;
  const int64_t bytes = svr::ws_measure(svr::mlp_tail_layout, hidden);
  const int64_t plane_bytes = 2 * hidden * hidden * (int64_t)sizeof(uint16_t);
  int carved = 0;
  const int misalign[5] = {0, 1, 16, 100, 255};
  for (int mis : misalign) {
    char *block = (char *)std::malloc((size_t)(bytes + 256));
    if (!block) return 2;
    // a base with the wanted misalignment against 256 bytes, and exactly `bytes` bytes behind it inside the block
    char *base = block + ((256 - (uintptr_t)block % 256) % 256 + mis) % 256;
    svr::WsCursor c(base);
    const svr::MlpTailWs ws = svr::mlp_tail_layout(c, hidden);
    if (c.bytes() != bytes) return 3;
    const struct { char *p; int64_t n; } piece[4] = {{(char *)ws.amax[0], 256}, {(char *)ws.amax[1], 256},
                                                      {(char *)ws.planes[0], plane_bytes}, {(char *)ws.planes[1], plane_bytes}};
    char *end = base;
    for (int i = 0; i < 4; ++i) {
      if (piece[i].p < end || (uintptr_t)piece[i].p % 256 != 0 || piece[i].p + piece[i].n > base + bytes) return 4;   // in order, aligned, inside
      std::memset(piece[i].p, 0xA5, (size_t)piece[i].n);
      end = piece[i].p + piece[i].n;
    }
    std::free(block);
    ++carved;
  }
  std::printf("ok %lld %d\n", (long long)bytes, carved);
  return 0;
}
