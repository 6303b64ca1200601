// Workspace of the fused point-MLP tail (mlp_tail.hip): per layer (fc_1, fc_2) one amax line and the f16 hi / lo planes of
// W 2^s.  One layout function, run by the size query on a measuring cursor and by the launcher on the caller's buffer.
// Host-only and free of HIP (tests/host/mlp_tail_layout_driver.cpp builds it with a plain C++ compiler).
#pragma once
#include "workspace.h"

namespace svr {
constexpr int64_t kMlpTailHidden = 256;   // the only width the kernel is built for
struct MlpTailWs {
  uint32_t *amax[2];   // bit pattern of max |W| of fc_1 / fc_2 (w_amax_launch); a 256-byte line each
  uint16_t *planes[2]; // [k-step][hi / lo][row tile of 32][lane 64][8 halves] of fc_1 / fc_2
};
inline MlpTailWs mlp_tail_layout(WsCursor &c, int64_t hidden) {
  return {{c.take<uint32_t>(64), c.take<uint32_t>(64)}, {c.take<uint16_t>(2 * hidden * hidden), c.take<uint16_t>(2 * hidden * hidden)}};
}
}  // namespace svr
