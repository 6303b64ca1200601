// One layout per device workspace.  A workspace that is cut into more than one piece has exactly one layout function,
//   XWs x_layout(svr::WsCursor &c, shape...)   -- takes the pieces in order and returns their typed pointers (a braced
//                                                 list `return {c.take.., c.take..}` is evaluated left to right),
// and both sides run it: the exported size function on a measuring cursor (null base: every piece is null, only the
// offset moves), the launcher on the caller's buffer.  So the size and the carving cannot disagree.
// Host-only and free of HIP, so a plain C++ compiler can build it (tests/host/workspace_driver.cpp does).
#pragma once
#include <cstdint>

namespace svr {
class WsCursor {
 public:
  // Every exported size carries this much room for aligning the base, whatever alignment the site then applies.
  static constexpr int64_t kSlack = 256;
  // base = nullptr: measure.  base_align (a power of two, <= kSlack): 256 for most sites; 16 for the weight-plane
  // workspaces of the split GEMMs / convs; 1 where the launcher has always used the caller's pointer as it is.
  explicit WsCursor(const void *base = nullptr, int64_t base_align = 256)
      : base_(base ? (char *)round_up((int64_t)(uintptr_t)base, base_align) : nullptr) {}
  // The next piece: `count` elements of T, the cursor then advances by their bytes rounded up to piece_align.
  template <class T>
  T *take(int64_t count, int64_t piece_align = 256) {
    const int64_t at = off_;
    off_ += round_up(count * (int64_t)sizeof(T), piece_align);
    return base_ ? (T *)(base_ + at) : nullptr;   // no arithmetic on a null base
  }
  int64_t bytes() const { return off_ + kSlack; }   // what the caller allocates: the pieces and the base slack

 private:
  static int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
  char *base_;
  int64_t off_ = 0;
};
// The body of a size function: run the layout on a measuring cursor.
template <class Layout, class... Shape>
int64_t ws_measure(Layout layout, Shape... shape) {
  WsCursor c;
  layout(c, shape...);
  return c.bytes();
}
}  // namespace svr
