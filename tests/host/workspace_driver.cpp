// Stand-alone check of csrc/workspace.h (the only project header included): for a dozen piece lists the layout is measured
// on a null base, then carved out of a heap block of exactly bytes() bytes whose start is offset by 0, 1, 15, 16 and 255
// bytes from a 256-byte line, and every piece is written over its full length, element by element and as bytes.  Built
// plain and with -fsanitize=address,undefined by tests/test_workspace_cpu.py: a piece past the block, a misaligned element or
// arithmetic on a null base ends the sanitized run.  Prints "ok <cases> <carvings>"; any failed check is named on stderr.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "workspace.h"

namespace {
struct alignas(16) V16 { uint64_t a, b; };
struct Piece { int elem; int64_t count, align; };
struct Case { int64_t base_align; std::vector<Piece> pieces; };

int failures = 0;
#define EXPECT(cond, ...)                          \
  do {                                             \
    if (!(cond)) {                                 \
      std::fprintf(stderr, "FAILED %s: ", #cond);  \
      std::fprintf(stderr, __VA_ARGS__);           \
      std::fprintf(stderr, "\n");                  \
      ++failures;                                  \
    }                                              \
  } while (0)

template <class T>
char *take_as(svr::WsCursor &c, const Piece &p) {
  T *q = c.take<T>(p.count, p.align);
  if (q) {
    EXPECT((uintptr_t)q % alignof(T) == 0, "a piece of %d-byte elements at %p", p.elem, (void *)q);
    for (int64_t i = 0; i < p.count; ++i) q[i] = T{};   // a typed store per element: misalignment is UB the sanitizer names
    if (p.count) std::memset(q, 0xA5, (size_t)p.count * sizeof(T));
  }
  return (char *)q;
}
char *take(svr::WsCursor &c, const Piece &p) {
  switch (p.elem) {
    case 1: return take_as<uint8_t>(c, p);
    case 2: return take_as<uint16_t>(c, p);
    case 4: return take_as<uint32_t>(c, p);
    case 8: return take_as<uint64_t>(c, p);
    default: return take_as<V16>(c, p);
  }
}
int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
}  // namespace

int main() {
  const std::vector<Case> cases = {
      {256, {{4, 1000, 256}, {4, 1000, 256}, {1, 77, 256}}},
      {256, {{8, 0, 256}, {4, 1, 256}, {2, 0, 256}, {16, 3, 256}}},
      {256, {{1, 1, 256}, {1, 1, 256}, {1, 1, 256}}},
      {256, {{8, 257, 256}, {8, 257, 256}, {2, 257, 256}, {1, 12345, 256}}},                  // counts, offsets, flags, scan temp
      {16, {{2, 63 * 65, 2}, {2, 63 * 65, 2}}},                                              // two bf16 planes back to back
      {16, {{2, 3 * 64 * 129, 2}}},                                                          // three planes as one piece
      {256, {{4, 64, 256}, {2, 2 * 65 * 63, 2}}},                                            // |max| line, then two f16 planes
      {256, {{4, 64, 256}, {2, 4096, 2}, {16, 5, 256}, {16, 7, 16}, {1, 700, 1}}},           // line, planes, table, boxes, pad
      {16, {{16, 1, 16}, {8, 1, 8}, {4, 1, 4}, {2, 1, 2}, {1, 1, 1}}},
      {256, {}},
      {16, {{1, 0, 1}, {16, 0, 16}, {8, 1, 8}}},
      {256, {{4, 1, 256}, {8, 1, 256}, {16, 1, 256}, {1, 255, 256}, {1, 256, 256}, {1, 257, 256}}},
  };
  int carvings = 0;
  for (size_t k = 0; k < cases.size(); ++k) {
    const Case &cs = cases[k];
    svr::WsCursor m(nullptr, cs.base_align);
    int64_t want = svr::WsCursor::kSlack;
    for (const Piece &p : cs.pieces) {
      EXPECT(take(m, p) == nullptr, "case %zu: a measuring cursor returned a piece", k);
      want += round_up(p.elem * p.count, p.align);
    }
    const int64_t bytes = m.bytes();
    EXPECT(bytes == want, "case %zu: bytes() = %ld, the pieces and the slack add up to %ld", k, (long)bytes, (long)want);
    for (int64_t off : {0, 1, 15, 16, 255}) {
      void *raw = nullptr;
      if (posix_memalign(&raw, 256, (size_t)(off + bytes)) != 0) return 2;   // the block ends where the workspace ends
      char *base = (char *)raw + off, *end = base + bytes;
      char *aligned = (char *)round_up((int64_t)(uintptr_t)base, cs.base_align), *prev_end = aligned;
      svr::WsCursor c(base, cs.base_align);
      int64_t at = 0;
      for (const Piece &p : cs.pieces) {
        char *q = take(c, p);
        EXPECT(q == aligned + at, "case %zu, offset %ld: a piece at %+ld from the aligned base, expected %+ld", k, (long)off, (long)(q - aligned), (long)at);
        EXPECT(q >= prev_end, "case %zu, offset %ld: a piece starts inside the one before it", k, (long)off);
        prev_end = q + (int64_t)p.elem * p.count;
        at += round_up(p.elem * p.count, p.align);
      }
      EXPECT(prev_end <= end, "case %zu, offset %ld: the last piece ends %ld bytes past the workspace", k, (long)off, (long)(prev_end - end));
      EXPECT(c.bytes() == bytes, "case %zu, offset %ld: carving measured %ld bytes, measuring %ld", k, (long)off, (long)c.bytes(), (long)bytes);
      std::free(raw);
      ++carvings;
    }
  }
  if (failures) return 1;
  std::printf("ok %zu %d\n", cases.size(), carvings);
  return 0;
}
