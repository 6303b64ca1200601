// Marching-cubes case table, built from a rule at compile time (plain C++17 constexpr: the same object initialises the
// kernels' __constant__ copy and the host export svr_mc_case_table).
//
// Corner c of a cell has the offset (c & 1, c >> 1 & 1, c >> 2 & 1) along axes (0, 1, 2); case bit c is set iff
// corner c is inside.  Edge e = 4 * axis + (o_u | o_v << 1): `axis` is the edge's direction, u < v the two other axes
// and o_u, o_v the offsets of the edge along them.
//
// The rule (no typed-in table):
//   1. the crossing edges of a case are the cube edges with exactly one inside endpoint;
//   2. every cube face is walked counter-clockwise as seen from outside the cube.  A face edge is an "entry" if the walk
//      goes from an outside to an inside corner there, an "exit" if it goes from inside to outside.  Each entry is joined
//      to the next exit along the walk by one segment, directed entry -> exit.  A face with 2 crossing edges gets one
//      segment; an ambiguous face (4 crossing edges, inside corners on a diagonal) gets two, each cutting off one inside
//      corner.  The choice depends on the face's 4 signs only, so the two cells sharing a face always agree on it;
//   3. a crossing edge is an entry on one of its two faces and an exit on the other (the two walks run along it in
//      opposite directions), so the segments chain into closed loops;
//   4. each loop, taken from its smallest edge id, is fan-triangulated: (l0, l1, l2), (l0, l2, l3), ...  With segments
//      directed entry -> exit this winding has its normals pointing from inside to outside.  The apex l0 is the first
//      loop edge that does not lie on an ambiguous face whose two segments both belong to this loop: from such an
//      edge the fan would draw a diagonal inside the face, and the neighbouring cell can draw the same one (an edge
//      shared by 4 triangles).  Every loop of the 256 cases has an allowed apex.
#pragma once
#include <stdint.h>

namespace svr {
namespace mc {

constexpr int kMaxTris = 5;  // the rule never gives more (checked by tests/test_marching_cubes_cpu.py)

struct CaseTable {
  int8_t ntri[256];
  int8_t edge[256][16];  // 3 edge ids per triangle, -1 after the last
};

constexpr int edge_between(int c0, int c1) {  // c0, c1 differ in exactly one offset
  const int d = c0 ^ c1;
  const int a = d == 1 ? 0 : d == 2 ? 1 : 2;
  const int lo = c0 & c1;
  const int u = a == 0 ? 1 : 0, v = a == 2 ? 1 : 2;
  return 4 * a + ((lo >> u) & 1) + (((lo >> v) & 1) << 1);
}

constexpr CaseTable build_case_table() {
  CaseTable T{};
  const int uu[4] = {0, 1, 1, 0}, vv[4] = {0, 0, 1, 1};  // counter-clockwise in the (u, v) plane
  for (int cs = 0; cs < 256; ++cs) {
    int next[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    for (int a = 0; a < 3; ++a) {
      const int u = (a + 1) % 3, v = (a + 2) % 3;  // (u, v, a) is right-handed
      for (int s = 0; s < 2; ++s) {
        int q[4] = {0, 0, 0, 0};
        bool in[4] = {false, false, false, false};
        for (int n = 0; n < 4; ++n) {
          const int m = s ? n : (4 - n) % 4;  // the face at offset 0 looks along -axis: reversed walk
          q[n] = (s << a) | (uu[m] << u) | (vv[m] << v);
          in[n] = ((cs >> q[n]) & 1) != 0;
        }
        for (int n = 0; n < 4; ++n) {
          if (in[n] || !in[(n + 1) % 4]) continue;  // entry: outside -> inside
          int m = (n + 1) % 4;
          while (!(in[m] && !in[(m + 1) % 4])) m = (m + 1) % 4;  // next exit
          next[edge_between(q[n], q[(n + 1) % 4])] = edge_between(q[m], q[(m + 1) % 4]);
        }
      }
    }
    // loop id of every crossing edge
    int loop_of[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    int n_loops = 0;
    for (int e = 0; e < 12; ++e) {
      if (next[e] < 0 || loop_of[e] >= 0) continue;
      int x = e;
      do {
        loop_of[x] = n_loops;
        x = next[x];
      } while (x != e);
      ++n_loops;
    }
    // an ambiguous face whose two segments lie in ONE loop: a fan apex on one of its 4 edges would put a diagonal into
    // the face, and the cell on the other side can put the same diagonal there (an edge used by 4 triangles)
    bool no_apex[12] = {false, false, false, false, false, false, false, false, false, false, false, false};
    for (int a = 0; a < 3; ++a) {
      const int u = (a + 1) % 3, v = (a + 2) % 3;
      for (int s = 0; s < 2; ++s) {
        int fe[4] = {0, 0, 0, 0};
        for (int n = 0; n < 4; ++n) {
          const int c0 = (s << a) | (uu[n] << u) | (vv[n] << v);
          const int c1 = (s << a) | (uu[(n + 1) % 4] << u) | (vv[(n + 1) % 4] << v);
          fe[n] = edge_between(c0, c1);
        }
        if (loop_of[fe[0]] >= 0 && loop_of[fe[0]] == loop_of[fe[1]] && loop_of[fe[0]] == loop_of[fe[2]] &&
            loop_of[fe[0]] == loop_of[fe[3]])
          for (int n = 0; n < 4; ++n) no_apex[fe[n]] = true;
      }
    }
    bool used[12] = {false, false, false, false, false, false, false, false, false, false, false, false};
    int k = 0;
    for (int e = 0; e < 12; ++e) {
      if (next[e] < 0 || used[e]) continue;
      int loop[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      int len = 0;
      int x = e;
      do {
        used[x] = true;
        loop[len++] = x;
        x = next[x];
      } while (x != e);
      int r = 0;  // apex: the first loop edge (from the smallest id) that is allowed to be one
      while (r < len && no_apex[loop[r]]) ++r;
      if (r == len) r = 0;
      for (int t = 1; t + 1 < len; ++t) {
        T.edge[cs][k++] = (int8_t)loop[r];
        T.edge[cs][k++] = (int8_t)loop[(r + t) % len];
        T.edge[cs][k++] = (int8_t)loop[(r + t + 1) % len];
      }
    }
    T.ntri[cs] = (int8_t)(k / 3);
    for (; k < 16; ++k) T.edge[cs][k] = -1;
  }
  return T;
}

}  // namespace mc
}  // namespace svr
