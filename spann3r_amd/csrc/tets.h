// The marching-tetrahedra rule of include/spann3r_hip.h ("TSDF fusion", sp3_tsdf_extract) as tables and helpers, shared by
// csrc/fusion.hip (the dense volume) and csrc/brick_mesh.hip (the brick pool) so that both extractions use one statement of it:
// the Kuhn cut, the 7 edge slots and the 16 cases of a tetrahedron (generated at compile time from the header's rule; no table is
// copied).  The colour channel's rounding, unorm8, comes with csrc/tsdf.h, which switches contraction off for itself and for what
// follows it.  Everything here is per translation unit (anonymous namespace).
#pragma once
#include "common.h"
#include "tsdf.h"

namespace {

// Cube corner code c = dx + 2 dy + 4 dz.  The six tetrahedra of the Kuhn cut around the diagonal 0-7, each listed with positive
// orientation, det(v1 - v0, v2 - v0, v3 - v0) > 0 (the header's table).
__device__ const signed char TET[6][4] = {{0, 1, 3, 7}, {0, 5, 1, 7}, {0, 3, 2, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 6, 4, 7}};
// slot of the edge whose endpoints differ by corner code c (1..7): +x, +y, +z, +x+y, +y+z, +x+z, +x+y+z
__device__ const signed char SLOT_OF[8] = {-1, 0, 1, 3, 2, 5, 4, 6};
__device__ const signed char SLOT_CODE[7] = {1, 2, 4, 3, 6, 5, 7};

struct Cases {
  signed char ntri[16];
  signed char e[16][2][3][2];      // [case][triangle][corner of the triangle] = the tetrahedron edge (vertex, vertex) it lies on
};

constexpr bool even4(int a, int b, int c, int d) {
  const int p[4] = {a, b, c, d};
  int inv = 0;
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j) inv += p[i] > p[j];
  return (inv & 1) == 0;
}

// The header's rule.  Bit m of the case = vertex m of the tetrahedron is inside.
constexpr Cases make_cases() {
  Cases t{};
  for (int c = 0; c < 16; ++c) {
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
    for (int m = 0; m < 4; ++m) {
      if ((c >> m) & 1) in[ni++] = m;
      else out[no++] = m;
    }
    if (ni == 0 || ni == 4) continue;
    if (ni == 2) {
      const int m = in[0], n = in[1];
      int q = out[0], r = out[1];
      if (!even4(m, n, q, r)) {
        const int s = q;
        q = r;
        r = s;
      }
      t.ntri[c] = 2;
      const int quad[4][2] = {{m, q}, {m, r}, {n, r}, {n, q}};
      const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
      for (int k = 0; k < 2; ++k)
        for (int x = 0; x < 3; ++x) {
          t.e[c][k][x][0] = (signed char)quad[pick[k][x]][0];
          t.e[c][k][x][1] = (signed char)quad[pick[k][x]][1];
        }
    } else {
      const int lone = ni == 1 ? in[0] : out[0];
      const int* rest = ni == 1 ? out : in;
      int a = rest[0], b = rest[1], d = rest[2];
      bool swap = !even4(lone, a, b, d);
      if (ni == 3) swap = !swap;      // the lone vertex is outside: the triangle turns round
      if (swap) {
        const int s = b;
        b = d;
        d = s;
      }
      t.ntri[c] = 1;
      const int o[3] = {a, b, d};
      for (int x = 0; x < 3; ++x) {
        t.e[c][0][x][0] = (signed char)lone;
        t.e[c][0][x][1] = (signed char)o[x];
      }
    }
  }
  return t;
}
__device__ const Cases CASES = make_cases();

}  // namespace
