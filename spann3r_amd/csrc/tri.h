// One face of an indexed triangle mesh, per translation unit: its corners, and the cross product of two edges in fp64 with its
// length (twice the area), which csrc/mesh_sample.hip weighs faces by and the searches over faces (csrc/mesh_distance.hip,
// csrc/mesh_ray.hip, csrc/mesh_bvh.hip) call a face usable by (has_area: > 0 and finite).  Every fp64 operation is rounded on its own (the block-scope pragma in edge_cross), whatever the including file sets.
#pragma once
#include "common.h"
#include <math.h>

namespace {

constexpr int NO_FACE = 0x7fffffff;      // "no winner yet" of the searches over faces (indices stay below it)

// the three indices and the nine coordinates of face f; false (nothing dereferenced beyond the indices) when one is outside 0..V-1
__device__ __forceinline__ bool load_face(const float* __restrict__ verts, int nverts, const int* __restrict__ faces, int64_t f, float (&v)[9],
                                          int (&abc)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) abc[k] = faces[3 * f + k];
  if (!((unsigned)abc[0] < (unsigned)nverts && (unsigned)abc[1] < (unsigned)nverts && (unsigned)abc[2] < (unsigned)nverts)) return false;
#pragma unroll
  for (int k = 0; k < 9; ++k) v[k] = verts[3 * (int64_t)abc[k / 3] + k % 3];
  return true;
}

__device__ __forceinline__ bool load_face(const float* __restrict__ verts, int nverts, const int* __restrict__ faces, int64_t f, float (&v)[9]) {
  int abc[3];
  return load_face(verts, nverts, faces, f, v, abc);
}

// corner A and the two edges B - A, C - A; e1 x e2 and its length
struct EdgeCross { double ax, ay, az, e1x, e1y, e1z, e2x, e2y, e2z, nx, ny, nz, d; };

__device__ __forceinline__ EdgeCross edge_cross(const float (&v)[9]) {
#pragma clang fp contract(off)
  EdgeCross r;
  r.ax = (double)v[0]; r.ay = (double)v[1]; r.az = (double)v[2];
  r.e1x = (double)v[3] - r.ax; r.e1y = (double)v[4] - r.ay; r.e1z = (double)v[5] - r.az;
  r.e2x = (double)v[6] - r.ax; r.e2y = (double)v[7] - r.ay; r.e2z = (double)v[8] - r.az;
  r.nx = r.e1y * r.e2z - r.e1z * r.e2y;
  r.ny = r.e1z * r.e2x - r.e1x * r.e2z;
  r.nz = r.e1x * r.e2y - r.e1y * r.e2x;
  r.d = sqrt(r.nx * r.nx + r.ny * r.ny + r.nz * r.nz);
  return r;
}
__device__ __forceinline__ bool is_finite(double d) { return d <= 1.7976931348623157e308; }      // false for NaN and +inf
// usable: the d > 0 of sp3_mesh_face_frames (rule 1 of "Mesh distance")
__device__ __forceinline__ bool has_area(const float (&v)[9]) { const double d = edge_cross(v).d; return d > 0.0 && is_finite(d); }

}  // namespace
