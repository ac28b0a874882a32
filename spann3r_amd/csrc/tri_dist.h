// The rule of one (query, face) pair of "Mesh distance" (include/spann3r_hip.h), per translation unit: Ericson's closest point on a
// triangle by Voronoi region in fp64, and the four outputs of a query for its winning face.  csrc/mesh_distance.hip (the grid and the
// brute-force kernels) and csrc/mesh_bvh.hip (the tree) evaluate faces with these very functions, so a face gives the same bits
// whichever structure reaches it.  Every fp64 operation is rounded on its own (the block-scope pragma in each body), whatever the
// including file sets.
#pragma once
#include "tri.h"

namespace {

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
  const double s = ax * bx + ay * by;
  return s + az * bz;
}

// Closest point of the triangle v (A, B, C) to p and its squared distance; regions in the header's order.
__device__ __forceinline__ double closest_on_face(double px, double py, double pz, const float* v, double& qx, double& qy, double& qz, int& region) {
#pragma clang fp contract(off)
  const double ax = (double)v[0], ay = (double)v[1], az = (double)v[2];
  const double bx = (double)v[3], by = (double)v[4], bz = (double)v[5];
  const double cx = (double)v[6], cy = (double)v[7], cz = (double)v[8];
  const double abx = bx - ax, aby = by - ay, abz = bz - az;
  const double acx = cx - ax, acy = cy - ay, acz = cz - az;
  const double apx = px - ax, apy = py - ay, apz = pz - az;
  const double bpx = px - bx, bpy = py - by, bpz = pz - bz;
  const double cpx = px - cx, cpy = py - cy, cpz = pz - cz;
  const double d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
  const double d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
  const double d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
  const double vc = d1 * d4 - d3 * d2;
  const double vb = d5 * d2 - d1 * d6;
  const double va = d3 * d6 - d5 * d4;
  const double e = d4 - d3, g = d5 - d6;
  if (d1 <= 0.0 && d2 <= 0.0) {
    region = 0; qx = ax; qy = ay; qz = az;
  } else if (d3 >= 0.0 && d4 <= d3) {
    region = 1; qx = bx; qy = by; qz = bz;
  } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    const double t = d1 / (d1 - d3);
    region = 2; qx = ax + t * abx; qy = ay + t * aby; qz = az + t * abz;
  } else if (d6 >= 0.0 && d5 <= d6) {
    region = 3; qx = cx; qy = cy; qz = cz;
  } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    const double t = d2 / (d2 - d6);
    region = 4; qx = ax + t * acx; qy = ay + t * acy; qz = az + t * acz;
  } else if (va <= 0.0 && e >= 0.0 && g >= 0.0) {
    const double t = e / (e + g);
    region = 5; qx = bx + t * (cx - bx); qy = by + t * (cy - by); qz = bz + t * (cz - bz);
  } else {
    const double den = 1.0 / ((va + vb) + vc);
    const double s = vb * den, t = vc * den;
    region = 6; qx = ax + (abx * s + acx * t); qy = ay + (aby * s + acy * t); qz = az + (abz * s + acz * t);
  }
  const double dx = px - qx, dy = py - qy, dz = pz - qz;
  return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ double dist2_to_face(double px, double py, double pz, const float* v) {
#pragma clang fp contract(off)
  double qx, qy, qz;
  int region;
  return closest_on_face(px, py, pz, v, qx, qy, qz, region);
}

// the four outputs of query qi for the winning face f (NO_FACE or anything unusable: the "no usable face" outputs)
__device__ __forceinline__ void write_result(const float* __restrict__ verts, int nverts, const int* __restrict__ faces, int nfaces, int64_t qi,
                                             float px, float py, float pz, int f, float* __restrict__ dist, float* __restrict__ closest,
                                             int* __restrict__ face, uint8_t* __restrict__ region) {
#pragma clang fp contract(off)
  float v[9];
  float d = INFINITY, x = px, y = py, z = pz;
  int fo = -1, ro = 255;
  if ((unsigned)f < (unsigned)nfaces && load_face(verts, nverts, faces, f, v)) {
    double qx, qy, qz;
    const double d2 = closest_on_face((double)px, (double)py, (double)pz, v, qx, qy, qz, ro);
    d = (float)sqrt(d2);
    x = (float)qx; y = (float)qy; z = (float)qz;
    fo = f;
  }
  dist[qi] = d;
  closest[3 * qi] = x; closest[3 * qi + 1] = y; closest[3 * qi + 2] = z;
  face[qi] = fo;
  region[qi] = (uint8_t)ro;
}

}  // namespace
