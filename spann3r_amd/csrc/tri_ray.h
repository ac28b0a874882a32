// The rule of one (ray, face) pair of "Mesh rays" (include/spann3r_hip.h), per translation unit: Woop, Benthin and Wald's watertight
// test in fp64, what a ray reports of its winning face, the clip of a ray against an axis-aligned box and the ray of a camera pixel.
// csrc/mesh_ray.hip (the grid and the brute-force kernels) and csrc/mesh_bvh.hip (the tree) evaluate faces with these very
// functions, so a face gives the same bits whichever structure reaches it.  Every fp64 operation is rounded on its own (the
// block-scope pragma in each body), whatever the including file sets.
#pragma once
#include "tri.h"

namespace {

enum { CULL_NONE = 0, CULL_BACK = 1, CULL_FRONT = 2 };

__device__ __forceinline__ float pick(float a, float b, float c, int k) { return k == 0 ? a : (k == 1 ? b : c); }
__device__ __forceinline__ double pick(double a, double b, double c, int k) { return k == 0 ? a : (k == 1 ? b : c); }

// the ray in the form the test wants it: the permuted origin and the shear (header, rule 3)
struct Ray {
  double okx, oky, okz, Sx, Sy, Sz;
  int kx, ky, kz;
  bool ok;      // finite and d != 0
};

__device__ __forceinline__ Ray make_ray(float ox, float oy, float oz, float dx, float dy, float dz) {
#pragma clang fp contract(off)
  Ray r;
  const double o0 = (double)ox, o1 = (double)oy, o2 = (double)oz, d0 = (double)dx, d1 = (double)dy, d2 = (double)dz;
  r.ok = is_finite(fabs(o0)) && is_finite(fabs(o1)) && is_finite(fabs(o2)) && is_finite(fabs(d0)) && is_finite(fabs(d1)) && is_finite(fabs(d2)) &&
         !(d0 == 0.0 && d1 == 0.0 && d2 == 0.0);
  const double a0 = fabs(d0), a1 = fabs(d1), a2 = fabs(d2);
  int kz = 0;
  if (a1 > a0) kz = 1;
  if (a2 > fmax(a0, a1)) kz = 2;
  int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
  const double dkz = pick(d0, d1, d2, kz);
  if (dkz < 0.0) { const int s = kx; kx = ky; ky = s; }
  r.kx = kx; r.ky = ky; r.kz = kz;
  r.okx = pick(o0, o1, o2, kx); r.oky = pick(o0, o1, o2, ky); r.okz = pick(o0, o1, o2, kz);
  r.Sx = pick(d0, d1, d2, kx) / dkz;
  r.Sy = pick(d0, d1, d2, ky) / dkz;
  r.Sz = 1.0 / dkz;
  return r;
}

struct Hit { double U, V, W, det, t; };

// rule 3 for the face whose nine coordinates are at v; true for a hit inside [t_min, t_max] that the culling keeps
__device__ __forceinline__ bool intersect(const Ray& r, const float* v, double t_min, double t_max, int cull, Hit& h) {
#pragma clang fp contract(off)
  double X[3], Y[3], Z[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float a = v[3 * i], b = v[3 * i + 1], c = v[3 * i + 2];
    const double px = (double)pick(a, b, c, r.kx) - r.okx, py = (double)pick(a, b, c, r.ky) - r.oky, pz = (double)pick(a, b, c, r.kz) - r.okz;
    X[i] = px - r.Sx * pz;
    Y[i] = py - r.Sy * pz;
    Z[i] = r.Sz * pz;
  }
  h.U = X[2] * Y[1] - Y[2] * X[1];
  h.V = X[0] * Y[2] - Y[0] * X[2];
  h.W = X[1] * Y[0] - Y[1] * X[0];
  if ((h.U < 0.0 || h.V < 0.0 || h.W < 0.0) && (h.U > 0.0 || h.V > 0.0 || h.W > 0.0)) return false;
  h.det = (h.U + h.V) + h.W;
  if (h.det == 0.0) return false;
  if ((cull == CULL_BACK && h.det < 0.0) || (cull == CULL_FRONT && h.det > 0.0)) return false;
  const double T = (h.U * Z[0] + h.V * Z[1]) + h.W * Z[2];
  double t = T / h.det;
  if (t == 0.0) t = 0.0;      // -0 -> +0
  h.t = t;
  return t_min <= t && t <= t_max;      // (false for a NaN)
}

// what a ray reports of its winning face f (NO_FACE, -1 or anything that is no hit: the outputs of a miss)
struct Result { float t, bary[3], point[3]; int face; int side; };

__device__ __forceinline__ Result result_of(const float* __restrict__ verts, int nverts, const int* __restrict__ faces, int nfaces, const Ray& r,
                                            float ox, float oy, float oz, float dx, float dy, float dz, double t_min, double t_max, int cull, int f) {
#pragma clang fp contract(off)
  Result o;
  o.t = INFINITY; o.face = -1; o.side = 255;
  o.bary[0] = o.bary[1] = o.bary[2] = 0.f;
  o.point[0] = ox; o.point[1] = oy; o.point[2] = oz;
  float v[9];
  Hit h;
  if (r.ok && (unsigned)f < (unsigned)nfaces && load_face(verts, nverts, faces, f, v) && intersect(r, v, t_min, t_max, cull, h)) {
    o.t = (float)h.t;
    o.face = f;
    o.side = h.det > 0.0 ? 0 : 1;
    o.bary[0] = (float)(h.U / h.det); o.bary[1] = (float)(h.V / h.det); o.bary[2] = (float)(h.W / h.det);
    const double mx = h.t * (double)dx, my = h.t * (double)dy, mz = h.t * (double)dz;
    o.point[0] = (float)((double)ox + mx); o.point[1] = (float)((double)oy + my); o.point[2] = (float)((double)oz + mz);
  }
  return o;
}

struct RayOut { float* t; int* face; float* bary; float* point; uint8_t* side; };

__device__ __forceinline__ void store(const RayOut& out, int64_t i, const Result& o) {
  out.t[i] = o.t;
  out.face[i] = o.face;
  out.side[i] = (uint8_t)o.side;
#pragma unroll
  for (int k = 0; k < 3; ++k) { out.bary[3 * i + k] = o.bary[k]; out.point[3 * i + k] = o.point[k]; }
}

// The slab test of the ray (o, d) against the box [lo, hi]: cuts [t0, t1] to the part of the ray inside it; a zero component is a
// test of the origin, not a division.  False when the ray misses the box or nothing of [t0, t1] is left.
__device__ __forceinline__ bool clip_box(const double (&o)[3], const double (&d)[3], const double (&lo)[3], const double (&hi)[3], double& t0,
                                         double& t1) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (d[k] == 0.0) {
      if (!(o[k] >= lo[k] && o[k] <= hi[k])) return false;
    } else {
      const double a = (lo[k] - o[k]) / d[k], b = (hi[k] - o[k]) / d[k];
      t0 = fmax(t0, fmin(a, b));
      t1 = fmin(t1, fmax(a, b));
    }
  }
  return t0 <= t1;
}

// the ray of pixel (px, py) of a camera of sp3_mesh_ray_views (header: the pixel rule): its origin and its fp32 direction
__device__ __forceinline__ void pixel_ray(const sp3_mesh_ray_view& vw, int px, int py, float pixel_offset, float (&oo)[3], float (&dd)[3]) {
#pragma clang fp contract(off)
  const double x = (((double)px + (double)pixel_offset) - (double)vw.cu) / (double)vw.fu;
  const double y = (((double)py + (double)pixel_offset) - (double)vw.cv) / (double)vw.fv;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double a = (double)vw.c2w[4 * i] * x, b = (double)vw.c2w[4 * i + 1] * y;
    dd[i] = (float)((a + b) + (double)vw.c2w[4 * i + 2]);
  }
  oo[0] = vw.c2w[3]; oo[1] = vw.c2w[7]; oo[2] = vw.c2w[11];
}

// what pixel (px, py) of a view keeps of its ray's result: depth 0 for a miss
__device__ __forceinline__ void store_pixel(const sp3_mesh_ray_view& vw, int px, int py, const Result& o) {
  const int64_t p = (int64_t)py * vw.row_stride + px;
  vw.depth[p] = o.face >= 0 ? o.t : 0.f;
  if (vw.face != nullptr) vw.face[p] = o.face;
  if (vw.bary != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; ++k) vw.bary[3 * p + k] = o.bary[k];
  }
}

}  // namespace
