// The per-voxel and per-pixel rules of the TSDF volumes (include/spann3r_hip.h, "TSDF fusion", "TSDF ray-casting and frame-to-model
// tracking", "Brick TSDF volume"), stated once for the dense volume (csrc/fusion.hip, csrc/raycast.hip) and the brick volume
// (csrc/bricks.hip): the integrate rule of one voxel, the ray march of one pixel over a volume type that supplies the cell gather,
// the colour channel's rounding, and the host checks of the frame and view tables.  The kernels keep what is theirs: the mapping
// of a lane to its voxel or pixel, their loads and stores, their volume type.  Everything here is per translation unit (anonymous
// namespace).
#pragma once
#include "common.h"
#include <math.h>

// Every fp32 operation here is rounded on its own (no contraction into FMAs): this pragma is what the compiler honours under its
// default -ffp-contract=fast-honor-pragmas, and it holds from here to the end of the translation unit (the files that include this
// one set it for themselves too).  The files are built without fast-math, so each operation is one IEEE operation wherever it is
// inlined: a kernel of either volume computes the bits it computed when it carried its own copy of this text.
#pragma clang fp contract(off)

#define RC_TILE 16      // a ray-cast workgroup's pixel block; its four waves are the 8 x 8 quadrants

namespace {

__device__ __forceinline__ unsigned unorm8(float c) {      // sp3_pack_rgba8's channel: floor(c * 255 + 0.5), clamped; NaN gives 0
  const float s = floorf(c * 255.0f + 0.5f);
  return s >= 255.0f ? 255u : (s > 0.0f ? (unsigned)s : 0u);
}

// ------------------------------------------------------------------------------------------------ integration
// The voxel with its centre at (x, y, z) and the state (D, W, cr, cg, cb) walks the T frames in order.
template <bool RGB>
__device__ __forceinline__ void integrate_voxel(const sp3_tsdf_frame* __restrict__ frames, int T, float x, float y, float z, float trunc,
                                                float& D, float& W, float& cr, float& cg, float& cb) {
  for (int f = 0; f < T; ++f) {      // (f is wave-uniform: the descriptor fields arrive by scalar loads)
    const sp3_tsdf_frame& fr = frames[f];
    const float* m = fr.w2c;
    const float zc = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    if (!(zc > 0.f)) continue;
    const float xc = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    const float yc = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    const float u = fr.fu * xc / zc + fr.cu, w_ = fr.fv * yc / zc + fr.cv;
    const float fpx = floorf(u + 0.5f), fpy = floorf(w_ + 0.5f);
    if (!(fpx >= 0.f && fpx < (float)fr.w && fpy >= 0.f && fpy < (float)fr.h)) continue;      // (a NaN fails the test)
    const int64_t p = (int64_t)fpy * fr.row_stride + (int64_t)fpx;
    if (fr.valid != nullptr && fr.valid[p] == 0) continue;
    float d;
    if (fr.depth != nullptr) {
      d = fr.depth[p];
    } else {
      const float X = fr.pts[3 * p], Y = fr.pts[3 * p + 1], Z = fr.pts[3 * p + 2];
      d = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11];
    }
    if (!isfinite(d) || d <= 0.f) continue;
    const float s = d - zc;
    if (s < -trunc) continue;
    const float q = s / trunc;
    const float fv = q < 1.0f ? q : 1.0f;
    const float a = fr.pixel_weight != nullptr ? fr.pixel_weight[p] : 1.0f;
    if (!(a > 0.f) || !isfinite(a)) continue;
    const float Wn = W + a;
    D = (W * D + a * fv) / Wn;
    if (RGB) {
      const unsigned c = fr.rgba[p];
      const float r = (float)(c & 255u) / 255.0f, gch = (float)((c >> 8) & 255u) / 255.0f, b = (float)((c >> 16) & 255u) / 255.0f;
      cr = (W * cr + a * r) / Wn;
      cg = (W * cg + a * gch) / Wn;
      cb = (W * cb + a * b) / Wn;
    }
    W = Wn;
  }
}

// ------------------------------------------------------------------------------------------------ ray-casting
// the voxel-centre lattice and the march over it; bx, by, bz: its bricks (the brick volume's table; the dense volume ignores them)
struct RcVol {
  int nx, ny, nz, bx, by, bz;
  float ox, oy, oz, voxel, min_weight, step;
  int cap;
};

struct Ray {
  float ex, ey, ez, dx, dy, dz, lam0, lam1, dl;
};

// what a volume's load() says of a cell; ABSENT: invalid because the brick of corner 0 is absent (the brick volume only)
enum { CELL_INVALID = 0, CELL_VALID = 1, CELL_ABSENT = 2 };

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

// the y-then-z (or whichever two axes remain, in the header's order) lerp of four values indexed [first axis][second axis]
__device__ __forceinline__ float lerp2(float v00, float v10, float v01, float v11, float t1, float t2) {
  return lerp(lerp(v00, v10, t1), lerp(v01, v11, t1), t2);
}

__device__ __forceinline__ float trilinear(const float (&v)[8], float tx, float ty, float tz) {
  const float e00 = lerp(v[0], v[1], tx), e10 = lerp(v[2], v[3], tx), e01 = lerp(v[4], v[5], tx), e11 = lerp(v[6], v[7], tx);
  return lerp(lerp(e00, e10, ty), lerp(e01, e11, ty), tz);
}

// Pixel (px, py) of view vw (inside it) on volume `vol`.  Vol supplies
//   g: the lattice (an RcVol);
//   Cell: tx, ty, tz (the point's place in its cell) and v[8] (tsdf of corner code c = dx + 2 dy + 4 dz), plus what is its own;
//   load(px, py, pz, cell) -> CELL_*: the cell of a world point by the header's rule;
//   skip(ray, i, cell) -> after load said ABSENT at sample i, the sample index to go on from (all up to it are invalid);
//   corner(cell, e) -> the linear index of corner e of a valid cell, for the colour gather from rgb.
template <bool RGB, typename Vol>
__device__ __forceinline__ void raycast_pixel(const sp3_tsdf_view& vw, int px, int py, const Vol& vol, const float* __restrict__ rgb) {
  const RcVol& g = vol.g;
  const float* m = vw.c2w;
  const float xn = ((float)px - vw.cu) / vw.fu, yn = ((float)py - vw.cv) / vw.fv;
  Ray r;
  r.dx = (m[0] * xn + m[1] * yn) + m[2];
  r.dy = (m[4] * xn + m[5] * yn) + m[6];
  r.dz = (m[8] * xn + m[9] * yn) + m[10];
  r.ex = m[3];
  r.ey = m[7];
  r.ez = m[11];
  const float len = sqrtf((r.dx * r.dx + r.dy * r.dy) + r.dz * r.dz);
  r.dl = g.step / len;
  // the voxel-centre lattice's box by slabs
  float enter = -INFINITY, leave = INFINITY;
  bool alive = true;
  {
    const float d3[3] = {r.dx, r.dy, r.dz}, e3[3] = {r.ex, r.ey, r.ez}, o3[3] = {g.ox, g.oy, g.oz};
    const int n3[3] = {g.nx, g.ny, g.nz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float lo = o3[a], hi = o3[a] + (float)(n3[a] - 1) * g.voxel;
      if (d3[a] == 0.f) {
        alive = alive && lo <= e3[a] && e3[a] <= hi;
      } else {
        const float q1 = (lo - e3[a]) / d3[a], q2 = (hi - e3[a]) / d3[a];
        const float small = q2 < q1 ? q2 : q1, large = q2 < q1 ? q1 : q2;
        enter = small > enter ? small : enter;
        leave = large < leave ? large : leave;
      }
    }
  }
  r.lam0 = vw.near > enter ? vw.near : enter;
  r.lam1 = vw.far < leave ? vw.far : leave;
  alive = alive && r.lam0 <= r.lam1;      // (a NaN fails)
  bool hit = false, prev_valid = false;
  float f_prev = 0.f, lam_star = 0.f;
  typename Vol::Cell c;
  if (alive) {
    for (int i = 0; i < g.cap; ++i) {      // (the cap is a hard bound: no input makes a lane loop without end)
      const float lam = r.lam0 + (float)i * r.dl;
      if (!(lam <= r.lam1)) break;
      const int st = vol.load(r.ex + r.dx * lam, r.ey + r.dy * lam, r.ez + r.dz * lam, c);
      if (st != CELL_VALID) {
        prev_valid = false;
        if (st == CELL_ABSENT) i = vol.skip(r, i, c);
        continue;
      }
      const float f = trilinear(c.v, c.tx, c.ty, c.tz);
      if (prev_valid && f_prev >= 0.f && f < 0.f) {
        const float lam_prev = r.lam0 + (float)(i - 1) * r.dl;
        lam_star = lam_prev + r.dl * (f_prev / (f_prev - f));
        hit = true;
        break;
      }
      if (prev_valid && f_prev < 0.f && f >= 0.f) break;      // a back face
      f_prev = f;
      prev_valid = true;
    }
  }
  float vx = 0.f, vy = 0.f, vz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
  unsigned word = 0u;
  if (hit) {
    vx = r.ex + r.dx * lam_star;
    vy = r.ey + r.dy * lam_star;
    vz = r.ez + r.dz * lam_star;
    hit = vol.load(vx, vy, vz, c) == CELL_VALID;
    if (hit) {
      const float* v = c.v;
      // d/dx: the four x-edge differences, lerped along y then z; d/dy: the y-edge differences along x then z; d/dz: along x then y
      const float gx = lerp2(v[1] - v[0], v[3] - v[2], v[5] - v[4], v[7] - v[6], c.ty, c.tz);
      const float gy = lerp2(v[2] - v[0], v[3] - v[1], v[6] - v[4], v[7] - v[5], c.tx, c.tz);
      const float gz = lerp2(v[4] - v[0], v[5] - v[1], v[6] - v[2], v[7] - v[3], c.tx, c.ty);
      const float gl = sqrtf((gx * gx + gy * gy) + gz * gz);
      hit = gl > 0.f && isfinite(gl);
      if (hit) {
        nx = gx / gl;
        ny = gy / gl;
        nz = gz / gl;
        if (RGB) {
          word = 255u << 24;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            float col[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) col[e] = rgb[3 * vol.corner(c, e) + ch];
            word |= unorm8(trilinear(col, c.tx, c.ty, c.tz)) << (8 * ch);
          }
        }
      }
    }
  }
  if (!hit) {
    lam_star = 0.f;
    vx = vy = vz = nx = ny = nz = 0.f;
    word = 0u;
  }
  const int64_t p = (int64_t)py * vw.row_stride + px;
  vw.depth[p] = lam_star;
  if (vw.vertex != nullptr) {
    vw.vertex[3 * p] = vx;
    vw.vertex[3 * p + 1] = vy;
    vw.vertex[3 * p + 2] = vz;
  }
  if (vw.normal != nullptr) {
    vw.normal[3 * p] = nx;
    vw.normal[3 * p + 1] = ny;
    vw.normal[3 * p + 2] = nz;
  }
  if (vw.rgba != nullptr) vw.rgba[p] = word;
}

// ------------------------------------------------------------------------------------------------ host checks
// Each takes the entry point's name for its message and returns 1 with the error set, as SP3_CHECK does.

// the frame table of an integrate or mark call; with_rgb: every frame needs rgba.  -> max_pixels (nullable): the largest w * h
inline int check_frames(const char* what, const sp3_tsdf_frame* frames_host, int T, bool with_rgb, int64_t* max_pixels) {
  int64_t mp = 0;
  for (int f = 0; f < T; ++f) {
    const sp3_tsdf_frame& d = frames_host[f];
    SP3_CHECK((d.depth != nullptr) != (d.pts != nullptr), "%s: frame %d: give depth or pts, exactly one", what, f);
    SP3_CHECK(d.w >= 1 && d.h >= 1 && d.w <= (1 << 24) && d.h <= (1 << 24) && d.row_stride >= d.w && (int64_t)d.h * d.row_stride < 0x7fffffffLL,
              "%s: frame %d: bad geometry: %d x %d, row stride %lld", what, f, d.w, d.h, (long long)d.row_stride);
    SP3_CHECK(!with_rgb || d.rgba != nullptr, "%s: frame %d has no rgba but the volume has colours", what, f);
    for (int e = 0; e < 12; ++e) SP3_CHECK(isfinite(d.w2c[e]), "%s: frame %d: world-to-camera matrix is not finite", what, f);
    SP3_CHECK(isfinite(d.fu) && isfinite(d.fv) && isfinite(d.cu) && isfinite(d.cv), "%s: frame %d: intrinsics are not finite", what, f);
    const int64_t px = (int64_t)d.w * d.h;
    mp = px > mp ? px : mp;
  }
  if (max_pixels != nullptr) *max_pixels = mp;
  return 0;
}

// the march of a ray-cast call over g's lattice (dims and voxel set): min_weight and step, and the sample cap they give, into g
inline int check_march(const char* what, float min_weight, float step, RcVol& g) {
  SP3_CHECK(min_weight > 0.f, "%s: min_weight %g must be > 0", what, (double)min_weight);
  SP3_CHECK(isfinite(step) && step > 0.f, "%s: step %g must be finite and > 0", what, (double)step);
  const double capd = ceil(2.0 * ((double)g.nx + g.ny + g.nz) * (double)g.voxel / (double)step);
  SP3_CHECK(capd <= (double)(1 << 24), "%s: step %g is too small for a volume of %d x %d x %d voxels of %g: over 2^24 samples per ray", what,
            (double)step, g.nx, g.ny, g.nz, (double)g.voxel);
  g.min_weight = min_weight;
  g.step = step;
  g.cap = (int)capd;
  return 0;
}

// the view table of a ray-cast call (T >= 1); has_rgb: the volume has colours.  -> the largest width and height
inline int check_views(const char* what, const sp3_tsdf_view* views_host, const sp3_tsdf_view* views_dev, int T, bool has_rgb, int& wmax,
                       int& hmax) {
  SP3_CHECK(views_host != nullptr && views_dev != nullptr, "%s: null views", what);
  wmax = hmax = 0;
  for (int f = 0; f < T; ++f) {
    const sp3_tsdf_view& d = views_host[f];
    SP3_CHECK(d.depth != nullptr, "%s: view %d: null depth", what, f);
    SP3_CHECK(d.w >= 1 && d.h >= 1 && d.w <= (1 << 24) && d.h <= (1 << 24) && d.row_stride >= d.w && (int64_t)d.h * d.row_stride < 0x7fffffffLL,
              "%s: view %d: bad geometry: %d x %d, row stride %lld", what, f, d.w, d.h, (long long)d.row_stride);
    SP3_CHECK(d.rgba == nullptr || has_rgb, "%s: view %d asks for rgba but the volume has no colours", what, f);
    for (int e = 0; e < 12; ++e) SP3_CHECK(isfinite(d.c2w[e]), "%s: view %d: camera-to-world matrix is not finite", what, f);
    SP3_CHECK(isfinite(d.fu) && isfinite(d.fv) && isfinite(d.cu) && isfinite(d.cv) && d.fu != 0.f && d.fv != 0.f,
              "%s: view %d: intrinsics must be finite, fu and fv not 0", what, f);
    SP3_CHECK(d.near >= 0.f && d.near <= d.far, "%s: view %d: near %g, far %g: 0 <= near <= far", what, f, (double)d.near, (double)d.far);
    wmax = d.w > wmax ? d.w : wmax;
    hmax = d.h > hmax ? d.h : hmax;
  }
  return 0;
}

// the launch grid of a ray-cast call: RC_TILE x RC_TILE pixel blocks of the largest view, one layer per view
inline int view_grid(const char* what, int wmax, int hmax, int T, dim3& grid) {
  grid = dim3((unsigned)((wmax + RC_TILE - 1) / RC_TILE), (unsigned)((hmax + RC_TILE - 1) / RC_TILE), (unsigned)T);
  SP3_CHECK(grid.y <= 65535u, "%s: a view of %d rows: the height must stay below 2^20", what, hmax);
  return 0;
}

}  // namespace
