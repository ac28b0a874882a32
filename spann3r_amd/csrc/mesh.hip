// Pointmap meshes (app.py:68-105 pts3d_to_trimesh, :38-47 cat_meshes, :132-167 of reconstruct; spann3r_amd/mesh.py and vis.py drive these):
// the face list of t pointmaps with invalid faces removed in order, the compaction of the vertices a mesh or a cloud keeps, and a
// triangle rasteriser into the 64-bit key buffer of csrc/render.hip.
//
// Both compactions are an order-preserving exclusive scan in plain multi-launch form: one count per 256-element tile, one
// single-workgroup scan of the counts, one scatter.  No workgroup waits on another; the launch boundaries are the only hand-offs.
//
// Every fp32 operation of the projection, the depth interpolation and the vertex transform is rounded on its own (no contraction
// into FMAs): the file-level pragma below is what the compiler honours under its default -ffp-contract=fast-honor-pragmas.
#include "common.h"
#include "scan.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + MB - 1) / MB); }
inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

// the validity rule shared by the face build and the point-cloud compaction
__device__ __forceinline__ bool pixel_ok(const uint8_t* __restrict__ valid, const float* __restrict__ conf, float conf_thresh,
                                         const float* __restrict__ pts, int64_t p) {
  if (valid != nullptr && valid[p] == 0) return false;
  if (conf != nullptr) {
    const float c = conf[p];
    if (!((c - 1.0f) / c > conf_thresh)) return false;          // the reference's mask (app.py:147-148); a NaN confidence is invalid
  }
  if (pts != nullptr && !(isfinite(pts[3 * p]) && isfinite(pts[3 * p + 1]) && isfinite(pts[3 * p + 2]))) return false;
  return true;
}

__global__ __launch_bounds__(MB) void k_mesh_mask(const uint8_t* __restrict__ valid, const float* __restrict__ conf, float conf_thresh,
                                                  const float* __restrict__ pts, int64_t n, uint8_t* __restrict__ mask) {
  const int64_t p = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (p < n) mask[p] = pixel_ok(valid, conf, conf_thresh, pts, p) ? 1 : 0;
}

// One candidate face: segment = (frame, block), block = 4 (both windings) or 2 (forward) per frame; tile = 256 cells of it.
struct FaceGeom {
  int h, w, cells, tps, nblk;      // tps: tiles per segment; nblk: blocks per frame
};
struct Cand {
  bool ok;
  int a, b, c, colour;
};
__device__ __forceinline__ Cand candidate(const uint8_t* __restrict__ mask, const FaceGeom g) {
  Cand r;
  r.ok = false;
  r.a = r.b = r.c = r.colour = 0;
  const int seg = blockIdx.x / g.tps, tile = blockIdx.x % g.tps;
  const int cell = tile * MB + threadIdx.x;
  if (cell >= g.cells) return r;
  const int f = seg / g.nblk, blk = seg % g.nblk;
  const int tri = g.nblk == 4 ? blk >> 1 : blk, rev = g.nblk == 4 ? blk & 1 : 0;
  const int y = cell / (g.w - 1), x = cell % (g.w - 1);
  const int tl = (f * g.h + y) * g.w + x, tr = tl + 1, bl = tl + g.w, br = bl + 1;
  if (tri == 0) {
    r.ok = mask[tl] && mask[tr] && mask[bl];
    r.a = rev ? bl : tl;
    r.b = tr;
    r.c = rev ? tl : bl;
    r.colour = tl;
  } else {
    r.ok = mask[tr] && mask[bl] && mask[br];
    r.a = rev ? br : tr;
    r.b = bl;
    r.c = rev ? tr : br;
    r.colour = br;
  }
  return r;
}

__global__ __launch_bounds__(MB) void k_mesh_face_count(const uint8_t* __restrict__ mask, FaceGeom g, int* __restrict__ counts) {
  const Cand c = candidate(mask, g);
  int total;
  block_rank(c.ok, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(MB) void k_mesh_face_scatter(const uint8_t* __restrict__ mask, FaceGeom g, const int* __restrict__ offsets,
                                                          int* __restrict__ faces, int* __restrict__ colour_px) {
  const Cand c = candidate(mask, g);
  int total;
  const int rank = block_rank(c.ok, total);
  if (!c.ok) return;
  const int64_t dst = (int64_t)offsets[blockIdx.x] + rank;
  faces[3 * dst] = c.a;
  faces[3 * dst + 1] = c.b;
  faces[3 * dst + 2] = c.c;
  colour_px[dst] = c.colour;
}

// ------------------------------------------------------------------------------------------------ vertex compaction
__global__ __launch_bounds__(MB) void k_mesh_flag_init(const uint8_t* __restrict__ valid, const float* __restrict__ conf, float conf_thresh,
                                                       const float* __restrict__ pts, int64_t n, int cloud, int* __restrict__ remap) {
  const int64_t p = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (p < n) remap[p] = cloud && pixel_ok(valid, conf, conf_thresh, pts, p) ? 1 : 0;
}

__global__ __launch_bounds__(MB) void k_mesh_flag_faces(const int* __restrict__ faces, int64_t elems, int64_t n, int* __restrict__ remap) {
  const int64_t e = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (e >= elems) return;
  const int v = faces[e];
  if (v >= 0 && v < n) remap[v] = 1;      // (every writer stores the same value)
}

__global__ __launch_bounds__(MB) void k_mesh_flag_count(const int* __restrict__ remap, int64_t n, int* __restrict__ counts) {
  const int64_t p = (int64_t)blockIdx.x * MB + threadIdx.x;
  int total;
  block_rank(p < n && remap[p] != 0, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

struct Xform {
  float m[12];      // the first three rows of the row-major 4x4
  float scale;
};

// kept vertex p -> row offsets[tile] + rank: position, colour; remap[p] = that row (-1: dropped); per-tile min / max of the written
// positions to part[tile][6] (+inf / -inf for a tile that keeps nothing)
__global__ __launch_bounds__(MB) void k_mesh_vertex_scatter(const float* __restrict__ pts, const unsigned* __restrict__ rgba, int64_t n,
                                                            const int* __restrict__ offsets, Xform xf, int* __restrict__ remap,
                                                            float* __restrict__ out_pos, unsigned* __restrict__ out_rgba,
                                                            float* __restrict__ part) {
  __shared__ float red[MB / SP3_WAVE][6];
  const int64_t p = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool keep = p < n && remap[p] != 0;
  int total;
  const int rank = block_rank(keep, total);
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (keep) {
    const int64_t dst = (int64_t)offsets[blockIdx.x] + rank;
    const float x = pts[3 * p] * xf.scale, y = pts[3 * p + 1] * xf.scale, z = pts[3 * p + 2] * xf.scale;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float o = ((xf.m[4 * r] * x + xf.m[4 * r + 1] * y) + xf.m[4 * r + 2] * z) + xf.m[4 * r + 3];
      out_pos[3 * dst + r] = o;
      lo[r] = hi[r] = o;
    }
    if (out_rgba != nullptr) out_rgba[dst] = rgba[p];
    remap[p] = (int)dst;
  } else if (p < n) {
    remap[p] = -1;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[r] = fminf(lo[r], __shfl_xor(lo[r], o));
      hi[r] = fmaxf(hi[r], __shfl_xor(hi[r], o));
    }
  }
  const int lane = threadIdx.x & (SP3_WAVE - 1), wave = threadIdx.x / SP3_WAVE;
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      red[wave][r] = lo[r];
      red[wave][3 + r] = hi[r];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = red[0][threadIdx.x];
    for (int wv = 1; wv < MB / SP3_WAVE; ++wv) v = threadIdx.x < 3 ? fminf(v, red[wv][threadIdx.x]) : fmaxf(v, red[wv][threadIdx.x]);
    part[(int64_t)blockIdx.x * 6 + threadIdx.x] = v;
  }
}

// minmax[c] over the nb tile records; one workgroup
__global__ __launch_bounds__(MB) void k_mesh_minmax(const float* __restrict__ part, int nb, float* __restrict__ minmax) {
  __shared__ float red[MB][6];
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int b = threadIdx.x; b < nb; b += MB) {
#pragma unroll
    for (int c = 0; c < 6; ++c) v[c] = c < 3 ? fminf(v[c], part[(int64_t)b * 6 + c]) : fmaxf(v[c], part[(int64_t)b * 6 + c]);
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) red[threadIdx.x][c] = v[c];
  __syncthreads();
  if (threadIdx.x < 6) {
    const int c = threadIdx.x;
    float r = red[0][c];
    for (int i = 1; i < MB; ++i) r = c < 3 ? fminf(r, red[i][c]) : fmaxf(r, red[i][c]);
    minmax[c] = r;
  }
}

__global__ __launch_bounds__(MB) void k_mesh_remap_faces(int* __restrict__ faces, int64_t elems, int64_t n, const int* __restrict__ remap) {
  const int64_t e = (int64_t)blockIdx.x * MB + threadIdx.x;
  if (e >= elems) return;
  const int v = faces[e];
  faces[e] = v >= 0 && v < n ? remap[v] : -1;
}

// ------------------------------------------------------------------------------------------------ triangle rasteriser
struct Snap {
  bool ok;
  int x, y;      // 1/16 pixel
  float z;
};
__device__ __forceinline__ Snap project_snap(const float* __restrict__ pts, int v, const sp3_render_cam& cam) {
  Snap s;
  s.ok = false;
  s.x = s.y = 0;
  s.z = 0.f;
  const float x = pts[3 * (int64_t)v], y = pts[3 * (int64_t)v + 1], z = pts[3 * (int64_t)v + 2];
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return s;
  const float xc = ((cam.R[0] * x + cam.R[1] * y) + cam.R[2] * z) + cam.t[0];      // (sp3_render_splat's projection, same order)
  const float yc = ((cam.R[3] * x + cam.R[4] * y) + cam.R[5] * z) + cam.t[1];
  const float zc = ((cam.R[6] * x + cam.R[7] * y) + cam.R[8] * z) + cam.t[2];
  if (!(isfinite(xc) && isfinite(yc) && isfinite(zc)) || zc <= cam.z_near) return s;
  const float u = cam.fx * xc / zc + cam.cx, v_ = cam.fy * yc / zc + cam.cy;
  const float sx = floorf(16.0f * u + 0.5f), sy = floorf(16.0f * v_ + 0.5f);
  const float lim = 1048576.0f;      // 2^20 (a NaN or infinite coordinate fails the test too)
  if (!(sx >= -lim && sx <= lim && sy >= -lim && sy <= lim)) return s;
  s.ok = true;
  s.x = (int)sx;
  s.y = (int)sy;
  s.z = zc;
  return s;
}

__device__ __forceinline__ bool top_left(int64_t dx, int64_t dy) { return dy < 0 || (dy == 0 && dx > 0); }

__global__ __launch_bounds__(MB) void k_render_tris(const float* __restrict__ pts, int64_t nverts, const int* __restrict__ faces,
                                                    const int* __restrict__ colour_px, int64_t nfaces, const int* __restrict__ nfaces_dev,
                                                    unsigned index_base, sp3_render_cam cam, int max_bbox_px,
                                                    unsigned long long* __restrict__ keys, unsigned long long* __restrict__ culled_big) {
  const int64_t i = (int64_t)blockIdx.x * MB + threadIdx.x;
  int64_t count = nfaces;
  if (nfaces_dev != nullptr) count = min(count, (int64_t)max(*nfaces_dev, 0));
  bool big = false;
  do {      // (one pass; `break` = this lane draws nothing)
    if (i >= count) break;
    const int ia = faces[3 * i], ib = faces[3 * i + 1], ic = faces[3 * i + 2];
    const int col = colour_px != nullptr ? colour_px[i] : ia;
    if (ia < 0 || ia >= nverts || ib < 0 || ib >= nverts || ic < 0 || ic >= nverts || col < 0 || col >= nverts) break;
    const Snap a = project_snap(pts, ia, cam);
    Snap b = project_snap(pts, ib, cam), c = project_snap(pts, ic, cam);
    if (!(a.ok && b.ok && c.ok)) break;
    int64_t area = (int64_t)(b.x - a.x) * (c.y - a.y) - (int64_t)(c.x - a.x) * (b.y - a.y);
    if (area == 0) break;
    if (area < 0) {      // both orientations are drawn: the second and third vertex swap
      const Snap t = b;
      b = c;
      c = t;
      area = -area;
    }
    // pixels whose centre (16 px, 16 py) lies inside the box of the snapped vertices, clipped to the image
    const int xmin = min(a.x, min(b.x, c.x)), xmax = max(a.x, max(b.x, c.x));
    const int ymin = min(a.y, min(b.y, c.y)), ymax = max(a.y, max(b.y, c.y));
    const int px0 = max((xmin + 15) >> 4, 0), px1 = min(xmax >> 4, cam.width - 1);
    const int py0 = max((ymin + 15) >> 4, 0), py1 = min(ymax >> 4, cam.height - 1);
    if (px0 > px1 || py0 > py1) break;
    if ((int64_t)(px1 - px0 + 1) * (py1 - py0 + 1) > max_bbox_px) {
      big = true;
      break;
    }
    // edge functions E(p) = dx (py - ya) - dy (px - xa): e0 of b->c (weight of a), e1 of c->a (of b), e2 of a->b (of c)
    const int64_t dx0 = c.x - b.x, dy0 = c.y - b.y, dx1 = a.x - c.x, dy1 = a.y - c.y, dx2 = b.x - a.x, dy2 = b.y - a.y;
    const bool tl0 = top_left(dx0, dy0), tl1 = top_left(dx1, dy1), tl2 = top_left(dx2, dy2);
    const float iza = 1.0f / a.z, izb = 1.0f / b.z, izc = 1.0f / c.z, farea = (float)area;
    const unsigned long long low = (unsigned long long)(index_base + (unsigned)col);
    for (int py = py0; py <= py1; ++py) {      // at most max_bbox_px pixels in all
      const int64_t cy = 16 * (int64_t)py, cx = 16 * (int64_t)px0;
      int64_t e0 = dx0 * (cy - b.y) - dy0 * (cx - b.x);
      int64_t e1 = dx1 * (cy - c.y) - dy1 * (cx - c.x);
      int64_t e2 = dx2 * (cy - a.y) - dy2 * (cx - a.x);
      for (int px = px0; px <= px1; ++px, e0 -= 16 * dy0, e1 -= 16 * dy1, e2 -= 16 * dy2) {
        if (!((e0 > 0 || (e0 == 0 && tl0)) && (e1 > 0 || (e1 == 0 && tl1)) && (e2 > 0 || (e2 == 0 && tl2)))) continue;
        const float s = ((float)e0 * iza + (float)e1 * izb) + (float)e2 * izc;
        const float depth = farea / s;
        if (!isfinite(depth)) continue;
        const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | low;
        unsigned long long* k = keys + (int64_t)py * cam.width + px;
        if (*k <= key) continue;      // (a stale cached value is an older, larger key: the atomic then decides)
        __hip_atomic_fetch_min(k, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  } while (false);
  if (culled_big != nullptr) {      // one add per wave that culled any
    const unsigned long long m = __ballot(big);
    if (m != 0 && (threadIdx.x & (SP3_WAVE - 1)) == 0)
      __hip_atomic_fetch_add(culled_big, (unsigned long long)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// tiles of the face build: per (frame, block) segment, ceil(cells / 256)
inline int64_t face_tiles(int t, int h, int w) { return (int64_t)t * 4 * (((int64_t)(h - 1) * (w - 1) + MB - 1) / MB); }

int check_grid(const char* what, int t, int h, int w) {
  SP3_CHECK(t >= 0 && h >= 1 && w >= 1, "%s: t %d, h %d, w %d: t >= 0 and h, w >= 1 wanted", what, t, h, w);
  SP3_CHECK((int64_t)t * h * w * 4 < 0x7fffffffLL, "%s: t h w = %lld: 4 t h w must stay below 2^31 (int32 face and vertex indices)", what,
            (long long)t * h * w);
  return 0;
}

}  // namespace

extern "C" int64_t sp3_mesh_faces_ws_bytes(int t, int h, int w) {
  if (t <= 0 || h < 1 || w < 1 || (int64_t)t * h * w * 4 >= 0x7fffffffLL) return 0;
  return align16((int64_t)t * h * w) + align16((face_tiles(t, h, w) + 1) * 4);
}

extern "C" int sp3_mesh_faces(const uint8_t* valid, const float* conf, float conf_thresh, const float* pts, int t, int h, int w,
                              int both_windings, void* ws, int32_t* faces, int32_t* colour_px, int32_t* counts, void* stream) {
  if (check_grid("sp3_mesh_faces", t, h, w)) return 1;
  SP3_CHECK(valid == nullptr || conf == nullptr, "sp3_mesh_faces: give valid or conf, not both");
  SP3_CHECK(both_windings == 0 || both_windings == 1, "sp3_mesh_faces: both_windings %d must be 0 or 1", both_windings);
  if (t == 0) return 0;
  SP3_CHECK(counts != nullptr && ws != nullptr, "sp3_mesh_faces: null counts/ws");
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "sp3_mesh_faces: ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  FaceGeom g;
  g.h = h;
  g.w = w;
  g.cells = (h - 1) * (w - 1);
  g.tps = (g.cells + MB - 1) / MB;
  g.nblk = both_windings ? 4 : 2;
  const int nseg = t * g.nblk, nb = nseg * g.tps;
  const int64_t n = (int64_t)t * h * w;
  uint8_t* mask = (uint8_t*)ws;
  int* offsets = (int*)((char*)ws + align16(n));
  SP3_CHECK(g.cells == 0 || (faces != nullptr && colour_px != nullptr), "sp3_mesh_faces: null faces/colour_px");
  hipLaunchKernelGGL(k_mesh_mask, dim3(blocks_for(n)), dim3(MB), 0, st, valid, conf, conf_thresh, pts, n, mask);
  if (nb > 0) hipLaunchKernelGGL(k_mesh_face_count, dim3(nb), dim3(MB), 0, st, (const uint8_t*)mask, g, offsets);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, offsets, nb, (nb + SCAN_T - 1) / SCAN_T, (int*)counts, nseg, g.tps);
  if (nb > 0) hipLaunchKernelGGL(k_mesh_face_scatter, dim3(nb), dim3(MB), 0, st, (const uint8_t*)mask, g, (const int*)offsets, (int*)faces, (int*)colour_px);
  SP3_LAUNCH_CHECK("sp3_mesh_faces");
  return 0;
}

extern "C" int64_t sp3_mesh_vertices_ws_bytes(int64_t n) {
  if (n <= 0 || n >= 0x7fffffffLL) return 0;
  const int64_t nb = (n + MB - 1) / MB;
  return align16(n * 4) + align16((nb + 1) * 4) + align16(nb * 6 * 4);
}

extern "C" int sp3_mesh_compact_vertices(const float* pts, const uint32_t* rgba, int64_t n, int32_t* faces, int64_t nfaces,
                                         const uint8_t* valid, const float* conf, float conf_thresh, float scale, const float* transform16,
                                         void* ws, float* out_pos, uint32_t* out_rgba, int32_t* count, float* minmax, void* stream) {
  SP3_CHECK(n >= 0 && n < 0x7fffffffLL && nfaces >= 0 && nfaces <= 0x7fffffffLL,
            "sp3_mesh_compact_vertices: n %lld or nfaces %lld out of range", (long long)n, (long long)nfaces);
  SP3_CHECK(valid == nullptr || conf == nullptr, "sp3_mesh_compact_vertices: give valid or conf, not both");
  SP3_CHECK(faces == nullptr || (valid == nullptr && conf == nullptr),
            "sp3_mesh_compact_vertices: valid / conf select the points of a cloud; with faces the kept set is what the faces reference");
  if (n == 0) return 0;
  SP3_CHECK(pts != nullptr && ws != nullptr && out_pos != nullptr && count != nullptr && minmax != nullptr,
            "sp3_mesh_compact_vertices: null pts/ws/out_pos/count/minmax");
  SP3_CHECK((rgba == nullptr) == (out_rgba == nullptr), "sp3_mesh_compact_vertices: rgba and out_rgba go together");
  SP3_CHECK(((uintptr_t)ws & 15) == 0, "sp3_mesh_compact_vertices: ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)((n + MB - 1) / MB);
  int* remap = (int*)ws;
  int* offsets = (int*)((char*)ws + align16(n * 4));
  float* part = (float*)((char*)offsets + align16(((int64_t)nb + 1) * 4));
  Xform xf;
  for (int i = 0; i < 12; ++i) xf.m[i] = transform16 != nullptr ? transform16[i] : (i % 5 == 0 ? 1.0f : 0.0f);
  xf.scale = scale;
  const int cloud = faces == nullptr;
  const int64_t elems = nfaces * 3;
  hipLaunchKernelGGL(k_mesh_flag_init, dim3(nb), dim3(MB), 0, st, valid, conf, conf_thresh, pts, n, cloud, remap);
  if (!cloud && elems > 0) hipLaunchKernelGGL(k_mesh_flag_faces, dim3(blocks_for(elems)), dim3(MB), 0, st, (const int*)faces, elems, n, remap);
  hipLaunchKernelGGL(k_mesh_flag_count, dim3(nb), dim3(MB), 0, st, (const int*)remap, n, offsets);
  hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, offsets, nb, (nb + SCAN_T - 1) / SCAN_T, (int*)count, 0, 0);
  hipLaunchKernelGGL(k_mesh_vertex_scatter, dim3(nb), dim3(MB), 0, st, pts, (const unsigned*)rgba, n, (const int*)offsets, xf, remap, out_pos,
                     (unsigned*)out_rgba, part);
  hipLaunchKernelGGL(k_mesh_minmax, dim3(1), dim3(MB), 0, st, (const float*)part, nb, minmax);
  if (!cloud && elems > 0) hipLaunchKernelGGL(k_mesh_remap_faces, dim3(blocks_for(elems)), dim3(MB), 0, st, (int*)faces, elems, n, (const int*)remap);
  SP3_LAUNCH_CHECK("sp3_mesh_compact_vertices");
  return 0;
}

extern "C" int sp3_render_tris(const float* pts, int64_t nverts, const int32_t* faces, const int32_t* colour_px, int64_t nfaces,
                               const int32_t* nfaces_dev, int64_t index_base, const sp3_render_cam* cam, int max_bbox_px, uint64_t* keys,
                               uint64_t* culled_big, void* stream) {
  SP3_CHECK(cam != nullptr, "sp3_render_tris: null camera");
  SP3_CHECK(cam->width > 0 && cam->height > 0 && (int64_t)cam->width * cam->height <= 0x7fffffff && cam->width <= (1 << 24) &&
                cam->height <= (1 << 24),
            "sp3_render_tris: image %d x %d outside 1..2^24 per side, 2^31-1 pixels", cam->width, cam->height);
  SP3_CHECK(cam->z_near >= 0.f, "sp3_render_tris: z_near %g must be >= 0 (depth keys are positive fp32 bit patterns)", (double)cam->z_near);
  SP3_CHECK(max_bbox_px > 0, "sp3_render_tris: max_bbox_px %d must be > 0 (it bounds every lane's pixel loop)", max_bbox_px);
  SP3_CHECK(nverts >= 0 && nverts < 0x7fffffffLL && nfaces >= 0 && nfaces <= 0x7fffffffLL && index_base >= 0,
            "sp3_render_tris: nverts %lld, nfaces %lld or index_base %lld out of range", (long long)nverts, (long long)nfaces, (long long)index_base);
  SP3_CHECK(index_base + nverts < 0xffffffffLL,
            "sp3_render_tris: index overflow: index_base %lld + nverts %lld reaches 2^32-1 (colour indices are the low 32 bits of a key, all-ones is empty)",
            (long long)index_base, (long long)nverts);
  if (nfaces == 0) return 0;
  SP3_CHECK(pts != nullptr && faces != nullptr && keys != nullptr, "sp3_render_tris: null pts/faces/keys");
  hipLaunchKernelGGL(k_render_tris, dim3(blocks_for(nfaces)), dim3(MB), 0, (hipStream_t)stream, pts, nverts, (const int*)faces, (const int*)colour_px,
                     nfaces, (const int*)nfaces_dev, (unsigned)index_base, *cam, max_bbox_px, (unsigned long long*)keys,
                     (unsigned long long*)culled_big);
  SP3_LAUNCH_CHECK("sp3_render_tris");
  return 0;
}
