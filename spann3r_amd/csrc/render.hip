// Headless point-cloud rendering (demo.py:221-225, spann3r/tools/vis.py): a z-buffered point rasteriser and the colourisers
// of vis_pred_and_imgs; spann3r_amd/vis.py drives these.
//
// The z-buffer is one 64-bit key per pixel, key = (bit pattern of the camera-space depth) << 32 | global point index, all-ones =
// empty.  A depth above z_near >= 0 is a positive fp32, whose bit patterns order like the values, so one unsigned 64-bit atomic min
// per covered pixel keeps the nearest point and, at equal depth, the lowest index: the picture does not depend on the order the
// lanes arrive in.  Keys only ever decrease, so the buffer is persistent: a new frame costs its own points, whatever the cloud holds.
//
// Every fp32 operation of the projection and of the HSV formula is rounded on its own (no contraction into FMAs): the file-level
// pragma below is what the compiler honours under its default -ffp-contract=fast-honor-pragmas.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

#define RB 256              // threads of every block here; the xyz staging buffer holds 3 floats per thread
#ifndef SP3_RENDER_PRETEST
#define SP3_RENDER_PRETEST 1
#endif

namespace {

// The block's RB consecutive [.,3] fp32 triples through LDS: three coalesced dword loads per lane instead of one 12-byte-strided
// triple each; the LDS read back (stride 3 words) is bank-conflict free.  Triples past n read as 0.
__device__ __forceinline__ void load_triples(const float* __restrict__ p, int64_t n, float (&lds)[3 * RB], float& a, float& b, float& c) {
  const int64_t base = (int64_t)blockIdx.x * RB * 3, end = n * 3;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int64_t e = base + j * RB + threadIdx.x;
    lds[j * RB + threadIdx.x] = e < end ? p[e] : 0.f;
  }
  __syncthreads();
  a = lds[3 * threadIdx.x];
  b = lds[3 * threadIdx.x + 1];
  c = lds[3 * threadIdx.x + 2];
}

__global__ __launch_bounds__(RB) void k_render_clear(unsigned long long* __restrict__ keys, int64_t pixels) {
  const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
  if (i < pixels) keys[i] = ~0ull;
}

__global__ __launch_bounds__(RB) void k_render_splat(const float* __restrict__ pts, const float* __restrict__ conf, float conf_thresh,
                                                     int64_t n, unsigned index_base, sp3_render_cam cam,
                                                     unsigned long long* __restrict__ keys) {
  __shared__ float lds[3 * RB];
  float x, y, z;
  load_triples(pts, n, lds, x, y, z);
  const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
  if (i >= n) return;
  if (conf != nullptr) {
    const float c = conf[i];
    if (!((c - 1.0f) / c > conf_thresh)) return;          // the reference's mask (demo.py:213); a NaN confidence drops the point
  }
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return;
  const float xc = ((cam.R[0] * x + cam.R[1] * y) + cam.R[2] * z) + cam.t[0];
  const float yc = ((cam.R[3] * x + cam.R[4] * y) + cam.R[5] * z) + cam.t[1];
  const float zc = ((cam.R[6] * x + cam.R[7] * y) + cam.R[8] * z) + cam.t[2];
  if (!(isfinite(xc) && isfinite(yc) && isfinite(zc)) || zc <= cam.z_near) return;
  const float u = cam.fx * xc / zc + cam.cx, v = cam.fy * yc / zc + cam.cy;
  const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
  // a footprint reaches at most 4 pixels from its centre: anything further out (or not finite) cannot touch the image, and the
  // test keeps the conversions to int in range
  if (!(fu >= -8.0f && fu < (float)(cam.width + 8) && fv >= -8.0f && fv < (float)(cam.height + 8))) return;
  const int off = (cam.point_size - 1) / 2;
  const int x0 = max((int)fu - off, 0), x1 = min((int)fu - off + cam.point_size, cam.width);
  const int y0 = max((int)fv - off, 0), y1 = min((int)fv - off + cam.point_size, cam.height);
  const unsigned long long key = ((unsigned long long)__float_as_uint(zc) << 32) | (unsigned long long)(index_base + (unsigned)i);
  for (int py = y0; py < y1; ++py)
    for (int px = x0; px < x1; ++px) {
      unsigned long long* k = keys + (int64_t)py * cam.width + px;
#if SP3_RENDER_PRETEST
      if (*k <= key) continue;      // (a stale cached value is an older, larger key: the atomic then decides)
#endif
      __hip_atomic_fetch_min(k, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct Px {
  unsigned rgb;      // r | g << 8 | b << 16
  float depth;
  int index;
};
__device__ __forceinline__ Px resolve_px(unsigned long long key, const unsigned* __restrict__ rgba, unsigned background) {
  Px p;
  if (key == ~0ull) {
    p.rgb = background & 0xffffffu;
    p.depth = INFINITY;
    p.index = -1;
  } else {
    const unsigned idx = (unsigned)key;
    p.rgb = rgba[idx] & 0xffffffu;
    p.depth = __uint_as_float((unsigned)(key >> 32));
    p.index = (int)idx;
  }
  return p;
}

struct U3 {
  unsigned a, b, c;
};

// Four consecutive pixels per lane (the [H, W, 3] picture is flat, so rows do not matter): 32 bytes of keys in, 12 bytes of rgb
// (three dwords), a float4 of depth and an int4 of indices out.  `wide` (uniform): the outputs are aligned for those stores;
// otherwise, and for the last pixels of a count that is no multiple of 4, plain element stores.
__global__ __launch_bounds__(RB) void k_render_resolve(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ rgba,
                                                       int64_t pixels, unsigned background, uint8_t* __restrict__ rgb_out,
                                                       float* __restrict__ depth_out, int* __restrict__ index_out, int wide) {
  const int64_t p0 = ((int64_t)blockIdx.x * RB + threadIdx.x) * 4;
  if (p0 >= pixels) return;
  if (wide && p0 + 4 <= pixels) {
    const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(keys + p0), k23 = *reinterpret_cast<const ulonglong2*>(keys + p0 + 2);
    const Px a = resolve_px(k01.x, rgba, background), b = resolve_px(k01.y, rgba, background);
    const Px c = resolve_px(k23.x, rgba, background), d = resolve_px(k23.y, rgba, background);
    U3 o;
    o.a = a.rgb | (b.rgb << 24);
    o.b = (b.rgb >> 8) | (c.rgb << 16);
    o.c = (c.rgb >> 16) | (d.rgb << 8);
    *reinterpret_cast<U3*>(rgb_out + p0 * 3) = o;
    if (depth_out != nullptr) *reinterpret_cast<float4*>(depth_out + p0) = make_float4(a.depth, b.depth, c.depth, d.depth);
    if (index_out != nullptr) *reinterpret_cast<int4*>(index_out + p0) = make_int4(a.index, b.index, c.index, d.index);
    return;
  }
  const int64_t p1 = p0 + 4 < pixels ? p0 + 4 : pixels;
  for (int64_t p = p0; p < p1; ++p) {
    const Px a = resolve_px(keys[p], rgba, background);
    rgb_out[p * 3] = (uint8_t)a.rgb;
    rgb_out[p * 3 + 1] = (uint8_t)(a.rgb >> 8);
    rgb_out[p * 3 + 2] = (uint8_t)(a.rgb >> 16);
    if (depth_out != nullptr) depth_out[p] = a.depth;
    if (index_out != nullptr) index_out[p] = a.index;
  }
}

__device__ __forceinline__ unsigned unorm8(float c) {      // floor(c * 255 + 0.5), clamped; NaN gives 0
  const float s = floorf(c * 255.0f + 0.5f);
  return s >= 255.0f ? 255u : (s > 0.0f ? (unsigned)s : 0u);
}

__global__ __launch_bounds__(RB) void k_pack_rgba8(const float* __restrict__ img, int64_t n, unsigned* __restrict__ rgba) {
  __shared__ float lds[3 * RB];
  float r, g, b;
  load_triples(img, n, lds, r, g, b);
  const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
  if (i < n) rgba[i] = unorm8(r) | (unorm8(g) << 8) | (unorm8(b) << 16) | 0xff000000u;
}

__device__ __forceinline__ unsigned trunc255(float c) {      // uint8(trunc(255 c)) for c in [0, 1]; clamped outside, NaN gives 0
  const float s = c * 255.0f;
  return s >= 255.0f ? 255u : (s > 0.0f ? (unsigned)s : 0u);
}

// matplotlib.colors.hsv_to_rgb of (h, s, v) = 1 - x, in fp32, one rounding per operation
__global__ __launch_bounds__(RB) void k_colorize_hsv(const float* __restrict__ x, int64_t n, uint8_t* __restrict__ out) {
  __shared__ float lds[3 * RB];
  float x0, x1, x2;
  load_triples(x, n, lds, x0, x1, x2);
  const int64_t e = (int64_t)blockIdx.x * RB + threadIdx.x;
  if (e >= n) return;
  const float h = 1.0f - x0, s = 1.0f - x1, v = 1.0f - x2;
  const float h6 = h * 6.0f;
  const int i = h6 >= 6.0f ? 6 : (h6 > 0.0f ? (int)h6 : 0);
  const float f = h6 - (float)i;
  const float p = v * (1.0f - s);
  const float q = v * (1.0f - s * f);
  const float t = v * (1.0f - s * (1.0f - f));
  float r, g, b;
  switch (i % 6) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
  if (s == 0.0f) r = g = b = v;
  out[e * 3] = (uint8_t)trunc255(r);
  out[e * 3 + 1] = (uint8_t)trunc255(g);
  out[e * 3 + 2] = (uint8_t)trunc255(b);
}

__global__ __launch_bounds__(RB) void k_colorize_lut(const float* __restrict__ x, int64_t n, const unsigned* __restrict__ lut,
                                                     unsigned* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * RB + threadIdx.x;
  if (i >= n) return;
  const float s = x[i] * 256.0f;
  out[i] = lut[s >= 255.0f ? 255 : (s > 0.0f ? (int)s : 0)];
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + RB - 1) / RB); }
const int64_t MAX_ELEMS = (int64_t)RB * 0x7fffffff;

}  // namespace

extern "C" int sp3_render_clear(uint64_t* keys, int64_t pixels, void* stream) {
  SP3_CHECK(keys != nullptr, "sp3_render_clear: null key buffer");
  SP3_CHECK(pixels > 0 && pixels <= 0x7fffffff, "sp3_render_clear: pixels %lld outside 1..2^31-1", (long long)pixels);
  hipLaunchKernelGGL(k_render_clear, dim3(blocks_for(pixels)), dim3(RB), 0, (hipStream_t)stream, (unsigned long long*)keys, pixels);
  SP3_LAUNCH_CHECK("sp3_render_clear");
  return 0;
}

static int check_cam(const char* what, const sp3_render_cam* cam) {
  SP3_CHECK(cam != nullptr, "%s: null camera", what);
  SP3_CHECK(cam->width > 0 && cam->height > 0 && (int64_t)cam->width * cam->height <= 0x7fffffff && cam->width <= (1 << 24) &&
                cam->height <= (1 << 24),
            "%s: image %d x %d outside 1..2^24 per side, 2^31-1 pixels", what, cam->width, cam->height);
  SP3_CHECK(cam->point_size >= 1 && cam->point_size <= 8, "%s: point_size %d outside 1..8", what, cam->point_size);
  SP3_CHECK(cam->z_near >= 0.f, "%s: z_near %g must be >= 0 (depth keys are positive fp32 bit patterns)", what, (double)cam->z_near);
  return 0;
}

extern "C" int sp3_render_splat(const float* pts, const float* conf, float conf_thresh, int64_t n, int64_t index_base,
                                const sp3_render_cam* cam, uint64_t* keys, void* stream) {
  if (check_cam("sp3_render_splat", cam)) return 1;
  SP3_CHECK(n >= 0 && index_base >= 0, "sp3_render_splat: negative n %lld or index_base %lld", (long long)n, (long long)index_base);
  SP3_CHECK(index_base + n < 0xffffffffLL,
            "sp3_render_splat: index overflow: index_base %lld + n %lld reaches 2^32-1 (point indices are the low 32 bits of a key, all-ones is empty)",
            (long long)index_base, (long long)n);
  if (n == 0) return 0;
  SP3_CHECK(pts != nullptr && keys != nullptr, "sp3_render_splat: null pts/keys");
  hipLaunchKernelGGL(k_render_splat, dim3(blocks_for(n)), dim3(RB), 0, (hipStream_t)stream, pts, conf, conf_thresh, n, (unsigned)index_base,
                     *cam, (unsigned long long*)keys);
  SP3_LAUNCH_CHECK("sp3_render_splat");
  return 0;
}

extern "C" int sp3_render_resolve(const uint64_t* keys, const uint32_t* rgba, const sp3_render_cam* cam, uint32_t background,
                                  uint8_t* rgb_out, float* depth_out, int32_t* index_out, void* stream) {
  if (check_cam("sp3_render_resolve", cam)) return 1;
  SP3_CHECK(keys != nullptr && rgb_out != nullptr, "sp3_render_resolve: null keys/rgb_out");
  SP3_CHECK(((uintptr_t)keys & 7) == 0 && ((uintptr_t)rgba & 3) == 0 && ((uintptr_t)depth_out & 3) == 0 && ((uintptr_t)index_out & 3) == 0,
            "sp3_render_resolve: keys / rgba / depth_out / index_out not aligned to their element size");
  const int64_t pixels = (int64_t)cam->width * cam->height;
  const int wide = ((uintptr_t)keys & 15) == 0 && ((uintptr_t)rgb_out & 3) == 0 && ((uintptr_t)depth_out & 15) == 0 && ((uintptr_t)index_out & 15) == 0;
  hipLaunchKernelGGL(k_render_resolve, dim3(blocks_for((pixels + 3) / 4)), dim3(RB), 0, (hipStream_t)stream, (const unsigned long long*)keys,
                     (const unsigned*)rgba, pixels, (unsigned)background, rgb_out, depth_out, (int*)index_out, wide);
  SP3_LAUNCH_CHECK("sp3_render_resolve");
  return 0;
}

extern "C" int sp3_pack_rgba8(const float* img, int64_t n, uint32_t* rgba, void* stream) {
  SP3_CHECK(n >= 0 && n <= MAX_ELEMS, "sp3_pack_rgba8: n %lld out of range", (long long)n);
  if (n == 0) return 0;
  SP3_CHECK(img != nullptr && rgba != nullptr, "sp3_pack_rgba8: null img/rgba");
  hipLaunchKernelGGL(k_pack_rgba8, dim3(blocks_for(n)), dim3(RB), 0, (hipStream_t)stream, img, n, (unsigned*)rgba);
  SP3_LAUNCH_CHECK("sp3_pack_rgba8");
  return 0;
}

extern "C" int sp3_colorize_hsv(const float* x, int64_t n, uint8_t* out, void* stream) {
  SP3_CHECK(n >= 0 && n <= MAX_ELEMS, "sp3_colorize_hsv: n %lld out of range", (long long)n);
  if (n == 0) return 0;
  SP3_CHECK(x != nullptr && out != nullptr, "sp3_colorize_hsv: null x/out");
  hipLaunchKernelGGL(k_colorize_hsv, dim3(blocks_for(n)), dim3(RB), 0, (hipStream_t)stream, x, n, out);
  SP3_LAUNCH_CHECK("sp3_colorize_hsv");
  return 0;
}

extern "C" int sp3_colorize_lut(const float* x, int64_t n, const uint8_t* lut, uint8_t* out, void* stream) {
  SP3_CHECK(n >= 0 && n <= MAX_ELEMS, "sp3_colorize_lut: n %lld out of range", (long long)n);
  if (n == 0) return 0;
  SP3_CHECK(x != nullptr && lut != nullptr && out != nullptr, "sp3_colorize_lut: null x/lut/out");
  SP3_CHECK(((uintptr_t)lut & 3) == 0 && ((uintptr_t)out & 3) == 0, "sp3_colorize_lut: lut / out must be 4-byte aligned (one rgba entry per word)");
  hipLaunchKernelGGL(k_colorize_lut, dim3(blocks_for(n)), dim3(RB), 0, (hipStream_t)stream, x, n, (const unsigned*)lut, (unsigned*)out);
  SP3_LAUNCH_CHECK("sp3_colorize_lut");
  return 0;
}
