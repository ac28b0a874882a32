// RGB-D views (include/spann3r_hip.h, "RGB-D views"): the depth side of a sequence of views with ground truth, one launch for all
// views.  Replaces, on the device, the per-view CPU work of the reference's data-set path for the depth map: the sanitising of
// the data-set classes (spann3r/datasets/seven_scenes.py:123-126), the crop / cv2.resize(INTER_NEAREST) / crop of
// `_crop_resize_if_necessary` (dust3r/datasets/base/base_stereo_view_dataset.py:143-194, dust3r/datasets/utils/cropping.py:54-112),
// depthmap_to_absolute_camera_coordinates (dust3r/utils/geometry.py:165-217), the mask of base_stereo_view_dataset.py:100-103 and
// transpose_to_landscape (:215-220).  Memory-bound gather: 2 or 4 bytes in and 17 bytes out per pixel, no LDS; a lane owns four
// consecutive OUTPUT pixels so that the depth, the mask and the 12-byte point records leave as whole 16-byte (4-byte) stores.
//
// Second entry, sp3_eval_align: the alignment of the reference's eval.py:128-168 (predictions and ground truth of one sequence into
// the world of view 0, with the medians of sp3_ssi_align_stats) and the masked clouds of eval.py:189-191 by the order-preserving
// compaction of csrc/scan.h.
//
// Every operation of the unprojection and of the rotation is rounded on its own (no contraction into FMAs): the file-level pragma
// below is what the compiler honours under its default -ffp-contract=fast-honor-pragmas.
#include "common.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace {

struct ViewPx {
  float z, xc, yc, X, Y, Z;
  uint8_t m;
};

// OpenCV's INTER_NEAREST source index for a given dsize: ifx = 1 / (dst / src) in double, floor, clamp
__device__ __forceinline__ int nearest_src(int xr, int dst, int src) {
  const double ifx = 1.0 / ((double)dst / (double)src);
  const int s = (int)floor((double)xr * ifx);
  return s < src - 1 ? s : src - 1;
}

// output pixel p (row-major in the landscape [out_h, out_w] map) of view d
__device__ __forceinline__ ViewPx view_pixel(const sp3_view_desc& d, int p, int out_w) {
  const int r = p / out_w, c = p - r * out_w;
  const int x = d.transpose ? r : c, y = d.transpose ? c : r;          // pixel of the view's own [h, w] orientation
  const int sx = nearest_src(x + d.l2, d.W2, d.W1), sy = nearest_src(y + d.t2, d.H2, d.H1);
  const int64_t off = (int64_t)(d.crop_t + sy) * d.row_stride + (d.crop_l + sx);
  float raw = d.dtype ? static_cast<const float*>(d.src)[off] : (float)static_cast<const uint16_t*>(d.src)[off];
  if (d.use_raw_invalid && raw == d.raw_invalid) raw = 0.f;
  float z = raw / d.depth_div;                                   // IEEE division (no fast-math in this build)
  if (!isfinite(z)) z = 0.f;
  if (z > d.max_depth) z = 0.f;
  if (z < d.min_depth) z = 0.f;
  ViewPx o;
  o.z = z;
  o.xc = (float)(((double)x - (double)d.cu) * (double)z / (double)d.fu);     // double throughout, rounded once (numpy's promotion)
  o.yc = (float)(((double)y - (double)d.cv) * (double)z / (double)d.fv);
  const float* R = d.pose;
  o.X = ((R[0] * o.xc + R[1] * o.yc) + R[2] * z) + R[3];
  o.Y = ((R[4] * o.xc + R[5] * o.yc) + R[6] * z) + R[7];
  o.Z = ((R[8] * o.xc + R[9] * o.yc) + R[10] * z) + R[11];
  o.m = (uint8_t)(z > 0.f && isfinite(o.X) && isfinite(o.Y) && isfinite(o.Z));
  return o;
}

// grid (pixel blocks, views).  WIDE (npx % 4 == 0, so every view's maps start 16-byte aligned and no group is ragged): a lane owns
// pixels 4i .. 4i+3 and writes one float4 of depth, one dword of mask and three float4 per point map; otherwise one pixel per lane.
template <bool WIDE>
__global__ __launch_bounds__(256) void view_depth_kernel(const sp3_view_desc* __restrict__ descs, int out_w, int npx,
                                                         float* __restrict__ depth, float* __restrict__ pts,
                                                         uint8_t* __restrict__ mask, float* __restrict__ xcam) {
  const sp3_view_desc& d = descs[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int64_t base = (int64_t)blockIdx.y * npx;
  if (WIDE) {
    const int p0 = 4 * i;
    if (p0 >= npx) return;
    ViewPx q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = view_pixel(d, p0 + k, out_w);
    *reinterpret_cast<float4*>(depth + base + p0) = make_float4(q[0].z, q[1].z, q[2].z, q[3].z);
    *reinterpret_cast<uchar4*>(mask + base + p0) = make_uchar4(q[0].m, q[1].m, q[2].m, q[3].m);
    float4* o = reinterpret_cast<float4*>(pts + 3 * (base + p0));
    o[0] = make_float4(q[0].X, q[0].Y, q[0].Z, q[1].X);
    o[1] = make_float4(q[1].Y, q[1].Z, q[2].X, q[2].Y);
    o[2] = make_float4(q[2].Z, q[3].X, q[3].Y, q[3].Z);
    if (xcam) {
      float4* c = reinterpret_cast<float4*>(xcam + 3 * (base + p0));
      c[0] = make_float4(q[0].xc, q[0].yc, q[0].z, q[1].xc);
      c[1] = make_float4(q[1].yc, q[1].z, q[2].xc, q[2].yc);
      c[2] = make_float4(q[2].z, q[3].xc, q[3].yc, q[3].z);
    }
  } else {
    if (i >= npx) return;
    const ViewPx q = view_pixel(d, i, out_w);
    const int64_t e = base + i;
    depth[e] = q.z;
    mask[e] = q.m;
    pts[3 * e] = q.X; pts[3 * e + 1] = q.Y; pts[3 * e + 2] = q.Z;
    if (xcam) { xcam[3 * e] = q.xc; xcam[3 * e + 1] = q.yc; xcam[3 * e + 2] = q.z; }
  }
}

}  // namespace

extern "C" int sp3_view_depth(const sp3_view_desc* descs_host, const sp3_view_desc* descs_dev, int n, int out_h, int out_w,
                              float* depth, float* pts, uint8_t* mask, float* xcam, void* stream) {
  if (n == 0) return 0;
  SP3_CHECK(n > 0 && n <= 65535, "sp3_view_depth: %d views (1..65535 per call)", n);
  SP3_CHECK(descs_host && descs_dev && depth && pts && mask, "sp3_view_depth: null pointer");
  SP3_CHECK(out_h > 0 && out_w > 0 && (int64_t)out_h * out_w < (1 << 28), "sp3_view_depth: bad output size %dx%d", out_w, out_h);
  for (int v = 0; v < n; ++v) {
    const sp3_view_desc& d = descs_host[v];
    SP3_CHECK(d.src && (d.dtype == 0 || d.dtype == 1), "sp3_view_depth: view %d: null source or unknown dtype %d", v, d.dtype);
    SP3_CHECK(d.src_w > 0 && d.src_h > 0 && d.row_stride >= d.src_w, "sp3_view_depth: view %d: bad source geometry", v);
    SP3_CHECK(d.W1 > 0 && d.H1 > 0 && d.crop_l >= 0 && d.crop_t >= 0 && d.crop_l + d.W1 <= d.src_w && d.crop_t + d.H1 <= d.src_h,
              "sp3_view_depth: view %d: first crop (%d,%d)+(%dx%d) outside the %dx%d source", v, d.crop_l, d.crop_t, d.W1, d.H1,
              d.src_w, d.src_h);
    SP3_CHECK(d.w > 0 && d.h > 0 && d.l2 >= 0 && d.t2 >= 0 && d.l2 + d.w <= d.W2 && d.t2 + d.h <= d.H2,
              "sp3_view_depth: view %d: second crop (%d,%d)+(%dx%d) outside the resized image %dx%d", v, d.l2, d.t2, d.w, d.h, d.W2, d.H2);
    SP3_CHECK((d.transpose ? d.w : d.h) == out_h && (d.transpose ? d.h : d.w) == out_w,
              "sp3_view_depth: view %d is %dx%d%s, the call's output is %dx%d", v, d.w, d.h, d.transpose ? " transposed" : "", out_w, out_h);
    SP3_CHECK(d.depth_div != 0.f, "sp3_view_depth: view %d: depth_div = 0", v);
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int npx = out_h * out_w;
  const uintptr_t al = reinterpret_cast<uintptr_t>(depth) | reinterpret_cast<uintptr_t>(pts) | reinterpret_cast<uintptr_t>(xcam);
  if (npx % 4 == 0 && al % 16 == 0 && reinterpret_cast<uintptr_t>(mask) % 4 == 0) {
    hipLaunchKernelGGL(view_depth_kernel<true>, dim3((unsigned)((npx / 4 + 255) / 256), (unsigned)n), dim3(256), 0, st, descs_dev, out_w,
                       npx, depth, pts, mask, xcam);
  } else {
    hipLaunchKernelGGL(view_depth_kernel<false>, dim3((unsigned)((npx + 255) / 256), (unsigned)n), dim3(256), 0, st, descs_dev, out_w,
                       npx, depth, pts, mask, xcam);
  }
  SP3_LAUNCH_CHECK("sp3_view_depth");
  return 0;
}

// ------------------------------------------------------------------------------------------------ evaluation alignment
namespace {

struct AlignArgs {
  const float* pred; const float* gt; const float* pose0; const float* stats;
  float* pred_out; float* gt_out;
  int m, n, B, HW, to_world;
};

// grid (point blocks, m + n stacks, B).  Every point in double from the fp32 inputs, rounded to fp32 once.
__global__ __launch_bounds__(256) void k_eval_align(const AlignArgs a) {
  __shared__ double M[12], Mi[12], sc[4];
  const int b = blockIdx.z, stack = blockIdx.y;
  if (threadIdx.x == 0) {
    const float* m = a.pose0 + 16 * b;
    for (int k = 0; k < 12; ++k) M[k] = m[k];
    const double A = M[5] * M[10] - M[6] * M[9], Bc = -(M[4] * M[10] - M[6] * M[8]), Cc = M[4] * M[9] - M[5] * M[8];
    const double id = 1.0 / (M[0] * A + M[1] * Bc + M[2] * Cc);
    const double r[9] = {A * id, -(M[1] * M[10] - M[2] * M[9]) * id, (M[1] * M[6] - M[2] * M[5]) * id,
                         Bc * id, (M[0] * M[10] - M[2] * M[8]) * id, -(M[0] * M[6] - M[2] * M[4]) * id,
                         Cc * id, -(M[0] * M[9] - M[1] * M[8]) * id, (M[0] * M[5] - M[1] * M[4]) * id};
    for (int i = 0; i < 3; ++i) {
      for (int k = 0; k < 3; ++k) Mi[4 * i + k] = r[3 * i + k];
      Mi[4 * i + 3] = -(r[3 * i] * M[3] + r[3 * i + 1] * M[7] + r[3 * i + 2] * M[11]);
    }
    for (int k = 0; k < 4; ++k) sc[k] = a.stats[4 * b + k];          // gt_shift_z, pred_shift_z, gt_scale, pred_scale
  }
  __syncthreads();
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= a.HW) return;
  const bool is_pred = stack < a.m;
  const int64_t e = ((int64_t)(is_pred ? stack : stack - a.m) * a.B + b) * a.HW + x;
  const float* src = (is_pred ? a.pred : a.gt) + 3 * e;
  float* dst = (is_pred ? a.pred_out : a.gt_out) + 3 * e;
  double px = src[0], py = src[1], pz = src[2];
  if (is_pred) {
    const double ratio = sc[2] / sc[3];
    px *= ratio; py *= ratio; pz = (pz - sc[1]) * ratio;
  } else {
    const double cx = Mi[0] * px + Mi[1] * py + Mi[2] * pz + Mi[3], cy = Mi[4] * px + Mi[5] * py + Mi[6] * pz + Mi[7],
                 cz = Mi[8] * px + Mi[9] * py + Mi[10] * pz + Mi[11];
    px = cx; py = cy; pz = cz - sc[0];
  }
  if (a.to_world) {
    pz += sc[0];
    const double wx = M[0] * px + M[1] * py + M[2] * pz + M[3], wy = M[4] * px + M[5] * py + M[6] * pz + M[7],
                 wz = M[8] * px + M[9] * py + M[10] * pz + M[11];
    px = wx; py = wy; pz = wz;
  }
  dst[0] = (float)px; dst[1] = (float)py; dst[2] = (float)pz;
}

// img fp32 [n][3][HW] in [-1, 1] -> images fp32 [n][HW][3] = (v + 1) / 2
__global__ __launch_bounds__(256) void k_eval_images(const float* __restrict__ img, int n, int HW, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n * HW * 3) return;
  const int64_t px = i / 3;
  const int c = (int)(i - 3 * px);
  const int64_t f = px / HW, x = px - f * HW;
  out[i] = (img[(f * 3 + c) * HW + x] + 1.0f) / 2.0f;
}

__global__ __launch_bounds__(MB) void k_cloud_count(const uint8_t* __restrict__ mask, int64_t n, int* __restrict__ counts) {
  const int64_t p = (int64_t)blockIdx.x * MB + threadIdx.x;
  int total;
  block_rank(p < n && mask[p] != 0, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(MB) void k_cloud_scatter(const uint8_t* __restrict__ mask, int64_t n, const int* __restrict__ offsets,
                                                      const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                                      float* __restrict__ oa, float* __restrict__ ob, float* __restrict__ oc,
                                                      int* __restrict__ src) {
  const int64_t p = (int64_t)blockIdx.x * MB + threadIdx.x;
  const bool keep = p < n && mask[p] != 0;
  int total;
  const int rank = block_rank(keep, total);
  if (!keep) return;
  const int64_t d = (int64_t)offsets[blockIdx.x] + rank;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    oa[3 * d + k] = a[3 * p + k];
    ob[3 * d + k] = b[3 * p + k];
    oc[3 * d + k] = c[3 * p + k];
  }
  src[d] = (int)p;
}

}  // namespace

extern "C" int64_t sp3_eval_align_ws_bytes(int64_t npts) { return 4 * ((npts + MB - 1) / MB + 2) + 16; }

extern "C" int sp3_eval_align(const float* pred, int m, const float* gt, int n, int B, int HW, const float* pose0, const float* stats,
                              int to_world, float* pred_out, float* gt_out, const uint8_t* mask, const float* img, void* ws,
                              float* images, float* cloud_pred, float* cloud_gt, float* cloud_rgb, int32_t* cloud_src, int32_t* count,
                              void* stream) {
  SP3_CHECK(pred && gt && pose0 && stats && pred_out && gt_out, "sp3_eval_align: null pointer");
  SP3_CHECK(m > 0 && n > 0 && B > 0 && B <= 65535 && m + n <= 65535 && HW > 0, "sp3_eval_align: bad sizes m=%d n=%d B=%d HW=%d", m, n, B, HW);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const AlignArgs a{pred, gt, pose0, stats, pred_out, gt_out, m, n, B, HW, to_world};
  hipLaunchKernelGGL(k_eval_align, dim3((unsigned)((HW + 255) / 256), (unsigned)(m + n), (unsigned)B), dim3(256), 0, st, a);
  if (mask != nullptr) {
    SP3_CHECK(B == 1 && m == n, "sp3_eval_align: the clouds need one sequence (B = 1) and one prediction per frame");
    SP3_CHECK(img && ws && images && cloud_pred && cloud_gt && cloud_rgb && cloud_src && count, "sp3_eval_align: null cloud pointer");
    const int64_t N = (int64_t)n * HW;
    SP3_CHECK(N < (1ll << 31) / 4, "sp3_eval_align: %lld points (indices are int32)", (long long)N);
    SP3_CHECK((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "sp3_eval_align: workspace alignment");
    const int nb = (int)((N + MB - 1) / MB);
    int* offsets = static_cast<int*>(ws);
    hipLaunchKernelGGL(k_eval_images, dim3((unsigned)((N * 3 + 255) / 256)), dim3(256), 0, st, img, n, HW, images);
    hipLaunchKernelGGL(k_cloud_count, dim3(nb), dim3(MB), 0, st, mask, N, offsets);
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(SCAN_T), 0, st, offsets, nb, (nb + SCAN_T - 1) / SCAN_T, (int*)count, 0, 0);
    hipLaunchKernelGGL(k_cloud_scatter, dim3(nb), dim3(MB), 0, st, mask, N, (const int*)offsets, (const float*)pred_out,
                       (const float*)gt_out, (const float*)images, cloud_pred, cloud_gt, cloud_rgb, (int*)cloud_src);
  }
  SP3_LAUNCH_CHECK("sp3_eval_align");
  return 0;
}
