// Multi-view consistency of pointmaps (include/spann3r_hip.h, "Multi-view consistency"; spann3r_amd/multiview.py drives these): every
// pixel's world point is looked up in every other frame of the table, classed as in front of, behind or in agreement with what that
// frame measured there, and its confidence is clipped where a more confident frame looks straight through it.
//
// ONE kernel template does everything.  A lane owns pixel q of frame i (i from blockIdx.z, plus a base for the per-frame launches of
// the sequence order); a wave owns an 8 x 8 pixel tile and a workgroup a 16 x 16 block (RC_TILE, view_grid: csrc/tsdf.h), so that
// the lanes of a wave gather neighbouring pixels of frame j.  The j loop is wave-uniform: the descriptors of both tables arrive by
// scalar loads of read-only tables, as in integrate_voxel; a lane that skips a frame just continues.  The four counts stay in
// registers; a pixel makes one 16-byte store of its counts and, when asked, one 4-byte store of its confidence.  No atomics, no LDS,
// no lane waits for another.
//
// The lookup is integrate_voxel's (csrc/tsdf.h), restated here step by step for a frame that has pts; that rule is not touched.
// SEQ = false: every frame is judged against the original confidences (sp3_multiview_counts, one launch over all (i, tile)).
// SEQ = true: launch i covers frame i only and reads the cleaned confidence out[j].conf_out of the frames j < i, which the earlier
// launches wrote (sp3_multiview_clean, T launches; the launch boundaries are the only hand-offs).
//
// Every fp32 operation is rounded on its own (no contraction into FMAs): the file-level pragma below.
#include "common.h"
#include "tsdf.h"
#include <math.h>

#include <algorithm>
#include <vector>

#pragma clang fp contract(off)

namespace {

template <bool SEQ>
__global__ __launch_bounds__(RC_TILE * RC_TILE) void k_multiview(const sp3_tsdf_frame* __restrict__ frames,
                                                                const sp3_multiview_out* __restrict__ outs, int T, int i0, float tol) {
  const int i = i0 + (int)blockIdx.z;      // (wave-uniform, as j below: the descriptor fields arrive by scalar loads)
  const sp3_tsdf_frame& fi = frames[i];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int qx = blockIdx.x * RC_TILE + (wave & 1) * 8 + (lane & 7);
  const int qy = blockIdx.y * RC_TILE + (wave >> 1) * 8 + (lane >> 3);
  if (qx >= fi.w || qy >= fi.h) return;
  const int64_t q = (int64_t)qy * fi.row_stride + qx;
  const bool has_ci = fi.pixel_weight != nullptr;
  const float ci = has_ci ? fi.pixel_weight[q] : 0.f;
  int seen = 0, agree = 0, front = 0, stronger = 0;
  bool bad = false;
  if (fi.valid == nullptr || fi.valid[q] != 0) {
    const float x = fi.pts[3 * q], y = fi.pts[3 * q + 1], z = fi.pts[3 * q + 2];
    const float tlo = 1.0f - tol, thi = 1.0f + tol;
    for (int j = 0; j < T; ++j) {
      if (j == i) continue;
      const sp3_tsdf_frame& fr = frames[j];
      const float* m = fr.w2c;
      const float zc = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
      if (!(zc > 0.f)) continue;
      const float xc = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
      const float yc = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
      const float u = fr.fu * xc / zc + fr.cu, v = fr.fv * yc / zc + fr.cv;
      const float fpx = floorf(u + 0.5f), fpy = floorf(v + 0.5f);
      if (!(fpx >= 0.f && fpx < (float)fr.w && fpy >= 0.f && fpy < (float)fr.h)) continue;      // (a NaN fails the test)
      const int64_t p = (int64_t)fpy * fr.row_stride + (int64_t)fpx;
      if (fr.valid != nullptr && fr.valid[p] == 0) continue;
      const float X = fr.pts[3 * p], Y = fr.pts[3 * p + 1], Z = fr.pts[3 * p + 2];
      const float d = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11];
      if (!isfinite(d) || d <= 0.f) continue;
      ++seen;
      const float lo = tlo * d, hi = thi * d;
      if (zc < lo) {
        ++front;
        if (has_ci && fr.pixel_weight != nullptr) {
          const bool st = ci < fr.pixel_weight[p];      // (a NaN on either side fails)
          stronger += st ? 1 : 0;
          if (SEQ && j < i)
            bad = bad || ci < outs[j].conf_out[p];      // the state of frame j: cleaned by launch j
          else
            bad = bad || st;
        }
      } else if (!(zc > hi)) {
        ++agree;
      }
    }
  }
  const sp3_multiview_out& o = outs[i];
  if (o.counts != nullptr) *reinterpret_cast<int4*>(o.counts + 4 * q) = make_int4(seen, agree, front, stronger);
  if (o.conf_out != nullptr) o.conf_out[q] = bad ? (ci < o.max_bad_conf ? ci : o.max_bad_conf) : ci;
}

// the checks the two entry points share (T >= 1); need_conf_out: every frame must have one.  -> the largest width and height
int check_multiview(const char* what, const sp3_tsdf_frame* frames_host, const sp3_tsdf_frame* frames_dev, int T, float tol,
                    const sp3_multiview_out* out_host, const sp3_multiview_out* out_dev, bool need_conf_out, int& wmax, int& hmax) {
  SP3_CHECK(T <= 65535, "%s: T %d must stay below 2^16", what, T);
  SP3_CHECK(frames_host != nullptr && out_host != nullptr, "%s: null frames/out", what);
  SP3_CHECK(tol >= 0.f && tol < 1.f, "%s: tol %g must lie in [0, 1)", what, (double)tol);      // (a NaN fails)
  if (check_frames(what, frames_host, T, false, nullptr)) return 1;
  bool any_conf = false;
  wmax = hmax = 0;
  for (int f = 0; f < T; ++f) {
    SP3_CHECK(frames_host[f].depth == nullptr, "%s: frame %d gives depth: multi-view consistency takes pointmaps (pts)", what, f);
    const sp3_multiview_out& o = out_host[f];
    SP3_CHECK(o.max_bad_conf == o.max_bad_conf, "%s: frame %d: max_bad_conf is NaN", what, f);
    SP3_CHECK(((uintptr_t)o.counts & 15) == 0, "%s: frame %d: counts must be 16-byte aligned", what, f);
    SP3_CHECK(!need_conf_out || o.conf_out != nullptr, "%s: frame %d: null conf_out", what, f);
    any_conf = any_conf || o.conf_out != nullptr;
    wmax = frames_host[f].w > wmax ? frames_host[f].w : wmax;
    hmax = frames_host[f].h > hmax ? frames_host[f].h : hmax;
  }
  if (any_conf) {
    std::vector<const float*> in(T), out;
    for (int f = 0; f < T; ++f) {
      SP3_CHECK(frames_host[f].pixel_weight != nullptr, "%s: frame %d has no pixel_weight but a conf_out is asked for", what, f);
      in[f] = frames_host[f].pixel_weight;
      if (out_host[f].conf_out != nullptr) out.push_back(out_host[f].conf_out);
    }
    std::sort(in.begin(), in.end());
    std::sort(out.begin(), out.end());
    for (size_t e = 0; e < out.size(); ++e) {
      SP3_CHECK(!std::binary_search(in.begin(), in.end(), out[e]), "%s: a conf_out aliases a pixel_weight", what);
      SP3_CHECK(e == 0 || out[e] != out[e - 1], "%s: two frames share a conf_out", what);
    }
  }
  SP3_CHECK(frames_dev != nullptr && out_dev != nullptr, "%s: null device copy of frames/out", what);      // (last: nothing launches without it)
  return 0;
}

}  // namespace

extern "C" int sp3_multiview_counts(const sp3_tsdf_frame* frames_host, const sp3_tsdf_frame* frames_dev, int T, float tol,
                                    const sp3_multiview_out* out_host, const sp3_multiview_out* out_dev, void* stream) {
  SP3_CHECK(T >= 0, "sp3_multiview_counts: T %d must be >= 0", T);
  if (T == 0) return 0;
  int wmax, hmax;
  if (check_multiview("sp3_multiview_counts", frames_host, frames_dev, T, tol, out_host, out_dev, false, wmax, hmax)) return 1;
  dim3 grid;
  if (view_grid("sp3_multiview_counts", wmax, hmax, T, grid)) return 1;
  hipLaunchKernelGGL(k_multiview<false>, grid, dim3(RC_TILE * RC_TILE), 0, (hipStream_t)stream, frames_dev, out_dev, T, 0, tol);
  SP3_LAUNCH_CHECK("sp3_multiview_counts");
  return 0;
}

extern "C" int sp3_multiview_clean(const sp3_tsdf_frame* frames_host, const sp3_tsdf_frame* frames_dev, int T, float tol,
                                   const sp3_multiview_out* out_host, const sp3_multiview_out* out_dev, void* stream) {
  SP3_CHECK(T >= 0, "sp3_multiview_clean: T %d must be >= 0", T);
  if (T == 0) return 0;
  int wmax, hmax;
  if (check_multiview("sp3_multiview_clean", frames_host, frames_dev, T, tol, out_host, out_dev, true, wmax, hmax)) return 1;
  dim3 grid;
  if (view_grid("sp3_multiview_clean", wmax, hmax, 1, grid)) return 1;      // (every frame's grid is checked before the first launch)
  for (int i = 0; i < T; ++i) {
    if (view_grid("sp3_multiview_clean", frames_host[i].w, frames_host[i].h, 1, grid)) return 1;
    hipLaunchKernelGGL(k_multiview<true>, grid, dim3(RC_TILE * RC_TILE), 0, (hipStream_t)stream, frames_dev, out_dev, T, i, tol);
    SP3_LAUNCH_CHECK("sp3_multiview_clean");
  }
  return 0;
}
