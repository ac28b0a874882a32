// The face classes of "Mesh visibility" (include/spann3r_hip.h, rule 4; spann3r_amd/mesh.py cull_to_views drives this;
// tests/mesh_visibility_ref.py restates the rule): from the number of views that see every vertex to one int32 per face that
// sp3_mesh_select_faces (csrc/mesh_components.hip) takes as a component id -- 1 keep, 0 drop, -1 a face with an index outside 0..V-1,
// whose vertices are never looked up.  The ordered compaction is that entry point's; nothing is compacted here.
// The kernels that decide visibility itself are the front ends k_ray_occluded and k_point_views of csrc/ray_kernels.h, instantiated
// with the grid's walk in csrc/mesh_ray.hip and with the tree's in csrc/mesh_bvh.hip.
#include "cell_grid.h"

namespace {

enum { VIS_ANY = 0, VIS_ALL = 1 };

// one lane per face
__global__ __launch_bounds__(TB) void k_vis_face_class(const int* __restrict__ faces, int64_t nfaces, int nverts, const int* __restrict__ count,
                                                        int min_views, int mode, int* __restrict__ cls) {
  const int64_t f = (int64_t)blockIdx.x * TB + threadIdx.x;
  if (f >= nfaces) return;
  const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  int k = -1;
  if ((unsigned)a < (unsigned)nverts && (unsigned)b < (unsigned)nverts && (unsigned)c < (unsigned)nverts) {
    const bool sa = count[a] >= min_views, sb = count[b] >= min_views, sc = count[c] >= min_views;
    k = (mode == VIS_ALL ? (sa && sb && sc) : (sa || sb || sc)) ? 1 : 0;
  }
  cls[f] = k;
}

}  // namespace

extern "C" int sp3_mesh_vis_face_class(const int32_t* faces, int64_t nfaces, int64_t nverts, const int32_t* count, int min_views, int mode,
                                       int32_t* cls, void* stream) {
  SP3_CHECK(sizes_ok_or_empty(nverts, nfaces), "sp3_mesh_vis_face_class: nverts %lld or nfaces %lld out of range (both below 2^31 - 1)",
            (long long)nverts, (long long)nfaces);
  SP3_CHECK(mode == VIS_ANY || mode == VIS_ALL, "sp3_mesh_vis_face_class: mode %d must be 0 (any) or 1 (all)", mode);
  if (nfaces == 0) return 0;
  SP3_CHECK(faces && cls && (nverts == 0 || count), "sp3_mesh_vis_face_class: null pointer");
  k_vis_face_class<<<blocks_for(nfaces), TB, 0, (hipStream_t)stream>>>((const int*)faces, nfaces, (int)nverts, (const int*)count, min_views, mode,
                                                                       (int*)cls);
  SP3_LAUNCH_CHECK("sp3_mesh_vis_face_class");
  return 0;
}
