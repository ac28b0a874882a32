"""TSDF fusion on the device: one welded surface per reconstruction.

The reference stops at per-frame pointmap sheets (app.py's triangle soup) and at the comment `# Get depth from pcd and run TSDFusion`
(eval.py:241).  Here a truncated signed distance volume is integrated from depth maps or world pointmaps (sp3_tsdf_integrate: one
launch for all frames of a call, one lane per voxel) and the zero level is extracted by marching tetrahedra as a welded, indexed
triangle mesh (sp3_tsdf_extract: two order-preserving compactions); csrc/fusion.hip, rules in include/spann3r_hip.h "TSDF fusion".
`mesh.compact_vertices` then drops the vertices no face uses, applies scale / transform and gives the bounds, so `extract_mesh`
returns the dict shape of `mesh.scene_mesh` and `mesh.write_glb` takes it as it is.

What is unpinned: there is no reference implementation of the fusion (Open3D is not available and the reference has only the
comment); tests/fusion_ref.py restates the header's rules in numpy and the kernels are checked against that.  `fuse_sequence`
inherits whatever error `estimate_poses` and the single shared focal of `estimate_focal_knowing_depth` have.
torch provides memory; there is no CPU path."""
import ctypes as C
import math

import numpy as np
import torch

from . import lib as L
from . import mesh as M

INDEX_LIMIT = (2 ** 31 - 1) // 7        # voxels: 7 n < 2^31 (int32 vertex indices, 7 edge slots per voxel)
BRICK_MESH_LIMIT = (2 ** 31 - 1) // (12 * 512)      # bricks: 12 * 512 n_bricks < 2^31 (sp3_tsdf_brick_extract's int32 indices)


def _dev(x, name):
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s: expected a CUDA tensor, got %s" % (name, type(x).__name__))
    if not x.is_cuda:
        raise RuntimeError("%s: fusion runs on the GPU (HIP kernels); there is no CPU path -- pass a CUDA tensor" % name)
    return x


def _check_dims(dims):
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3 or min(dims) < 0:
        raise ValueError("TSDFVolume: dims %s must be three sizes (nx, ny, nz) >= 0" % (dims,))
    if dims[0] * dims[1] * dims[2] > INDEX_LIMIT:
        raise ValueError("TSDFVolume: dims %s over the index limit: %d voxels, 7 nx ny nz must stay below 2^31 (int32 vertex and face indices)"
                         % (dims, dims[0] * dims[1] * dims[2]))
    return dims


def _frames_list(x, name, tail, optional=False):
    """a [T, h, w(, 3)] stack or a list of [h, w(, 3)] maps -> list of device tensors (None stays None; with `optional` a list may hold
    None for a frame without that map)"""
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        if x.dim() != 3 + len(tail):
            raise RuntimeError("integrate: %s %s must be a [T, h, w%s] stack or a list of maps" % (name, tuple(x.shape), ", 3" if tail else ""))
        x = list(x)
    out = []
    for i, m in enumerate(x):
        if m is None and optional:
            out.append(None)
            continue
        m = _dev(m, "integrate: %s[%d]" % (name, i))
        if m.dim() != 2 + len(tail) or tuple(m.shape[2:]) != tail:
            raise RuntimeError("integrate: %s[%d] %s must be [h, w%s]" % (name, i, tuple(m.shape), ", 3" if tail else ""))
        out.append(m)
    return out


def _host_array(x):
    """an array, a tensor (host or device) or a non-empty list of them -> float64 numpy"""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    elif isinstance(x, (list, tuple)) and len(x):
        x = np.stack([m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m) for m in x])
    return np.asarray(x, np.float64)


def _host_mats(x, T, shape, name):
    """one matrix or T of them (array, tensor or list, host or device) -> float64 numpy [T, *shape]"""
    x = _host_array(x)
    if x.shape == shape:
        x = np.broadcast_to(x, (T,) + shape)
    if x.shape != (T,) + shape:
        raise ValueError("integrate: %s %s must be %s or [%d, %d, %d]" % (name, x.shape, list(shape), T, shape[0], shape[1]))
    return x


def camera_tables(intrinsics, cam2world, T):
    """The host side of `integrate`: intrinsics [3, 3] or [T, 3, 3], cam2world [T, 4, 4] -> (fu, fv, cu, cv float64 [T, 4],
    world-to-camera fp32 [T, 12]), the poses inverted in float64.  Raises for a skewed K or a non-finite or singular pose."""
    K = _host_mats(intrinsics, T, (3, 3), "intrinsics")
    P = _host_mats(cam2world, T, (4, 4), "cam2world")
    for i in range(T):
        if K[i, 0, 1] != 0.0 or K[i, 1, 0] != 0.0:
            raise ValueError("integrate: frame %d: intrinsics with a skew term" % i)
        if not np.isfinite(K[i]).all():
            raise ValueError("integrate: frame %d: non-finite intrinsics" % i)
        if not np.isfinite(P[i]).all():
            raise ValueError("integrate: frame %d: camera pose must be a finite 4x4 cam2world matrix" % i)
    try:
        w2c = np.linalg.inv(P) if T else P
    except np.linalg.LinAlgError:
        raise ValueError("integrate: a camera pose is singular")
    if not np.isfinite(w2c).all():
        raise ValueError("integrate: a camera pose is singular")
    return np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], axis=1), w2c[:, :3, :].reshape(T, 12).astype(np.float32)


class _Volume:
    """What TSDFVolume and BrickTSDFVolume share: the lattice parameters, the frame and view descriptor tables, the argument handling
    of integrate / raycast / extract.  A volume class adds its storage (tsdf, weight, rgb or None, dims) and its launches:
    integrate_table, _raycast_launch, extract_raw."""

    def _set_lattice(self, origin, voxel_size, trunc, device):
        """origin, voxel_size, trunc (None: 3 voxels) and device, validated; messages carry the volume class's name"""
        name = type(self).__name__
        origin = np.asarray(origin, np.float64).reshape(-1)
        if origin.shape != (3,) or not np.isfinite(origin).all():
            raise ValueError("%s: origin must be three finite numbers" % name)
        self.voxel_size = float(np.float32(voxel_size))
        if not (self.voxel_size > 0 and math.isfinite(self.voxel_size)):
            raise ValueError("%s: voxel_size must be positive and finite, got %r" % (name, voxel_size))
        self.trunc = float(np.float32(3.0 * self.voxel_size if trunc is None else trunc))
        if not (self.trunc > 0 and math.isfinite(self.trunc)):
            raise ValueError("%s: trunc must be positive and finite, got %r" % (name, trunc))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("%s: fusion runs on the GPU (HIP kernels); there is no CPU path" % name)
        self.origin = origin.astype(np.float32)
        self._origin_c = (C.c_float * 3)(*self.origin.tolist())

    def integrate(self, depth=None, pts=None, intrinsics=None, cam2world=None, valid=None, weight=None, images=None):
        """T frames into the volume in ONE launch.  depth [T, h, w] (camera z) or pts [T, h, w, 3] (world points; the depth of a pixel
        is the z of its point in that frame's camera) -- stacks or lists of device tensors; intrinsics [3, 3] or [T, 3, 3];
        cam2world [T, 4, 4], inverted in float64 on the host; valid bool / uint8, weight fp32 (lists of these may hold None for single
        frames) and images (floats in [0, 1], [T, h, w, 3]; required when the volume has colours) are optional.  Nothing synchronises."""
        if (depth is None) == (pts is None):
            raise ValueError("integrate: give depth or pts, exactly one")
        if intrinsics is None or cam2world is None:
            raise ValueError("integrate: intrinsics and cam2world are required")
        src = _frames_list(depth, "depth", ()) if depth is not None else _frames_list(pts, "pts", (3,))
        T = len(src)
        if T == 0:
            return self
        return self.integrate_table(self.frame_table(src, depth is not None, intrinsics, cam2world, valid, weight, images))

    def frame_table(self, src, is_depth, intrinsics, cam2world, valid=None, weight=None, images=None, need_images=True):
        """The descriptor table of `integrate` for the list `src` of depth maps (is_depth) or pointmaps: (host table, device copy, T,
        the tensors it points to).  integrate_table launches it; a table can be launched again as long as its tensors live.
        need_images=False: the table is not for integrating (BrickTSDFVolume.allocate), so a volume with colours asks for no images."""
        T = len(src)
        depth = src if is_depth else None
        fk, w2c = camera_tables(intrinsics, cam2world, T)
        maps = {"valid": _frames_list(valid, "valid", (), True), "weight": _frames_list(weight, "weight", (), True),
                "images": _frames_list(images, "images", (3,))}
        for name, m in maps.items():
            if m is not None and len(m) != T:
                raise RuntimeError("integrate: mismatched lengths: %d frames, %d %s maps" % (T, len(m), name))
        if need_images and self.rgb is not None and maps["images"] is None:
            raise ValueError("integrate: the volume has colours: pass images (or build it with color=False)")
        lib = L.load()
        st = L.stream_ptr()
        table = (L.TsdfFrame * T)()
        keep = []
        for i in range(T):
            s = src[i].float().contiguous()
            h, w = s.shape[:2]
            e = table[i]
            if depth is not None:
                e.depth, e.pts = s.data_ptr(), None
            else:
                e.depth, e.pts = None, s.data_ptr()
            keep.append(s)
            for name, m in maps.items():
                if m is not None and m[i] is not None and tuple(m[i].shape[:2]) != (h, w):
                    raise RuntimeError("integrate: mismatched shapes: frame %d is %d x %d, its %s map %s" % (i, h, w, name, tuple(m[i].shape)))
            if maps["valid"] is not None and maps["valid"][i] is not None:
                v = maps["valid"][i].to(torch.uint8).contiguous()
                e.valid = v.data_ptr()
                keep.append(v)
            if maps["weight"] is not None and maps["weight"][i] is not None:
                a = maps["weight"][i].float().contiguous()
                e.pixel_weight = a.data_ptr()
                keep.append(a)
            if maps["images"] is not None and self.rgb is not None:
                c = maps["images"][i].float().contiguous()
                rgba = torch.empty(h * w, dtype=torch.int32, device=self.device)
                L.check(lib.sp3_pack_rgba8(c.data_ptr(), h * w, rgba.data_ptr(), st), "sp3_pack_rgba8")
                e.rgba = rgba.data_ptr()
                keep += [c, rgba]
            e.row_stride, e.w, e.h = w, w, h
            e.fu, e.fv, e.cu, e.cv = (float(x) for x in fk[i])
            e.w2c[:] = w2c[i].tolist()
        table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(self.device)
        return table, table_d, T, keep

    def raycast(self, intrinsics, cam2world, size, near=0.0, far=math.inf, step_voxels=1.0, min_weight=1.0, vertices=True, normals=True,
                colors=None):
        """The zero level seen from T cameras in ONE launch, with no meshing (sp3_tsdf_raycast): intrinsics [3, 3] or [T, 3, 3],
        cam2world [T, 4, 4] (or one [4, 4]), size = (h, w).  -> dict of device tensors: depth fp32 [T, h, w] (camera z, 0 = miss) and, as
        asked, vertices fp32 [T, h, w, 3] (world), normals fp32 [T, h, w, 3] (unit, outward), colors uint8 [T, h, w, 4] (default: whether
        the volume has colours).  The march takes steps of step_voxels (>= 0.25) voxels of ray length between near and far (camera z).
        Skewed intrinsics and non-finite or singular poses are refused as `camera_tables` refuses them.  Nothing synchronises."""
        return self.raycast_table(self.view_table(intrinsics, cam2world, size, near, far, vertices, normals, colors), step_voxels, min_weight)

    def view_table(self, intrinsics, cam2world, size, near=0.0, far=math.inf, vertices=True, normals=True, colors=None):
        """The descriptor table of `raycast` and the maps it points to: (host table, device copy, T, the dict `raycast` returns).
        raycast_table launches it; a table can be launched again, into the same maps."""
        h, w = (int(x) for x in size)
        if h < 1 or w < 1:
            raise ValueError("raycast: size %s must be (h, w) >= 1" % (size,))
        if not (0.0 <= near <= far):
            raise ValueError("raycast: 0 <= near <= far, got near %r, far %r" % (near, far))
        colors = self.rgb is not None if colors is None else bool(colors)
        if colors and self.rgb is None:
            raise ValueError("raycast: colors asked of a volume without colours")
        P = _host_array(cam2world)
        P = P[None] if P.ndim == 2 else P.reshape(-1, 4, 4) if P.size == 0 else P
        if P.ndim != 3 or P.shape[1:] != (4, 4):
            raise ValueError("raycast: cam2world %s must be [4, 4] or [T, 4, 4]" % (P.shape,))
        T = P.shape[0]
        fk, _ = camera_tables(intrinsics, P, T)                  # (the inverse is only computed for its checks)
        if not (fk[:, :2] != 0).all():
            raise ValueError("raycast: intrinsics with a zero focal length")
        out = dict(depth=torch.empty((T, h, w), dtype=torch.float32, device=self.device))
        if vertices:
            out["vertices"] = torch.empty((T, h, w, 3), dtype=torch.float32, device=self.device)
        if normals:
            out["normals"] = torch.empty((T, h, w, 3), dtype=torch.float32, device=self.device)
        if colors:
            rgba = torch.empty((T, h, w), dtype=torch.int32, device=self.device)
            out["colors"] = rgba.view(torch.uint8).reshape(T, h, w, 4)
        if T == 0:
            return None, None, 0, out
        table = (L.TsdfView * T)()
        for i in range(T):
            e = table[i]
            e.depth = out["depth"][i].data_ptr()
            e.vertex = out["vertices"][i].data_ptr() if vertices else None
            e.normal = out["normals"][i].data_ptr() if normals else None
            e.rgba = rgba[i].data_ptr() if colors else None
            e.row_stride, e.w, e.h = w, w, h
            e.fu, e.fv, e.cu, e.cv = (float(x) for x in fk[i])
            e.c2w[:] = P[i, :3].reshape(12).astype(np.float32).tolist()
            e.near, e.far = float(near), float(far)
        table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(self.device)
        return table, table_d, T, out

    def raycast_table(self, tbl, step_voxels=1.0, min_weight=1.0):
        """one ray-cast launch of a view_table -> its maps"""
        table, table_d, T, out = tbl
        if not (step_voxels >= 0.25 and math.isfinite(step_voxels)):
            raise ValueError("raycast: step_voxels must be finite and >= 0.25, got %r" % (step_voxels,))
        if not min_weight > 0:
            raise ValueError("raycast: min_weight must be > 0, got %r" % (min_weight,))
        if T == 0:
            return out
        step = float(np.float32(np.float32(step_voxels) * np.float32(self.voxel_size)))
        self._raycast_launch(table, table_d, T, float(min_weight), step)
        self.raycasts += 1
        return out

    def _mesh_buffers(self, n, max_vertices, max_faces):
        """extract_raw's capacities for n voxels (the first guesses when None is given) and output buffers:
        -> (cap_v, cap_f, vertices fp32 [cap, 3], rgba int32 [cap], faces int32 [cap, 3], counts int32 [2] zeroed)"""
        cap_v = int(max_vertices) if max_vertices is not None else min(7 * n, max(4096, n // 4))
        cap_f = int(max_faces) if max_faces is not None else min(12 * n, 2 * cap_v)
        vertices = torch.empty((max(cap_v, 1), 3), dtype=torch.float32, device=self.device)
        rgba = torch.empty(max(cap_v, 1), dtype=torch.int32, device=self.device)
        faces = torch.empty((max(cap_f, 1), 3), dtype=torch.int32, device=self.device)
        counts = torch.zeros(2, dtype=torch.int32, device=self.device)
        return cap_v, cap_f, vertices, rgba, faces, counts

    def extract_mesh(self, min_weight=1.0, scale=1.0, transform=None, min_component_faces=0, keep_largest=None, simplify_cell=None,
                     smooth_iters=0, fill_holes=0):
        """The zero level as a welded mesh of the voxels seen with weight >= min_weight: dict(vertices fp32 [V, 3], colors uint8
        [V, 4], faces int32 [F, 3], bounds float32 numpy [2, 3]), the shape of mesh.scene_mesh; positions are transform (scale x).
        The counts are read once on the host; if the first guess of the capacities was too small the extraction runs once more with
        the reported sizes.  Vertices that no face uses are dropped (mesh.compact_vertices).
        min_component_faces > 0 or keep_largest = k: the floaters go (mesh.select_components, the rule of mesh.filter_components) --
        only the faces of connected components with at least that many faces, and among the k largest, are kept, before the vertices
        are compacted (once); the dict then also has components = dict(total, kept, faces_removed).  With the defaults nothing of
        that runs.
        simplify_cell = c (world units, before scale): the surface is simplified by vertex clustering (mesh.simplify) on the grid of
        cell c from the volume's origin, after the component filter -- clustering can join a floater to the surface -- and before
        the final compaction, which applies scale / transform; the result is mesh.simplify(extract_mesh(...), c, origin) and the
        dict also has simplify = dict(cell, clusters, faces_in, faces_collapsed, faces_duplicate, faces_invalid).  None: nothing
        of that runs.
        smooth_iters = n > 0: n rounds of Taubin's filter (mesh.smooth with its defaults: boundary vertices fixed) on the compacted,
        unscaled vertices -- after the component filter, because a floater must not be smoothed into the surface, and before
        simplify_cell; scale / transform are applied afterwards, by simplify or by one more compaction.  With scale = 1 and no
        transform the result is mesh.smooth(extract_mesh(...), n); the dict also has smooth = dict(iterations, lam, mu, boundary,
        fixed_vertices).  0: nothing of that runs.
        fill_holes = n >= 3: every boundary loop of at most n edges is closed (mesh.fill_holes: a fan about the mean of the loop, one
        face for a loop of 3) -- after the component filter and the first compaction, and before smooth_iters, so that the filter
        relaxes the fans (their centres are interior vertices: they move), and before simplify_cell; scale / transform are applied
        afterwards, as for smooth_iters.  The rim of what was observed is a long loop and stays open.  With scale = 1 and no transform
        the result is mesh.fill_holes(extract_mesh(...), n), then mesh.smooth, then mesh.simplify; the dict also has fill =
        dict(max_edges, loops, filled, vertices_added, faces_added, open).  0: nothing of that runs."""
        if not min_weight > 0:
            raise ValueError("extract_mesh: min_weight must be > 0, got %r" % (min_weight,))
        if simplify_cell is not None and not (simplify_cell > 0 and math.isfinite(simplify_cell)):
            raise ValueError("extract_mesh: simplify_cell must be positive and finite, got %r" % (simplify_cell,))
        if min_component_faces < 0 or (keep_largest is not None and keep_largest < 0):
            raise ValueError("extract_mesh: min_component_faces %r and keep_largest %r must be >= 0" % (min_component_faces, keep_largest))
        if smooth_iters < 0:
            raise ValueError("extract_mesh: smooth_iters must be >= 0, got %r" % (smooth_iters,))
        if fill_holes != 0 and fill_holes < 3:
            raise ValueError("extract_mesh: fill_holes must be 0 or >= 3 (the shortest loop), got %r" % (fill_holes,))
        vertices, rgba, faces, counts = self.extract_raw(min_weight)
        nv, nf = counts.cpu().tolist()
        if nv > vertices.shape[0] or nf > faces.shape[0]:
            vertices, rgba, faces, counts = self.extract_raw(min_weight, nv, nf)
            nv2, nf2 = counts.cpu().tolist()
            if (nv2, nf2) != (nv, nf):
                raise RuntimeError("extract_mesh: the volume changed between two extractions (%d, %d) -> (%d, %d)" % (nv, nf, nv2, nf2))
        faces = faces[:nf].contiguous()
        stats = None
        if min_component_faces > 0 or keep_largest is not None:
            faces, stats = M.select_components(faces, nv, min_component_faces, keep_largest)
        if simplify_cell is None and smooth_iters == 0 and fill_holes == 0:
            pos, col, bounds = M.compact_vertices(vertices[:nv].contiguous(), rgba[:nv].contiguous(), faces=faces, scale=scale, transform=transform)
        else:      # only the vertices the kept faces name enter a cluster or a row: compact first, unscaled, then fill, smooth, cluster, scale / transform
            pos, col, bounds = M.compact_vertices(vertices[:nv].contiguous(), rgba[:nv].contiguous(), faces=faces)
        if pos.shape[0] == 0:
            faces = faces[:0]
        out = dict(vertices=pos, colors=col.contiguous().view(torch.uint8).reshape(-1, 4), faces=faces, bounds=bounds)
        if fill_holes > 0:
            out = M.fill_holes(out, fill_holes)
        if smooth_iters > 0:
            out = M.smooth(out, smooth_iters)
        if simplify_cell is not None:
            out = M.simplify(out, simplify_cell, origin=self.origin, scale=scale, transform=transform)
        elif (smooth_iters > 0 or fill_holes > 0) and (scale != 1.0 or transform is not None) and out["vertices"].shape[0] > 0:
            # (every vertex is named by a face: this compaction keeps them all, in order, and only applies scale / transform)
            pos, col, out["bounds"] = M.compact_vertices(out["vertices"], out["colors"].view(torch.int32).reshape(-1), faces=out["faces"].clone(),
                                                         scale=scale, transform=transform)
            out["vertices"] = pos
        if stats is not None:
            out["components"] = stats
        return out


class TSDFVolume(_Volume):
    """A truncated signed distance volume on the device: tsdf fp32 [nz, ny, nx] (initial 1), weight (initial 0) and, with color,
    rgb fp32 [nz, ny, nx, 3] in [0, 1].  Voxel (i, j, k) has its centre at origin + (i, j, k) * voxel_size.  trunc defaults to
    3 voxels."""

    def __init__(self, origin, voxel_size, dims, trunc=None, color=True, device="cuda"):
        self.dims = _check_dims(dims)
        self._set_lattice(origin, voxel_size, trunc, device)
        nx, ny, nz = self.dims
        self.tsdf = torch.empty((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.weight = torch.empty((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.rgb = torch.empty((nz, ny, nx, 3), dtype=torch.float32, device=self.device) if color else None
        self.launches = 0                   # sp3_tsdf_integrate launches so far
        self.raycasts = 0                   # sp3_tsdf_raycast launches so far
        self.reset()

    def reset(self):
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        if self.rgb is not None:
            self.rgb.zero_()

    def integrate_table(self, tbl):
        """one sp3_tsdf_integrate launch of a frame_table"""
        table, table_d, T, _ = tbl
        lib, st = L.load(), L.stream_ptr()
        nx, ny, nz = self.dims
        L.check(lib.sp3_tsdf_integrate(table, table_d.data_ptr(), T, nx, ny, nz, self._origin_c, self.voxel_size, self.trunc,
                                       self.tsdf.data_ptr(), self.weight.data_ptr(), L.ptr(self.rgb), st), "sp3_tsdf_integrate")
        self.launches += 1
        return self

    def _raycast_launch(self, table, table_d, T, min_weight, step):
        nx, ny, nz = self.dims
        L.check(L.load().sp3_tsdf_raycast(table, table_d.data_ptr(), T, nx, ny, nz, self._origin_c, self.voxel_size, self.tsdf.data_ptr(),
                                          self.weight.data_ptr(), L.ptr(self.rgb), min_weight, step, L.stream_ptr()), "sp3_tsdf_raycast")

    def extract_raw(self, min_weight=1.0, max_vertices=None, max_faces=None):
        """sp3_tsdf_extract as it is: -> (vertices fp32 [cap, 3], rgba int32 [cap], faces int32 [cap, 3], counts int32 [2] on the
        device = the true V and F).  Nothing beyond the capacities is written; nothing synchronises."""
        nx, ny, nz = self.dims
        n = nx * ny * nz
        lib = L.load()
        cap_v, cap_f, vertices, rgba, faces, counts = self._mesh_buffers(n, max_vertices, max_faces)
        ws = torch.empty(max(int(lib.sp3_tsdf_extract_ws_bytes(nx, ny, nz)), 16), dtype=torch.uint8, device=self.device)
        L.check(lib.sp3_tsdf_extract(self.tsdf.data_ptr(), self.weight.data_ptr(), L.ptr(self.rgb), nx, ny, nz, self._origin_c, self.voxel_size,
                                     float(min_weight), ws.data_ptr(), cap_v, cap_f, vertices.data_ptr(), rgba.data_ptr(), faces.data_ptr(),
                                     counts.data_ptr(), L.stream_ptr()), "sp3_tsdf_extract")
        return vertices[:cap_v], rgba[:cap_v], faces[:cap_f], counts


class BrickTSDFVolume(_Volume):
    """The volume of TSDFVolume on two levels (include/spann3r_hip.h "Brick TSDF volume", csrc/bricks.hip): a virtual grid of `dims`
    voxels (rounded up to multiples of 8) whose 8 x 8 x 8 bricks are allocated where measurements land -- every brick within `band`
    (metric, default trunc, at most 8 voxels) of a measured point -- and a pool of `capacity` bricks that doubles when it runs out.
    Memory follows the surface, not the box, and the extent need not be known: give a generous box.  An allocated voxel holds the
    bits the dense volume gives it after the same frames; a brick born in a later call does not hold what earlier frames would have
    given it.  `integrate`, `frame_table`, `raycast`, `view_table`, `raycast_table` and `extract_raw` take and return what
    TSDFVolume's do; `track_frame` takes a brick volume as it is.  `extract_mesh(direct=True)` meshes the bricks themselves."""

    def __init__(self, origin, voxel_size, dims, trunc=None, band=None, color=True, capacity=4096, device="cuda"):
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or min(dims) < 0:
            raise ValueError("BrickTSDFVolume: dims %s must be three sizes (nx, ny, nz) >= 0" % (dims,))
        self.dims = tuple(-(-d // 8) * 8 for d in dims)
        self.bricks = tuple(d // 8 for d in self.dims)
        n_table = self.bricks[0] * self.bricks[1] * self.bricks[2]
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("BrickTSDFVolume: capacity must be >= 1, got %r" % (capacity,))
        if max(self.dims) >= 2 ** 20 or 2 * n_table + 256 >= 2 ** 31:
            raise ValueError("BrickTSDFVolume: dims %s over the index limit: %d bricks (bricks + capacity must stay below 2^31)" % (self.dims, n_table))
        self._set_lattice(origin, voxel_size, trunc, device)
        self.band = float(np.float32(self.trunc if band is None else band))
        if not (0 < self.band <= float(np.float32(8.0) * np.float32(self.voxel_size))):
            raise ValueError("BrickTSDFVolume: band %r must lie in (0, 8 voxels = %g]" % (self.band, 8 * self.voxel_size))
        self.color = bool(color)
        dev = self.device
        self.table = torch.empty(max(n_table, 1), dtype=torch.int32, device=dev)[:n_table]
        self.flags = torch.empty(max(n_table, 1), dtype=torch.uint8, device=dev)[:n_table]
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)
        self._counts = torch.zeros(2, dtype=torch.int32, device=dev)
        self._ws = torch.empty(max(int(L.load().sp3_tsdf_brick_alloc_ws_bytes(*self.dims)), 16), dtype=torch.uint8, device=dev)
        self._pool(min(capacity, max(n_table, 1)))          # (a grid has no use for more slots than bricks)
        self.launches = 0                   # sp3_tsdf_brick_integrate launches so far
        self.raycasts = 0                   # sp3_tsdf_brick_raycast launches so far
        self.grown = 0                      # times the pool doubled
        self.reset()

    def _pool(self, capacity):
        """a fresh pool of `capacity` slots (alloc initialises a slot when it hands it out)"""
        dev = self.device
        self.capacity = capacity
        self.slot_brick = torch.empty(capacity, dtype=torch.int32, device=dev)
        self.tsdf = torch.empty((capacity, 512), dtype=torch.float32, device=dev)
        self.weight = torch.empty((capacity, 512), dtype=torch.float32, device=dev)
        self.rgb = torch.empty((capacity, 512, 3), dtype=torch.float32, device=dev) if self.color else None
        self._mesh_ws = None                # extract_raw's scratch: sized for the pool, so it goes with it

    def reset(self):
        self.table.fill_(-1)
        self.flags.zero_()
        self.count.zero_()
        self.n_bricks = 0

    @property
    def memory_bytes(self):
        """bytes held on the device: table, flags, slot_brick, the pool and, once extract_raw has run, its scratch"""
        ts = [self.table, self.flags, self.slot_brick, self.tsdf, self.weight, self.count, self._counts, self._ws] + ([self.rgb] if self.color else [])
        ts += [self._mesh_ws] if self._mesh_ws is not None else []
        return sum(t.numel() * t.element_size() for t in ts)

    def frame_table(self, src, is_depth, intrinsics, cam2world, valid=None, weight=None, images=None, need_images=True):
        """the base's frame_table plus, as a fifth entry, the device fp32 [T, 12] camera-to-world matrices `mark` reads for depth frames"""
        tbl = super().frame_table(src, is_depth, intrinsics, cam2world, valid, weight, images, need_images)
        P = _host_mats(cam2world, tbl[2], (4, 4), "cam2world")
        c2w = torch.from_numpy(np.ascontiguousarray(P[:, :3, :].reshape(tbl[2], 12).astype(np.float32))).to(self.device)
        return tbl + (c2w,)

    def allocate(self, depth=None, pts=None, intrinsics=None, cam2world=None, valid=None, weight=None, images=None):
        """`mark` + `alloc` for T frames (the arguments of `integrate`; images are not needed): the bricks within `band` of their points
        exist afterwards.  One read of two int32 per alloc call."""
        if (depth is None) == (pts is None):
            raise ValueError("allocate: give depth or pts, exactly one")
        if intrinsics is None or cam2world is None:
            raise ValueError("allocate: intrinsics and cam2world are required")
        src = _frames_list(depth, "depth", ()) if depth is not None else _frames_list(pts, "pts", (3,))
        if len(src) == 0:
            return self
        return self.allocate_table(self.frame_table(src, depth is not None, intrinsics, cam2world, valid, weight, need_images=False))

    def allocate_table(self, tbl):
        table, table_d, T, _, c2w = tbl
        lib, st = L.load(), L.stream_ptr()
        nx, ny, nz = self.dims
        L.check(lib.sp3_tsdf_brick_mark(table, table_d.data_ptr(), c2w.data_ptr(), T, nx, ny, nz, self._origin_c, self.voxel_size, self.band,
                                        self.flags.data_ptr(), st), "sp3_tsdf_brick_mark")
        while True:
            L.check(lib.sp3_tsdf_brick_alloc(self.flags.data_ptr(), nx, ny, nz, self.table.data_ptr(), self.slot_brick.data_ptr(),
                                             self.count.data_ptr(), self.capacity, self.tsdf.data_ptr(), self.weight.data_ptr(), L.ptr(self.rgb),
                                             self._ws.data_ptr(), self._counts.data_ptr(), st), "sp3_tsdf_brick_alloc")
            count, need = self._counts.cpu().tolist()
            if need <= self.capacity:
                self.n_bricks = count
                return self
            old = (self.slot_brick, self.tsdf, self.weight, self.rgb)
            capacity = self.capacity
            while capacity < need:
                capacity *= 2
            self._pool(min(capacity, self.table.numel()))
            for new, o in zip((self.slot_brick, self.tsdf, self.weight, self.rgb), old):
                if o is not None:
                    new[:count].copy_(o[:count])
            self.grown += 1

    def integrate_table(self, tbl):
        """mark, alloc, then one sp3_tsdf_brick_integrate launch of a frame_table"""
        self.allocate_table(tbl)
        table, table_d, T, _, _ = tbl
        nx, ny, nz = self.dims
        L.check(L.load().sp3_tsdf_brick_integrate(table, table_d.data_ptr(), T, nx, ny, nz, self._origin_c, self.voxel_size, self.trunc,
                                                  self.slot_brick.data_ptr(), self.n_bricks, self.tsdf.data_ptr(), self.weight.data_ptr(),
                                                  L.ptr(self.rgb), L.stream_ptr()), "sp3_tsdf_brick_integrate")
        self.launches += 1
        return self

    def _raycast_launch(self, table, table_d, T, min_weight, step):
        nx, ny, nz = self.dims
        L.check(L.load().sp3_tsdf_brick_raycast(table, table_d.data_ptr(), T, nx, ny, nz, self._origin_c, self.voxel_size, self.table.data_ptr(),
                                                self.tsdf.data_ptr(), self.weight.data_ptr(), L.ptr(self.rgb), min_weight, step,
                                                L.stream_ptr()), "sp3_tsdf_brick_raycast")

    def brick_box(self):
        """(lo, size) in voxels of the bounding box of the allocated bricks; size 0 without any"""
        if self.n_bricks == 0:
            return (0, 0, 0), (0, 0, 0)
        b = self.slot_brick[:self.n_bricks].cpu().numpy().astype(np.int64)
        bx, by, _ = self.bricks
        ijk = np.stack([b % bx, (b // bx) % by, b // (bx * by)], 1)
        lo, hi = ijk.min(0), ijk.max(0) + 1
        return tuple(int(x) * 8 for x in lo), tuple(int(x) * 8 for x in hi - lo)

    def to_dense(self, box=None, dims_limit=512):
        """The densified volume of a box of voxels, box = (lo, size) (default: the bounding box of the allocated bricks), as a TSDFVolume:
        allocated voxels copied, absent ones (1, 0, 0).  Its origin is origin + fp32(lo) * voxel_size, rounded per axis, and it
        places its voxels from there by its own rule.  More than dims_limit voxels on an axis raises ValueError."""
        lo, size = self.brick_box() if box is None else (tuple(int(x) for x in box[0]), tuple(int(x) for x in box[1]))
        if len(lo) != 3 or len(size) != 3 or min(lo) < 0 or min(size) < 0 or any(l + s > d for l, s, d in zip(lo, size, self.dims)):
            raise ValueError("to_dense: box (lo %s, size %s) must lie inside the grid of %s voxels" % (lo, size, self.dims))
        if max(size) > dims_limit:
            raise ValueError("to_dense: a box of %s voxels is over dims_limit %d per axis" % (size, dims_limit))
        origin = self.origin + np.asarray(lo, np.float32) * np.float32(self.voxel_size)
        out = TSDFVolume(origin, self.voxel_size, size, trunc=self.trunc, color=self.color, device=self.device)
        nx, ny, nz = self.dims
        L.check(L.load().sp3_tsdf_brick_to_dense(nx, ny, nz, self.table.data_ptr(), self.tsdf.data_ptr(), self.weight.data_ptr(), L.ptr(self.rgb),
                                                 (C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*size), out.tsdf.data_ptr(), out.weight.data_ptr(),
                                                 L.ptr(out.rgb), L.stream_ptr()), "sp3_tsdf_brick_to_dense")
        return out

    def extract_raw(self, min_weight=1.0, max_vertices=None, max_faces=None):
        """sp3_tsdf_brick_extract as it is, on the bricks themselves: -> the tuple of TSDFVolume.extract_raw (vertices fp32 [cap, 3],
        rgba int32 [cap], faces int32 [cap, 3], counts int32 [2] on the device = the true V and F), in pool-slot order, positions by
        the virtual grid's own origin.  The first guesses of the capacities are TSDFVolume's with n = 512 * n_bricks.  The scratch
        (5 bytes per allocated voxel) is kept on the volume and regrown with the pool.  Nothing beyond the capacities is written;
        nothing synchronises."""
        if self.n_bricks > BRICK_MESH_LIMIT:
            raise ValueError("extract_raw: %d bricks over the index limit: 12 * 512 * n_bricks must stay below 2^31 (int32 vertex and face "
                             "indices), at most %d bricks" % (self.n_bricks, BRICK_MESH_LIMIT))
        lib = L.load()
        cap_v, cap_f, vertices, rgba, faces, counts = self._mesh_buffers(512 * self.n_bricks, max_vertices, max_faces)
        if self._mesh_ws is None:
            self._mesh_ws = torch.empty(max(int(lib.sp3_tsdf_brick_extract_ws_bytes(min(self.capacity, BRICK_MESH_LIMIT))), 16), dtype=torch.uint8,
                                        device=self.device)
        nx, ny, nz = self.dims
        L.check(lib.sp3_tsdf_brick_extract(nx, ny, nz, self._origin_c, self.voxel_size, self.table.data_ptr(), self.slot_brick.data_ptr(),
                                           self.n_bricks, self.tsdf.data_ptr(), self.weight.data_ptr(), L.ptr(self.rgb), float(min_weight),
                                           self._mesh_ws.data_ptr(), cap_v, cap_f, vertices.data_ptr(), rgba.data_ptr(), faces.data_ptr(),
                                           counts.data_ptr(), L.stream_ptr()), "sp3_tsdf_brick_extract")
        return vertices[:cap_v], rgba[:cap_v], faces[:cap_f], counts

    def extract_mesh(self, min_weight=1.0, scale=1.0, transform=None, dims_limit=512, direct=False, min_component_faces=0,
                     keep_largest=None, simplify_cell=None, smooth_iters=0, fill_holes=0):
        """direct=False: to_dense().extract_mesh(...), the surface of the allocated bricks' bounding box through the dense kernel (a box
        of more than dims_limit voxels on an axis raises).  direct=True: marching tetrahedra on the bricks themselves
        (sp3_tsdf_brick_extract) -- no dense intermediate, no limit on the extent, dims_limit ignored; the same surface as a set of
        triangles, its vertices and faces in pool-slot order and its positions from the virtual grid's own origin (the dense route
        places them from the box's).  Capacities, the one retry, min_component_faces / keep_largest, simplify_cell, smooth_iters, fill_holes and
        the dict are TSDFVolume.extract_mesh's, on both routes (the dense route clusters on the grid from the box's origin)."""
        if not direct:
            return self.to_dense(dims_limit=dims_limit).extract_mesh(min_weight, scale, transform, min_component_faces, keep_largest, simplify_cell,
                                                                     smooth_iters, fill_holes)
        return super().extract_mesh(min_weight, scale, transform, min_component_faces, keep_largest, simplify_cell, smooth_iters, fill_holes)


def _extent_box(extent):
    box = np.asarray([np.asarray(e, np.float64).reshape(-1) for e in extent], np.float64)
    if box.shape != (2, 3) or not np.isfinite(box).all() or not (box[1] >= box[0]).all():
        raise ValueError("extent must be (lo, hi): two finite points with lo <= hi, got %r" % (extent,))
    return box


def brick_volume_for_extent(extent, voxel_size, trunc_voxels=3.0, color=True, capacity=4096, device="cuda"):
    """The BrickTSDFVolume whose virtual grid covers the box extent = (lo, hi) padded by trunc = trunc_voxels voxels (the padding
    rule of volume_for_points)."""
    box = _extent_box(extent)
    if voxel_size is None or not (voxel_size > 0 and math.isfinite(voxel_size)):
        raise ValueError("a brick volume needs voxel_size (positive, finite), got %r" % (voxel_size,))
    pad = math.ceil(trunc_voxels) * voxel_size
    dims = tuple(int(math.ceil((e + 2 * pad) / voxel_size - 1e-9)) + 1 for e in box[1] - box[0])
    return BrickTSDFVolume(box[0] - pad, voxel_size, dims, trunc=trunc_voxels * voxel_size, color=color, capacity=capacity, device=device)


def volume_for_points(points, voxel_size=None, dims_max=256, trunc_voxels=3.0, color=True):
    """The volume whose box is that of `points` (device fp32 [n, 3], all finite) padded by trunc = trunc_voxels voxels.  voxel_size
    None: the largest voxel with which the longest side fits dims_max voxels."""
    pts = _dev(points, "volume_for_points: points").reshape(-1, 3).float()
    if pts.shape[0] == 0:
        raise RuntimeError("volume_for_points: no point to fit a volume to")
    box = torch.stack([pts.amin(0), pts.amax(0)]).double().cpu().numpy()
    if not np.isfinite(box).all():
        raise RuntimeError("volume_for_points: non-finite point")
    extent = box[1] - box[0]
    if dims_max < 2 * trunc_voxels + 2:
        raise ValueError("volume_for_points: dims_max %d leaves no room inside a padding of %g voxels" % (dims_max, trunc_voxels))
    if voxel_size is None:
        voxel_size = max(float(extent.max()), 1e-6) / (dims_max - 1 - 2 * math.ceil(trunc_voxels))
    trunc = trunc_voxels * voxel_size
    pad = math.ceil(trunc_voxels) * voxel_size
    dims = tuple(int(math.ceil((e + 2 * pad) / voxel_size - 1e-9)) + 1 for e in extent)
    if max(dims) > dims_max:
        raise ValueError("volume_for_points: voxel_size %g needs %s voxels, over dims_max %d" % (voxel_size, dims, dims_max))
    return TSDFVolume(box[0] - pad, voxel_size, dims, trunc=trunc, color=color, device=pts.device)


def _expm_se3(xi):
    """(omega, delta) of y' = y + omega x y + delta -> the rigid 4 x 4 [exp(omega) | delta], the update of estimate_poses"""
    from .postprocess import _expm_so3
    U = np.eye(4)
    U[:3, :3], U[:3, 3] = _expm_so3(xi[:3]), xi[3:]
    return U


def _rt12(M):
    """4 x 4 -> the 12 doubles row-major R (9) | t (3) of sp3_pnp_gn_accum's pose"""
    return np.concatenate([M[:3, :3].reshape(9), M[:3, 3]])


def track_frame(vol, pts, valid, intrinsics, cam2world, iterations=10, recasts=2, dist_max=None, min_pairs=64, step_voxels=1.0,
                min_weight=1.0, relative_rmse=1e-6, timings=None):
    """The KinectFusion registration of one frame against the model in `vol`, which must not contain the frame yet: pts fp32 [h, w, 3]
    (the frame's world points), valid [h, w] (nullable), intrinsics [3, 3], cam2world [4, 4] as the frame claims them.
    -> (T float64 [4, 4], info): the rigid correction to apply on the left of the points and of the pose.
    `recasts` times: the volume is ray-cast from the currently corrected pose (one launch), then up to `iterations` Gauss-Newton
    steps of projective point-to-plane registration run against those maps: one sp3_tsdf_track_accum launch and one read of 29
    doubles each, the 6 x 6 system solved on the host in float64 (lstsq), T <- exp(xi) T.  A recast stops early when the rmse changes
    by less than relative_rmse (icp_point_to_point's rule).  dist_max defaults to vol.trunc.  A frame is not tracked when fewer than
    min_pairs pairs are found or a non-finite or rank-deficient system appears (a singular value of H below 1e-9 of the largest):
    T is then the identity and info["tracked"] False; nothing raises.  info: tracked, pairs, rmse, iterations.
    timings (a dict, optional) accumulates the host seconds spent in `raycast`, `accumulate` (launch and read-back) and `solve`, and
    the number of `round_trips` (one per Gauss-Newton step)."""
    import time
    pts = _dev(pts, "track_frame: pts").float().contiguous()
    if pts.dim() != 3 or pts.shape[-1] != 3:
        raise RuntimeError("track_frame: pts %s must be [h, w, 3]" % (tuple(pts.shape),))
    h, w = pts.shape[:2]
    n = h * w
    v = None
    if valid is not None:
        v = _dev(valid, "track_frame: valid").to(torch.uint8).contiguous()
        if tuple(v.shape) != (h, w):
            raise RuntimeError("track_frame: mismatched shapes: pts %s, valid %s" % (tuple(pts.shape), tuple(v.shape)))
    P0 = _host_mats(cam2world, 1, (4, 4), "cam2world")[0]
    fk, _ = camera_tables(intrinsics, P0[None], 1)
    K = _host_mats(intrinsics, 1, (3, 3), "intrinsics")[0]
    dist_max = vol.trunc if dist_max is None else float(dist_max)
    lib, dev = L.load(), vol.device
    ws = torch.empty(max(int(lib.sp3_tsdf_track_accum_ws_bytes(n)), 16), dtype=torch.uint8, device=dev)
    out_d = torch.empty(29, dtype=torch.float64, device=dev)
    fu, fv, cu, cv = (float(np.float32(x)) for x in fk[0])
    T = np.eye(4)
    info = dict(tracked=False, pairs=0, rmse=float("nan"), iterations=0)
    clock = (lambda: time.perf_counter()) if timings is not None else (lambda: 0.0)

    def spent(key, t0):
        if timings is not None:
            timings[key] = timings.get(key, 0.0) + clock() - t0

    for _ in range(int(recasts)):
        t0 = clock()
        P = T @ P0
        model = vol.raycast(K, P[None], (h, w), step_voxels=step_voxels, min_weight=min_weight, colors=False)
        w2c_d = torch.from_numpy(_rt12(np.linalg.inv(P))).to(dev)
        spent("raycast", t0)
        last = None
        for _ in range(int(iterations)):
            t0 = clock()
            T_d = torch.from_numpy(_rt12(T)).to(dev)
            L.check(lib.sp3_tsdf_track_accum(pts.data_ptr(), L.ptr(v), n, T_d.data_ptr(), model["vertices"].data_ptr(),
                                             model["normals"].data_ptr(), model["depth"].data_ptr(), w, h, w, fu, fv, cu, cv, w2c_d.data_ptr(),
                                             dist_max, ws.data_ptr(), out_d.data_ptr(), L.stream_ptr()), "sp3_tsdf_track_accum")
            out = out_d.cpu().numpy()
            spent("accumulate", t0)
            if timings is not None:
                timings["round_trips"] = timings.get("round_trips", 0) + 1
            t0 = clock()
            info["iterations"] += 1
            info["pairs"] = int(out[28]) if math.isfinite(out[28]) else 0
            if not out[28] >= min_pairs:
                return np.eye(4), info
            rmse = math.sqrt(out[27] / out[28]) if out[27] >= 0 else float("nan")
            info["rmse"] = rmse
            if last is not None and abs(rmse - last) < relative_rmse:
                spent("solve", t0)
                break
            last = rmse
            H = np.zeros((6, 6))
            H[np.triu_indices(6)] = out[:21]
            H = H + np.triu(H, 1).T
            g = out[21:27]
            if not (np.isfinite(H).all() and np.isfinite(g).all()):
                return np.eye(4), info
            sv = np.linalg.svd(H, compute_uv=False)
            if not (sv[0] > 0 and sv[-1] >= 1e-9 * sv[0]):
                return np.eye(4), info
            T = _expm_se3(np.linalg.lstsq(H, -g, rcond=None)[0]) @ T
            spent("solve", t0)
    info["tracked"] = True
    return T, info


def _transform_points(pts, T):
    """T [4, 4] float64 applied to device points fp32 [..., 3] (sp3_transform_points: fp64, rounded to fp32)"""
    src = pts.float().contiguous()
    out = torch.empty_like(src)
    n = src.numel() // 3
    if n:
        L.check(L.load().sp3_transform_points(src.data_ptr(), n, (C.c_double * 12)(*_rt12(T).tolist()), out.data_ptr(), L.stream_ptr()),
                "sp3_transform_points")
    return out


def _fuse_frame(vol, pts, valid, K, pose, image, track, track_args=None):
    """One step of the KinectFusion sequence on `vol` (dense or bricks): with `track` the frame -- pts [h, w, 3] world points, valid
    [h, w], K [3, 3], pose = its claimed cam2world [4, 4], image [h, w, 3] or None -- is registered to the model that does not contain
    it yet (track_frame), its pointmap moved by the correction T (sp3_transform_points) and its pose set to T @ pose; then it is
    integrated in one launch.  -> (the pose used, T, track_frame's info or None)."""
    T, info = np.eye(4), None
    if track:
        Tt, info = track_frame(vol, pts, valid, K, pose, **(track_args or {}))
        if info["tracked"]:
            T, pose = Tt, Tt @ pose
            pts = _transform_points(pts, T)
    vol.integrate(pts=pts[None], intrinsics=K, cam2world=pose[None], valid=valid[None], images=None if image is None else image[None])
    return pose, T, info


class FusionSession:
    """Fusion one frame at a time, with no knowledge of the frames to come: a BrickTSDFVolume of voxel_size inside the generous box
    extent = (lo, hi).  push() runs the step of fuse_pointmaps(track=True, bricks=True) -- the same function -- so a session over the
    frames of a sequence ends in the state that call ends in."""

    def __init__(self, voxel_size, extent, trunc_voxels=3.0, color=True, track=True, track_args=None, capacity=4096, device="cuda"):
        self.volume = brick_volume_for_extent(extent, voxel_size, trunc_voxels, color, capacity, device)
        self.track, self.track_args = bool(track), track_args
        self.frames = 0
        self.poses, self.corrections, self.tracked = [], [], []

    def push(self, pts, intrinsics, cam2world, valid, image=None):
        """pts fp32 [h, w, 3] (world points), intrinsics [3, 3], cam2world [4, 4] as the frame claims it, valid [h, w], image [h, w, 3]
        in [0, 1] (required when the session has colours).  -> (the cam2world used, info): info is track_frame's from the second frame
        on (tracked False: the pose was used as claimed), dict(tracked=...) for the first frame and without tracking."""
        pts = _dev(pts, "push: pts").float()
        if pts.dim() != 3 or pts.shape[-1] != 3 or _dev(valid, "push: valid").shape != pts.shape[:2]:
            raise RuntimeError("push: mismatched shapes: pts %s must be [h, w, 3], valid %s [h, w]" % (tuple(pts.shape), tuple(valid.shape)))
        if self.volume.color and image is None:
            raise ValueError("push: the session has colours: pass image (or build it with color=False)")
        valid = valid.bool() & torch.isfinite(pts).all(-1)
        K = _host_mats(intrinsics, 1, (3, 3), "intrinsics")[0]
        pose = _host_mats(cam2world, 1, (4, 4), "cam2world")[0].copy()
        first = self.frames == 0
        pose, T, info = _fuse_frame(self.volume, pts, valid, K, pose, image if self.volume.color else None, self.track and not first,
                                    self.track_args)
        if info is None:
            info = dict(tracked=bool(self.track and first))        # (frame 0 is the model's own frame)
        self.frames += 1
        self.poses.append(pose)
        self.corrections.append(T)
        self.tracked.append(bool(info["tracked"]))
        return pose, info

    def raycast(self, intrinsics, cam2world, size, **kw):
        """BrickTSDFVolume.raycast of the model so far"""
        return self.volume.raycast(intrinsics, cam2world, size, **kw)

    def mesh(self, min_weight=1.0, scale=1.0, transform=None, dims_limit=512, direct=False, min_component_faces=0, keep_largest=None,
             simplify_cell=None, smooth_iters=0, fill_holes=0):
        """BrickTSDFVolume.extract_mesh of the model so far (direct=True: meshed on the bricks, whatever the extent;
        min_component_faces / keep_largest: without its floaters; simplify_cell: simplified by vertex clustering; smooth_iters:
        smoothed by that many rounds of Taubin's filter before that; fill_holes: its boundary loops of at most that many edges closed
        before that)"""
        return self.volume.extract_mesh(min_weight, scale, transform, dims_limit, direct, min_component_faces, keep_largest, simplify_cell,
                                        smooth_iters, fill_holes)


def fuse_sequence(preds, batch, conf_thresh=1e-3, voxel_size=None, dims_max=256, trunc_voxels=3.0, min_weight=1.0, scale=1.0,
                  transform=None, color=True, return_volume=False, focal=None, poses=None, track=False, return_poses=False, bricks=False,
                  extent=None, direct_mesh=False, min_component_faces=0, keep_largest=None, simplify_cell=None, smooth_iters=0,
                  fill_holes=0, clean_tol=None, clean_order="sequence"):
    """The fused surface of a reconstruction from model.forward's `preds` and its `batch`: demo.py's own sequence -- the stacked
    pointmaps (mesh.sequence_tensors), the focal of frame 0 (estimate_focal_knowing_depth), one pose per frame (estimate_poses) --
    then the pointmaps of the pixels with (conf - 1) / conf > conf_thresh integrated through the `pts` path into a volume around
    the confident points.  -> the mesh dict of TSDFVolume.extract_mesh (and the volume with return_volume).
    focal / poses (cam2world [t, 4, 4]) given: used instead of the estimates.  track / return_poses: as fuse_pointmaps (every frame
    after the first is registered to the model before it is integrated).  bricks / extent / direct_mesh: as fuse_pointmaps (a
    BrickTSDFVolume at voxel_size instead of the dense volume).  min_component_faces / keep_largest: as TSDFVolume.extract_mesh (the
    floaters of the surface are dropped).  simplify_cell, smooth_iters, fill_holes: as TSDFVolume.extract_mesh.  clean_tol = t: the confidences are cleaned across the frames first
    (multiview.clean_confidence with tol t and clean_order, through the same focal and poses), so a pixel that floats in front of what a
    more confident frame measured does not pass conf_thresh; None: nothing of that runs.  Pointmaps without geometry (seeded random weights)
    give a focal near 0: that raises rather than fusing through meaningless cameras."""
    from .postprocess import estimate_focal_knowing_depth, estimate_poses
    pts_all, images_all, conf_all = M.sequence_tensors(preds, batch)
    _dev(pts_all, "fuse_sequence: pts3d")
    t, h, w, _ = pts_all.shape
    pp = (w / 2, h / 2)
    if focal is None:
        focal = float(estimate_focal_knowing_depth(pts_all[:1], torch.tensor(pp), focal_mode="weiszfeld").item())
        if not (focal > 1e-3 and math.isfinite(focal)):
            raise RuntimeError("fuse_sequence: degenerate pointmaps: the focal of the first frame came out as %g" % focal)
    focal = float(focal)
    if not (focal > 0 and math.isfinite(focal)):
        raise ValueError("fuse_sequence: focal must be positive and finite, got %r" % focal)
    if poses is None:
        poses, _ = estimate_poses(pts_all, focal, pp)
    K = np.array([[focal, 0, pp[0]], [0, focal, pp[1]], [0, 0, 1]], np.float64)
    if clean_tol is not None:
        from .multiview import clean_confidence
        conf_all = clean_confidence(pts_all, conf_all, K, np.asarray(poses, np.float64), tol=clean_tol, order=clean_order)
    valid = (conf_all - 1) / conf_all > conf_thresh
    return fuse_pointmaps(pts_all, K, np.asarray(poses, np.float64), valid, images_all, voxel_size, dims_max, trunc_voxels, min_weight, scale,
                          transform, color, return_volume, track, return_poses, bricks=bricks, extent=extent, direct_mesh=direct_mesh,
                          min_component_faces=min_component_faces, keep_largest=keep_largest, simplify_cell=simplify_cell,
                          smooth_iters=smooth_iters, fill_holes=fill_holes)


def fuse_pointmaps(pts_all, intrinsics, cam2world, valid, images=None, voxel_size=None, dims_max=256, trunc_voxels=3.0, min_weight=1.0,
                   scale=1.0, transform=None, color=True, return_volume=False, track=False, return_poses=False, track_args=None,
                   bricks=False, extent=None, direct_mesh=False, min_component_faces=0, keep_largest=None, simplify_cell=None, smooth_iters=0,
                   fill_holes=0):
    """World pointmaps pts_all [t, h, w, 3] with their cameras, integrated through the `pts` path into a volume around the valid
    (and finite) points -> the mesh dict of TSDFVolume.extract_mesh (and the volume with return_volume).
    track=False: one integrate launch for all frames.  track=True: the KinectFusion sequence -- frame 0 is integrated; every later
    frame is registered to the model that does not contain it yet (track_frame, keywords from track_args), its pointmap moved by the
    correction T (sp3_transform_points), its pose set to T @ pose, and only then integrated: one launch per frame.  The volume is
    still fitted to the points as predicted; the trunc padding absorbs the corrections.  return_poses adds to the mesh dict `poses`
    (the cam2world used, float64 [t, 4, 4]), `corrections` (the T of every frame) and `tracked` (a list of bool: frame 0, the model's own
    frame, counts as tracked; all False without track).
    bricks=True: the volume is a BrickTSDFVolume at voxel_size (required then) over the box of the valid points, or over
    extent = (lo, hi) when given -- the points are then not consulted at all, which is what a stream needs; the mesh comes from
    to_dense() of the allocated bricks' bounding box, which may have max(512, dims_max) voxels per axis, or with direct_mesh=True
    from the bricks themselves (BrickTSDFVolume.extract_mesh(direct=True): no such limit).
    min_component_faces / keep_largest / simplify_cell / smooth_iters / fill_holes: as TSDFVolume.extract_mesh, whichever volume and
    route."""
    pts_all = _dev(pts_all, "fuse_pointmaps: pts_all").float()
    if pts_all.dim() != 4 or pts_all.shape[-1] != 3 or _dev(valid, "fuse_pointmaps: valid").shape != pts_all.shape[:3]:
        raise RuntimeError("fuse_pointmaps: mismatched shapes: pts_all %s must be [t, h, w, 3], valid %s [t, h, w]" %
                           (tuple(pts_all.shape), tuple(valid.shape)))
    valid = valid.bool() & torch.isfinite(pts_all).all(-1)
    if extent is not None and not bricks:
        raise ValueError("fuse_pointmaps: extent is for bricks=True (the dense volume is fitted to the points)")
    if direct_mesh and not bricks:
        raise ValueError("fuse_pointmaps: direct_mesh is for bricks=True (the dense volume has one extraction)")
    if bricks and voxel_size is None:
        raise ValueError("fuse_pointmaps: bricks=True needs voxel_size")
    if extent is None and not bool(valid.any()):
        raise RuntimeError("fuse_pointmaps: no valid point (nothing passes the confidence threshold)")
    color = color and images is not None
    if not bricks:
        vol = volume_for_points(pts_all[valid], voxel_size, dims_max, trunc_voxels, color)
    else:
        if extent is None:
            sel = pts_all[valid]
            extent = torch.stack([sel.amin(0), sel.amax(0)]).double().cpu().numpy()
        vol = brick_volume_for_extent(extent, voxel_size, trunc_voxels, color, device=pts_all.device)
    t = pts_all.shape[0]
    poses = _host_mats(cam2world, t, (4, 4), "cam2world").copy()
    corrections, tracked = np.stack([np.eye(4)] * t), [bool(track)] + [False] * (t - 1)      # (frame 0 is the model's own frame)
    if not track:
        vol.integrate(pts=pts_all, intrinsics=intrinsics, cam2world=cam2world, valid=valid, images=images if color else None)
    else:
        K = _host_mats(intrinsics, t, (3, 3), "intrinsics")
        for i in range(t):
            poses[i], T, info = _fuse_frame(vol, pts_all[i], valid[i], K[i], poses[i], images[i] if color else None, i > 0, track_args)
            if i > 0:
                tracked[i] = bool(info["tracked"])
                if tracked[i]:
                    corrections[i] = T
    if bricks:
        out = vol.extract_mesh(min_weight, scale, transform, dims_limit=max(512, dims_max), direct=direct_mesh,
                               min_component_faces=min_component_faces, keep_largest=keep_largest, simplify_cell=simplify_cell,
                               smooth_iters=smooth_iters, fill_holes=fill_holes)
    else:
        out = vol.extract_mesh(min_weight, scale, transform, min_component_faces, keep_largest, simplify_cell, smooth_iters, fill_holes)
    if return_poses:
        out.update(poses=poses, corrections=corrections, tracked=tracked)
    return (out, vol) if return_volume else out


def fuse_views(views, voxel_size=None, dims_max=256, trunc_voxels=3.0, min_weight=1.0, scale=1.0, transform=None, color=True,
               return_volume=False, min_component_faces=0, keep_largest=None, simplify_cell=None, smooth_iters=0, fill_holes=0):
    """The ground-truth surface of an RGB-D sequence: the views of views.build_views integrated through `depthmap`,
    `camera_intrinsics`, `camera_pose` and `valid_mask` into a volume around their valid `pts3d`.  -> as fuse_sequence
    (min_component_faces / keep_largest / simplify_cell / smooth_iters / fill_holes: as TSDFVolume.extract_mesh).
    Landscape views only: a portrait view rectified to landscape carries row-permuted intrinsics, which are refused as skewed."""
    if len(views) == 0:
        raise ValueError("fuse_views: no views")
    depth = torch.cat([_dev(v["depthmap"], "fuse_views: depthmap") for v in views]).float()
    valid = torch.cat([v["valid_mask"] for v in views])
    pts = torch.cat([v["pts3d"] for v in views]).float()
    if depth.dim() != 3 or valid.shape != depth.shape or pts.shape != depth.shape + (3,):
        raise RuntimeError("fuse_views: mismatched shapes: depthmap %s, valid_mask %s, pts3d %s" % (tuple(depth.shape), tuple(valid.shape), tuple(pts.shape)))
    if not bool(valid.any()):
        raise RuntimeError("fuse_views: no valid pixel")
    K = torch.cat([v["camera_intrinsics"] for v in views]).double().cpu().numpy()
    poses = torch.cat([v["camera_pose"] for v in views]).double().cpu().numpy()
    images = None
    if color:
        images = (torch.cat([v["img"] for v in views]).to(depth.device).permute(0, 2, 3, 1).float() + 1.0) / 2.0
        if images.shape[1:3] != depth.shape[1:3]:
            raise RuntimeError("fuse_views: img %s does not match depthmap %s" % (tuple(images.shape), tuple(depth.shape)))
    vol = volume_for_points(pts[valid], voxel_size, dims_max, trunc_voxels, color)
    vol.integrate(depth=depth, intrinsics=K, cam2world=poses, valid=valid, images=images)
    out = vol.extract_mesh(min_weight, scale, transform, min_component_faces, keep_largest, simplify_cell, smooth_iters, fill_holes)
    return (out, vol) if return_volume else out
