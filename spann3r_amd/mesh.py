"""Pointmap meshes and GLB export on the device (reference: app.py:38-47 cat_meshes, :68-105 pts3d_to_trimesh, :132-171 of reconstruct).

The reference masks the predictions by confidence, turns every frame's pointmap into a triangle mesh on the host (two triangles per
pixel cell, each in both windings, filtered with a fancy-indexed `valid[faces].all(-1)`), concatenates the frames and exports one
GLB through trimesh.  Here the face list, the compaction of the vertices that survive and the x10 / transform of the positions are
HIP kernels (csrc/mesh.hip: order-preserving scans, three launches each); the host reads the counts once, copies the compacted
arrays and writes the file with struct / json.

What this restates and what it does not:
- `pts3d_to_mesh` / `cat_meshes` give the reference's vertices, faces and face_colors bit for bit, order and dtypes included
  (tests/golden/mesh_faces.npz is the reference's own output).
- `write_glb` writes vertex colours (each pixel's own colour): glTF has no face colours.  What trimesh makes of `face_colors` on
  export, how it merges or orders vertices and how it rounds float colours cannot be checked here: parity unpinned vs trimesh.
  Instead of the reference's duplicated reversed faces the material is `doubleSided`, which halves the index buffer.
- `scene_mesh` also drops pixels whose point is not finite; the reference would export them.
torch provides memory and the gather behind `face_colors`; trimesh, gradio and the ffmpeg frame extraction of app.py are not covered."""
import ctypes as C
import json
import math
import struct

import numpy as np
import torch

from . import cell_grid as G
from . import lib as L

SCALE = 10.0                                      # app.py:143
TRANSFORM = np.diag([-1.0, -1.0, 1.0, 1.0])       # app.py:165-167: inv(OPENGL @ rot_y(180 deg)) = inv(diag(1,-1,-1,1) diag(-1,1,-1,1))


def _dev(x, name):
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s: expected a CUDA tensor, got %s" % (name, type(x).__name__))
    if not x.is_cuda:
        raise RuntimeError("%s: meshes are built on the GPU (HIP kernels); there is no CPU path -- pass a CUDA tensor" % name)
    return x


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def build_faces(t, h, w, device, valid=None, conf=None, conf_thresh=0.0, pts=None, both_windings=True, sync=True):
    """sp3_mesh_faces: -> (faces int32 [F, 3], colour_px int32 [F], counts).  valid uint8 / bool [t, h, w] or conf fp32 [t, h, w] with
    conf_thresh; pts fp32 [t, h, w, 3] adds the finiteness test.  With sync=True the host reads the counts once and the tensors are
    cut to F (counts: a list, [F] + per frame and block); with sync=False they keep their full capacity and counts stays on the device."""
    n = t * h * w
    for name, x, dt in (("valid", valid, torch.uint8), ("conf", conf, torch.float32), ("pts", pts, torch.float32)):
        if x is not None and (x.dtype != dt or not x.is_contiguous() or x.numel() != n * (3 if name == "pts" else 1)):
            raise RuntimeError("build_faces: %s must be a contiguous %s tensor of %d x %d x %d pixels" % (name, dt, t, h, w))
    lib = L.load()
    nblk = 4 if both_windings else 2
    cap = max(t * nblk * (h - 1) * (w - 1), 1)
    faces = torch.empty((cap, 3), dtype=torch.int32, device=device)
    colour_px = torch.empty(cap, dtype=torch.int32, device=device)
    counts = torch.zeros(1 + nblk * t, dtype=torch.int32, device=device)
    ws = _ws(lib.sp3_mesh_faces_ws_bytes(t, h, w), device)
    L.check(lib.sp3_mesh_faces(L.ptr(valid), L.ptr(conf), float(conf_thresh), L.ptr(pts), t, h, w, int(both_windings), ws.data_ptr(),
                               faces.data_ptr(), colour_px.data_ptr(), counts.data_ptr(), L.stream_ptr()), "sp3_mesh_faces")
    if not sync:
        return faces, colour_px, counts
    counts = counts.cpu().tolist()
    return faces[:counts[0]], colour_px[:counts[0]], counts


def compact_vertices(pts, rgba=None, faces=None, valid=None, conf=None, conf_thresh=0.0, scale=1.0, transform=None):
    """sp3_mesh_compact_vertices: pts fp32 [n, 3], rgba int32 [n] (optional), and either faces int32 [F, 3] (rewritten in place) or
    valid / conf for a cloud -> (positions fp32 [V, 3], rgba int32 [V] or None, bounds float32 numpy [2, 3]).  One host read."""
    n = pts.shape[0]
    lib = L.load()
    if n == 0 or (faces is not None and faces.shape[0] == 0):          # nothing to keep (and an empty tensor has no pointer to pass)
        none = np.array([[np.inf] * 3, [-np.inf] * 3], np.float32)
        return pts.new_empty((0, 3)), None if rgba is None else rgba[:0], none
    out_pos = torch.empty((n, 3), dtype=torch.float32, device=pts.device)
    out_rgba = torch.empty(n, dtype=torch.int32, device=pts.device) if rgba is not None else None
    info = torch.zeros(8, dtype=torch.float32, device=pts.device)      # [0]: V (int32 bits), [2..8): min / max
    info[2:5] = float("inf")
    info[5:8] = float("-inf")
    ws = _ws(lib.sp3_mesh_vertices_ws_bytes(n), pts.device)
    m = None if transform is None else (C.c_float * 16)(*np.asarray(transform, np.float64).reshape(16))
    L.check(lib.sp3_mesh_compact_vertices(pts.data_ptr(), L.ptr(rgba), n, L.ptr(faces), 0 if faces is None else faces.shape[0], L.ptr(valid),
                                          L.ptr(conf), float(conf_thresh), float(scale), m, ws.data_ptr(), out_pos.data_ptr(), L.ptr(out_rgba),
                                          info.data_ptr(), info.data_ptr() + 8, L.stream_ptr()), "sp3_mesh_compact_vertices")
    host = info.cpu().numpy()
    v = int(host[:1].view(np.int32)[0])
    return out_pos[:v], None if out_rgba is None else out_rgba[:v], host[2:8].reshape(2, 3).copy()


def _components_raw(lib, faces, n_vertices, cap):
    dev, nf = faces.device, faces.shape[0]
    out = dict(vertex_component=torch.empty(n_vertices, dtype=torch.int32, device=dev),
               face_component=torch.empty(nf, dtype=torch.int32, device=dev),
               component_faces=torch.empty(max(cap, 1), dtype=torch.int32, device=dev),
               component_vertices=torch.empty(max(cap, 1), dtype=torch.int32, device=dev))
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = _ws(lib.sp3_mesh_components_ws_bytes(n_vertices), dev)
    L.check(lib.sp3_mesh_components(faces.data_ptr(), nf, n_vertices, ws.data_ptr(), cap, out["vertex_component"].data_ptr(),
                                    out["face_component"].data_ptr(), out["component_faces"].data_ptr(),
                                    out["component_vertices"].data_ptr(), info.data_ptr(), L.stream_ptr()), "sp3_mesh_components")
    return out, info


def components(faces, n_vertices):
    """sp3_mesh_components: the connected pieces of the mesh faces int32 [F, 3] over vertices 0..n_vertices-1, by vertex
    connectivity (include/spann3r_hip.h "Mesh components").  -> dict(vertex_component int32 [V] (-1: no valid face names the vertex),
    face_component int32 [F] (-1: a face with an index outside 0..V-1), component_faces / component_vertices int32 [C], on the
    device; n_components, invalid_faces: ints).  Components are numbered by ascending smallest vertex.  One host read (C and the
    invalid count); if the first guess of the capacity for C was short the call runs once more at the reported size.  F = 0 or
    V = 0 returns empties (every face invalid when V = 0) and launches nothing."""
    faces = _dev(faces, "components: faces")
    n_vertices = int(n_vertices)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise RuntimeError("components: faces must be int32 [F, 3], got %s %s" % (faces.dtype, tuple(faces.shape)))
    if not 0 <= n_vertices < 2 ** 31 - 1 or faces.shape[0] >= 2 ** 31 - 1:
        raise ValueError("components: %d vertices, %d faces: both must stay below 2^31 - 1 (int32 indices)" % (n_vertices, faces.shape[0]))
    dev, nf = faces.device, faces.shape[0]
    if nf == 0 or n_vertices == 0:
        empty = torch.empty(0, dtype=torch.int32, device=dev)
        return dict(vertex_component=torch.full((n_vertices,), -1, dtype=torch.int32, device=dev),
                    face_component=torch.full((nf,), -1, dtype=torch.int32, device=dev), component_faces=empty,
                    component_vertices=empty.clone(), n_components=0, invalid_faces=nf)
    faces = faces.contiguous()
    lib = L.load()
    cap = min(n_vertices, max(4096, n_vertices // 16))
    out, info = _components_raw(lib, faces, n_vertices, cap)
    c, invalid = info.cpu().tolist()
    if c > cap:
        out, info = _components_raw(lib, faces, n_vertices, c)
        c2, invalid = info.cpu().tolist()
        if c2 != c:
            raise RuntimeError("components: the faces changed between two runs (%d -> %d components)" % (c, c2))
    out["component_faces"], out["component_vertices"] = out["component_faces"][:c], out["component_vertices"][:c]
    out.update(n_components=c, invalid_faces=invalid)
    return out


def keep_mask(component_faces, min_faces=0, keep_largest=None):
    """The selection rule of filter_components on the host: component_faces (array of C counts) -> bool [C].  A component is kept when
    it has at least min_faces faces and, with keep_largest = k, is among the first k in the order (faces descending, id ascending)."""
    cf = np.asarray(component_faces, np.int64).reshape(-1)
    keep = cf >= int(min_faces)
    if keep_largest is not None:
        k = int(keep_largest)
        if k < 0:
            raise ValueError("keep_largest must be >= 0, got %r" % (keep_largest,))
        first = np.zeros(len(cf), bool)
        first[np.lexsort((np.arange(len(cf)), -cf))[:k]] = True
        keep &= first
    return keep


def select_components(faces, n_vertices, min_faces=0, keep_largest=None):
    """components + keep_mask + sp3_mesh_select_faces: -> (the faces of the kept components int32 [K, 3], in their original order and
    with their indices unchanged; dict(total, kept, faces_removed)).  Faces with an index outside 0..n_vertices-1 are removed too.
    Host reads: the one of `components` and the component_faces that rank the components."""
    comp = components(faces, n_vertices)
    nf, c = faces.shape[0], comp["n_components"]
    cf = comp["component_faces"].cpu().numpy().astype(np.int64)
    keep = keep_mask(cf, min_faces, keep_largest)
    kept_faces = int(cf[keep].sum())
    stats = dict(total=c, kept=int(keep.sum()), faces_removed=nf - kept_faces)
    if kept_faces == 0:
        return faces.new_empty((0, 3)), stats
    lib = L.load()
    faces = faces.contiguous()
    keep_d = torch.from_numpy(keep.astype(np.uint8)).to(faces.device)
    out = torch.empty((nf, 3), dtype=torch.int32, device=faces.device)
    count = torch.zeros(1, dtype=torch.int32, device=faces.device)
    ws = _ws(lib.sp3_mesh_select_faces_ws_bytes(nf), faces.device)
    L.check(lib.sp3_mesh_select_faces(faces.data_ptr(), comp["face_component"].data_ptr(), nf, keep_d.data_ptr(), c,
                                      ws.data_ptr(), out.data_ptr(), count.data_ptr(), L.stream_ptr()), "sp3_mesh_select_faces")
    return out[:kept_faces], stats              # (the count the kernel reports is the sum of the kept components' faces)


def filter_components(m, min_faces=0, keep_largest=None):
    """Drop the floaters of a mesh: m is the dict scene_mesh / extract_mesh return (vertices fp32 [V, 3], colors uint8 [V, 4], faces
    int32 [F, 3], on the device).  A component (vertex connectivity) is kept when it has at least min_faces faces and, with
    keep_largest = k, is among the first k in the order (faces descending, id ascending).  -> the same kind of dict -- vertices, colors,
    faces, bounds recomputed -- plus components = dict(total, kept, faces_removed).  Kept faces and vertices stay in their original
    relative order, positions and colours bit for bit; everything removed gives an empty mesh, not an error."""
    if m.get("faces") is None:
        raise ValueError("filter_components: a point cloud has no faces to connect")
    vertices, faces = _dev(m["vertices"], "filter_components: vertices").float().contiguous(), _dev(m["faces"], "filter_components: faces")
    colors = m["colors"].contiguous()
    if colors.dtype != torch.uint8 or colors.shape != (vertices.shape[0], 4):
        raise RuntimeError("filter_components: colors must be uint8 [V, 4], got %s %s" % (colors.dtype, tuple(colors.shape)))
    kept, stats = select_components(faces, vertices.shape[0], min_faces, keep_largest)
    # (`kept` is select_components' own buffer, never the caller's faces: compact_vertices may rewrite its indices in place)
    pos, col, bounds = compact_vertices(vertices, colors.view(torch.int32).reshape(-1), faces=kept)
    out = {k: v for k, v in m.items() if k not in ("vertices", "colors", "faces", "bounds", "components")}
    out.update(vertices=pos, colors=col.contiguous().view(torch.uint8).reshape(-1, 4), faces=kept[:0] if pos.shape[0] == 0 else kept,
               bounds=bounds, components=stats)
    return out


def _table_log2(items):
    """the table of sp3_mesh_cluster / sp3_mesh_cluster_faces: the next power of two >= 2 x items"""
    return max(1, (2 * int(items) - 1).bit_length())


def _grid(cell, origin, what):
    """(cell as a float that fp32 holds, origin as a ctypes float[3]); raises before anything is launched"""
    try:
        c = float(np.float32(cell))
    except (TypeError, ValueError):
        raise ValueError("%s: cell must be a number, got %r" % (what, cell))
    if not (c > 0 and np.isfinite(c)):
        raise ValueError("%s: cell must be positive and finite (in fp32), got %r" % (what, cell))
    o = np.zeros(3, np.float32) if origin is None else np.asarray(_host(origin), np.float32).reshape(-1)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError("%s: origin must be 3 finite numbers, got %r" % (what, origin))
    return c, (C.c_float * 3)(*o.tolist())


def _cluster_raw(lib, vertices, rgba, cell, origin3, table_log2):
    """sp3_mesh_cluster at full capacity, no host read: -> (positions [V, 3], rgba [V] or None, vertex_cluster [V], info int32 [1])"""
    nv, dev = vertices.shape[0], vertices.device
    log2 = _table_log2(nv) if table_log2 is None else int(table_log2)
    if not (1 <= log2 <= 31 and 2 ** log2 > nv):
        raise ValueError("cluster_vertices: table_log2 %r: the table needs 2^1 .. 2^31 slots and more slots than the %d vertices" % (table_log2, nv))
    pos = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    col = torch.empty(nv, dtype=torch.int32, device=dev) if rgba is not None else None
    vc = torch.empty(nv, dtype=torch.int32, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _ws(lib.sp3_mesh_cluster_ws_bytes(nv, log2), dev)
    L.check(lib.sp3_mesh_cluster(vertices.data_ptr(), L.ptr(rgba), nv, origin3, cell, log2, ws.data_ptr(), pos.data_ptr(), L.ptr(col),
                                 vc.data_ptr(), info.data_ptr(), L.stream_ptr()), "sp3_mesh_cluster")
    return pos, col, vc, info


def _cluster_faces_raw(lib, faces, vc, dedup, table_log2=None):
    """sp3_mesh_cluster_faces at full capacity, no host read: -> (faces [F, 3], info int32 [4] = kept, invalid, collapsed, duplicate)"""
    nf, dev = faces.shape[0], faces.device
    log2 = 0 if not dedup else _table_log2(nf) if table_log2 is None else int(table_log2)
    out = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    ws = _ws(lib.sp3_mesh_cluster_faces_ws_bytes(nf, log2), dev)
    L.check(lib.sp3_mesh_cluster_faces(faces.data_ptr(), nf, vc.data_ptr(), vc.shape[0], int(bool(dedup)), log2, ws.data_ptr(), out.data_ptr(),
                                       info.data_ptr(), L.stream_ptr()), "sp3_mesh_cluster_faces")
    return out, info


def _check_vertices(vertices, rgba, what):
    vertices = _dev(vertices, what + ": vertices")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError("%s: vertices must be [V, 3], got %s" % (what, tuple(vertices.shape)))
    if vertices.shape[0] >= 2 ** 31 - 1:
        raise ValueError("%s: %d vertices: must stay below 2^31 - 1 (int32 indices)" % (what, vertices.shape[0]))
    vertices = vertices.float().contiguous()
    if rgba is not None:
        rgba = _dev(rgba, what + ": rgba").contiguous()
        if rgba.dtype == torch.uint8 and rgba.shape == (vertices.shape[0], 4):
            rgba = rgba.reshape(-1).view(torch.int32)              # (flat first: an empty [0, 4] has no unit stride to view through)
        if rgba.dtype != torch.int32 or rgba.shape != (vertices.shape[0],):
            raise RuntimeError("%s: colours must be int32 [V] (packed rgba) or uint8 [V, 4], got %s %s" % (what, rgba.dtype, tuple(rgba.shape)))
    return vertices, rgba


def cluster_vertices(vertices, cell, origin=None, rgba=None, table_log2=None):
    """sp3_mesh_cluster: vertex clustering on the uniform grid of `cell` from `origin` (include/spann3r_hip.h "Mesh simplification").
    vertices fp32 [V, 3], rgba int32 [V] (or uint8 [V, 4]; optional) -> dict(positions fp32 [C, 3], rgba int32 [C] or None,
    vertex_cluster int32 [V] (-1: a vertex that is not finite or beyond 2^30 cells), on the device; n_clusters).  A cluster is the
    set of vertices of one cell, numbered by its smallest vertex; its position is origin + (cell index + mean 16-bit fraction) * cell
    from integer sums, its colour the rounded mean per byte: the same bits every run.  origin defaults to zeros and never depends
    on the data, so two meshes simplified with the same cell share a grid.  table_log2: the hash table's size (default: the next
    power of two >= 2 V); the result does not depend on it.  One host read (C)."""
    cell, origin3 = _grid(cell, origin, "cluster_vertices")
    vertices, rgba = _check_vertices(vertices, rgba, "cluster_vertices")
    if vertices.shape[0] == 0:
        return dict(positions=vertices.new_empty((0, 3)), rgba=None if rgba is None else rgba[:0], n_clusters=0,
                    vertex_cluster=torch.empty(0, dtype=torch.int32, device=vertices.device))
    pos, col, vc, info = _cluster_raw(L.load(), vertices, rgba, cell, origin3, table_log2)
    c = int(info.cpu().item())
    return dict(positions=pos[:c], rgba=None if col is None else col[:c], vertex_cluster=vc, n_clusters=c)


def simplify(m, cell, origin=None, dedup=True, return_map=False, scale=1.0, transform=None):
    """Vertex clustering of a mesh (include/spann3r_hip.h "Mesh simplification"): m is the dict scene_mesh / extract_mesh return
    (vertices fp32 [V, 3], colors uint8 [V, 4], faces int32 [F, 3] or None, on the device).  Every vertex moves to the representative
    of its cell of the grid (cell, origin) -- cluster_vertices -- faces whose corners then coincide are dropped as collapsed, with
    dedup so are all but the first of the faces that became the same triangle with the same winding, and the clusters no kept face
    names are dropped.  -> the same kind of dict -- vertices, colors, faces, bounds recomputed -- plus simplify = dict(cell, clusters,
    faces_in, faces_collapsed, faces_duplicate, faces_invalid) and, with return_map, vertex_cluster int32 [V] (the cluster of every
    input vertex in the numbering of cluster_vertices, -1: unusable).  Kept faces stay in their original order and rotation.  A
    face with an index outside 0..V-1 or at an unusable vertex is invalid and dropped.  A cloud (faces None) is clustered too and
    comes back as a cloud; everything collapsed gives an empty mesh, not an error.  scale / transform: applied to the
    representatives by the final compaction, as extract_mesh applies them.  One host read of the counts (C and the four face
    counts), then compact_vertices' own of V and the bounds."""
    cell, origin3 = _grid(cell, origin, "simplify")
    colors = m["colors"]
    vertices, rgba = _check_vertices(m["vertices"], colors, "simplify")
    if colors.dtype != torch.uint8 or colors.shape != (vertices.shape[0], 4):
        raise RuntimeError("simplify: colors must be uint8 [V, 4], got %s %s" % (colors.dtype, tuple(colors.shape)))
    faces = m.get("faces")
    if faces is not None:
        faces = _dev(faces, "simplify: faces")
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
            raise RuntimeError("simplify: faces must be int32 [F, 3], got %s %s" % (faces.dtype, tuple(faces.shape)))
        if faces.shape[0] >= 2 ** 31 - 1:
            raise ValueError("simplify: %d faces: must stay below 2^31 - 1 (int32 indices)" % faces.shape[0])
        faces = faces.contiguous()
    nv, nf, dev = vertices.shape[0], 0 if faces is None else faces.shape[0], vertices.device
    lib = L.load()
    none = np.array([[np.inf] * 3, [-np.inf] * 3], np.float32)
    c, kept, invalid, collapsed, duplicate = 0, 0, nf, 0, 0
    vc = torch.empty(0, dtype=torch.int32, device=dev)
    pos, col, bounds, out_faces = vertices[:0], rgba[:0], none, None if faces is None else faces[:0]
    if nv > 0:
        cpos, ccol, vc, info = _cluster_raw(lib, vertices, rgba, cell, origin3, None)
        if nf > 0:
            kfaces, finfo = _cluster_faces_raw(lib, faces, vc, dedup)
            c, kept, invalid, collapsed, duplicate = torch.cat([info, finfo]).cpu().tolist()
            if kept > 0:
                out_faces = kfaces[:kept]
                pos, col, bounds = compact_vertices(cpos[:c], ccol[:c], faces=out_faces, scale=scale, transform=transform)
        else:
            c = int(info.cpu().item())
            if faces is None and c > 0:
                ok = torch.ones(c, dtype=torch.uint8, device=dev)
                pos, col, bounds = compact_vertices(cpos[:c], ccol[:c], valid=ok, scale=scale, transform=transform)
    out = {k: v for k, v in m.items() if k not in ("vertices", "colors", "faces", "bounds", "simplify", "vertex_cluster")}
    out.update(vertices=pos, colors=col.contiguous().view(torch.uint8).reshape(-1, 4), faces=out_faces, bounds=bounds,
               simplify=dict(cell=cell, clusters=c, faces_in=nf, faces_collapsed=collapsed, faces_duplicate=duplicate, faces_invalid=invalid))
    if return_map:
        out["vertex_cluster"] = vc
    return out


def _check_mesh(m, what):
    """(vertices fp32 [V, 3], rgba int32 [V] or None, faces int32 [F, 3]) of a mesh dict, contiguous on the device; a cloud raises"""
    if m.get("faces") is None:
        raise ValueError("%s: a point cloud has no faces (no surface to measure)" % what)
    vertices, rgba = _check_vertices(m["vertices"], m.get("colors"), what)
    faces = _dev(m["faces"], what + ": faces")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise RuntimeError("%s: faces must be int32 [F, 3], got %s %s" % (what, faces.dtype, tuple(faces.shape)))
    if faces.shape[0] >= 2 ** 31 - 1:
        raise ValueError("%s: %d faces: must stay below 2^31 - 1 (int32 indices)" % (what, faces.shape[0]))
    return vertices, rgba, faces.contiguous()


def _frames_raw(lib, vertices, faces, normals=True):
    """sp3_mesh_face_frames, no host read: -> (face_normals fp32 [F, 3] or None, cum int64 [F] (the uint64 bits; W < 2^63), info int64 [2])"""
    nv, nf, dev = vertices.shape[0], faces.shape[0], vertices.device
    fn = torch.empty((nf, 3), dtype=torch.float32, device=dev) if normals else None
    cum = torch.empty(nf, dtype=torch.int64, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    ws = _ws(lib.sp3_mesh_face_frames_ws_bytes(nf), dev)
    L.check(lib.sp3_mesh_face_frames(L.ptr(vertices) if nv else 0, nv, L.ptr(faces) if nf else 0, nf, ws.data_ptr(), L.ptr(fn) if nf else 0,
                                     cum.data_ptr() if nf else 0, info.data_ptr(), L.stream_ptr()), "sp3_mesh_face_frames")
    return fn, cum, info


def _read_info(info):
    """the one 16-byte host read: -> (W, dmax, the quantised area W / 2^32 * dmax / 2)"""
    host = info.cpu().numpy()
    w, dmax = int(host[0]), float(host[1:].view(np.float64)[0])
    return w, dmax, float(np.float64(w) / 4294967296.0 * np.float64(dmax) / 2.0)


def face_frames(m):
    """sp3_mesh_face_frames (include/spann3r_hip.h "Mesh surface sampling and normals") of the dict scene_mesh / extract_mesh /
    simplify return: per face the cross product n of two edges in fp64 and its length d, twice the area.  -> dict(face_normals fp32
    [F, 3] (zeros for a face that is invalid, not finite or without area), cum int64 [F] (the inclusive prefix sum of the integer
    weights floor(d / dmax * 2^32)), info int64 [2] (W, the bits of dmax), on the device; W int, dmax float, area float = W / 2^32 *
    dmax / 2, the QUANTISED area: a face below 2^-32 of the largest one counts as nothing).  The same bits every run.  One host read
    of 16 bytes.  A cloud raises ValueError."""
    vertices, _, faces = _check_mesh(m, "face_frames")
    fn, cum, info = _frames_raw(L.load(), vertices, faces)
    w, dmax, area = _read_info(info)
    return dict(face_normals=fn, cum=cum, info=info, W=w, dmax=dmax, area=area)


def surface_area(m):
    """The quantised area of face_frames as a float.  A cloud raises ValueError."""
    vertices, _, faces = _check_mesh(m, "surface_area")
    return _read_info(_frames_raw(L.load(), vertices, faces, normals=False)[2])[2]


def sample_surface(m, n, seed=0, return_faces=False):
    """n points drawn independently and uniformly by area from the surface of a mesh dict (include/spann3r_hip.h "Mesh surface
    sampling and normals"; sp3_mesh_face_frames + sp3_mesh_sample): sample k takes its face from the integer prefix sum of the face
    weights and its place from two 24-bit barycentric coordinates, all three from a counter-based generator of (seed, k) -- the same
    bits every run, and the first n of a longer draw are the shorter draw.  -> dict(points fp32 [n, 3], normals fp32 [n, 3] (the exact
    unit normal of the face drawn), colors uint8 [n, 4] (the corners' colours mixed per byte; None when the mesh has none), area
    (float, the quantised area) and, with return_faces, faces int32 [n]), tensors on the device.  One host read of 16 bytes between
    the two calls: a mesh with no area to sample (no face, or every face invalid, non-finite or degenerate) with n > 0 raises
    ValueError; n = 0 gives empty tensors.  A cloud raises ValueError."""
    n, seed = int(n), int(seed)
    if n < 0 or n >= 2 ** 40:
        raise ValueError("sample_surface: n = %d must lie in 0 .. 2^40 - 1" % n)
    vertices, rgba, faces = _check_mesh(m, "sample_surface")
    dev, lib = vertices.device, L.load()
    _, cum, info = _frames_raw(lib, vertices, faces, normals=False)
    w, _, area = _read_info(info)
    if n > 0 and w == 0:
        raise ValueError("sample_surface: %d faces over %d vertices, none valid, finite and with an area: no area to sample" %
                         (faces.shape[0], vertices.shape[0]))
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    col = torch.empty(n, dtype=torch.int32, device=dev) if rgba is not None else None
    fidx = torch.empty(n, dtype=torch.int32, device=dev)
    if n > 0:
        L.check(lib.sp3_mesh_sample(vertices.data_ptr(), L.ptr(rgba), vertices.shape[0], faces.data_ptr(), faces.shape[0], cum.data_ptr(),
                                    info.data_ptr(), n, seed & (2 ** 64 - 1), points.data_ptr(), normals.data_ptr(), L.ptr(col), fidx.data_ptr(),
                                    L.stream_ptr()), "sp3_mesh_sample")
    out = dict(points=points, normals=normals, colors=None if col is None else col.view(torch.uint8).reshape(-1, 4), area=area)
    if return_faces:
        out["faces"] = fidx
    return out


def vertex_normals(m):
    """Area-weighted unit vertex normals fp32 [V, 3] of a mesh dict, on the device (include/spann3r_hip.h "Mesh surface sampling and
    normals"; sp3_mesh_face_frames + sp3_mesh_vertex_normals): every face adds its cross product, quantised to 2^-30 of the largest
    one, to its three vertices in 64-bit integers -- the same bits every run and for any order of the faces.  A vertex no valid face
    names, or whose faces cancel, gets (0, 0, 0).  No host read.  A cloud raises ValueError.  (Recompute after simplify: the
    normals of a mesh do not survive it.)"""
    vertices, _, faces = _check_mesh(m, "vertex_normals")
    nv, nf, lib = vertices.shape[0], faces.shape[0], L.load()
    out = torch.empty((nv, 3), dtype=torch.float32, device=vertices.device)
    if nv == 0:
        return out
    _, _, info = _frames_raw(lib, vertices, faces, normals=False)
    ws = _ws(lib.sp3_mesh_vertex_normals_ws_bytes(nv), vertices.device)
    L.check(lib.sp3_mesh_vertex_normals(vertices.data_ptr(), nv, L.ptr(faces) if nf else 0, nf, info.data_ptr(), ws.data_ptr(), out.data_ptr(),
                                        L.stream_ptr()), "sp3_mesh_vertex_normals")
    return out


# ------------------------------------------------------------------------------------------------ mesh topology and smoothing
_REPORT_KEYS = ("edges", "boundary", "interior", "inconsistent", "nonmanifold", "faces_usable", "faces_unusable", "vertices_referenced")
_BOUNDARY_MODES = ("fixed", "free")


class MeshTopology:
    """The edge table and vertex adjacency of a mesh dict (include/spann3r_hip.h "Mesh topology and smoothing"): built once, reusable
    while the faces do not change -- positions may move, which is what smooth(topology=) relies on.  A face is usable when its three
    indices lie in 0..V-1 and are pairwise distinct; the unique pairs (lo, hi) of the usable faces' half-edges h = 3 f + c are the
    edges, numbered in ascending (lo, hi) order.  Two stable sorts (the edge keys, the directed keys of the unique edges) and ten
    launches; ONE host read, the 64 bytes behind `report`, between the two halves.  A cloud raises ValueError; F = 0, V = 0 or no
    usable face give E = 0, empty tables, all-zero vertex_offsets and closed = False (F = 0 or V = 0 launch nothing).
    Attributes, on the device: faces (the contiguous int32 [F, 3] it was built from), edges int32 [E, 2], edge_first int32 [E + 1],
    half_edges int32 [3 x usable faces] (edge e: half_edges[edge_first[e] : edge_first[e + 1]], ascending; its faces are h // 3),
    edge_uses, edge_fwd int32 [E], edge_class uint8 [E] (0 boundary, 1 interior, 2 inconsistent, 3 non-manifold), vertex_offsets
    int32 [V + 1], vertex_neighbors int32 [2 E] (row v: the distinct neighbours of v, ascending), vertex_boundary uint8 [V].
    On the host: n_vertices, n_faces, n_edges, boundary_vertices, report = dict(edges, boundary, interior, inconsistent,
    nonmanifold, faces_usable, faces_unusable, vertices_referenced, euler = vertices_referenced - edges + faces_usable, closed =
    every edge interior and E > 0)."""

    def __init__(self, m):
        vertices, _, faces = _check_mesh(m, "MeshTopology")
        nv, nf, dev = vertices.shape[0], faces.shape[0], faces.device
        if 3 * nf >= 2 ** 31:
            raise ValueError("MeshTopology: %d faces: 3 F must stay below 2^31 (int32 half-edges)" % nf)
        self.faces, self.n_vertices, self.n_faces = faces, nv, nf
        i32 = dict(dtype=torch.int32, device=dev)
        host = [0] * 9
        host[6] = nf                                             # (V = 0: every face is unusable)
        self.vertex_boundary = torch.zeros(nv, dtype=torch.uint8, device=dev)
        if nf > 0 and nv > 0:
            lib, n = L.load(), 3 * nf
            keys = torch.empty(n, dtype=torch.int64, device=dev)
            info = torch.zeros(16, **i32)
            L.check(lib.sp3_mesh_edge_keys(faces.data_ptr(), nf, nv, keys.data_ptr(), info.data_ptr(), L.stream_ptr()), "sp3_mesh_edge_keys")
            keys, order = torch.sort(keys, stable=True)
            edges, first = torch.empty((n, 2), **i32), torch.empty(n + 1, **i32)
            uses, fwd, half = torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(n, **i32)
            cls = torch.empty(n, dtype=torch.uint8, device=dev)
            ws = _ws(lib.sp3_mesh_edge_table_ws_bytes(n, nv), dev)
            L.check(lib.sp3_mesh_edge_table(keys.data_ptr(), order.data_ptr(), n, nv, ws.data_ptr(), edges.data_ptr(), first.data_ptr(),
                                            uses.data_ptr(), fwd.data_ptr(), cls.data_ptr(), half.data_ptr(), self.vertex_boundary.data_ptr(),
                                            info.data_ptr(), L.stream_ptr()), "sp3_mesh_edge_table")
            host = info.cpu().tolist()[:9]                       # the one read
        e, usable = host[0], host[5]
        self.n_edges, self.boundary_vertices = e, host[8]
        self.report = dict(zip(_REPORT_KEYS, host[:8]))
        self.report.update(euler=host[7] - e + usable, closed=e > 0 and host[2] == e)
        self.vertex_offsets = torch.zeros(nv + 1, **i32)
        if e == 0:
            self.edges, self.edge_first = torch.empty((0, 2), **i32), torch.zeros(1, **i32)
            self.edge_uses, self.edge_fwd, self.half_edges, self.vertex_neighbors = (torch.empty(0, **i32) for _ in range(4))
            self.edge_class = torch.empty(0, dtype=torch.uint8, device=dev)
            return
        if 2 * e >= 2 ** 31:
            raise ValueError("MeshTopology: %d edges: 2 E must stay below 2^31 (int32 row offsets)" % e)
        # (copies, so that the tables do not hold their 3 F capacity alive)
        self.edges, self.edge_first, self.half_edges = edges[:e].clone(), first[:e + 1].clone(), half[:3 * usable].clone()
        self.edge_uses, self.edge_fwd, self.edge_class = uses[:e].clone(), fwd[:e].clone(), cls[:e].clone()
        dkeys = torch.empty(2 * e, dtype=torch.int64, device=dev)
        L.check(lib.sp3_mesh_adjacency_keys(self.edges.data_ptr(), e, dkeys.data_ptr(), L.stream_ptr()), "sp3_mesh_adjacency_keys")
        dkeys = torch.sort(dkeys, stable=True)[0]
        self.vertex_neighbors = torch.empty(2 * e, **i32)
        L.check(lib.sp3_mesh_adjacency_rows(dkeys.data_ptr(), 2 * e, nv, self.vertex_offsets.data_ptr(), self.vertex_neighbors.data_ptr(),
                                            L.stream_ptr()), "sp3_mesh_adjacency_rows")

    def matches(self, faces):
        """True when this topology was built from exactly this face list (int32 [F, 3] on the device); compares the indices unless
        it is the very tensor"""
        if faces.shape != self.faces.shape or faces.device != self.faces.device:
            return False
        return faces.data_ptr() == self.faces.data_ptr() or bool(torch.equal(faces, self.faces))

    def smooth_pass(self, positions, factor, fixed=None, out=None):
        """sp3_mesh_smooth_pass: positions fp32 [V, 3] -> out (another buffer): every vertex with neighbours that `fixed` (uint8 [V] or
        None) does not hold moves by factor x (mean of its row - itself), the row summed in its order in fp64.  No host read."""
        if out is None:
            out = torch.empty_like(positions)
        if self.n_vertices > 0:
            L.check(L.load().sp3_mesh_smooth_pass(positions.data_ptr(), self.n_vertices, self.vertex_offsets.data_ptr(),
                                                  L.ptr(self.vertex_neighbors) if self.n_edges else 0, L.ptr(fixed), float(factor),
                                                  out.data_ptr(), L.stream_ptr()), "sp3_mesh_smooth_pass")
        return out


def topology(m):
    """MeshTopology(m): the edge table, the vertex adjacency and the manifold report of a mesh dict, on the device."""
    return MeshTopology(m)


def _own_topology(what, topology, vertices, faces):
    """the MeshTopology of these very faces: built when None; one built from another face list raises ValueError"""
    if topology is None:
        return MeshTopology(dict(vertices=vertices, faces=faces))
    if not isinstance(topology, MeshTopology):
        raise TypeError("%s: topology must be a MeshTopology, got %s" % (what, type(topology).__name__))
    if topology.n_vertices != vertices.shape[0] or topology.n_faces != faces.shape[0] or not topology.matches(faces):
        raise ValueError("%s: the topology was built from another mesh (%d vertices, %d faces; this one has %d, %d, or other indices)" %
                         (what, topology.n_vertices, topology.n_faces, vertices.shape[0], faces.shape[0]))
    return topology


def smooth(m, iterations=10, lam=0.5, mu=-0.53, boundary="fixed", topology=None):
    """Taubin's lambda|mu low-pass on the vertices of a mesh dict (include/spann3r_hip.h "Mesh topology and smoothing"; Open3D's
    filter_smooth_taubin has these defaults): each of `iterations` rounds is one pass with factor lam, then one with mu unless mu ==
    0 (mu = 0: a plain Laplacian, which shrinks the surface; the negative step is what keeps its volume).  A pass moves every vertex
    by factor x (the mean of its distinct neighbours - itself), uniform weights, summed in ascending neighbour order in fp64: the
    same bits every run and for any order of the faces.  boundary="fixed" holds the end points of boundary edges where they are -- a
    TSDF surface is open at the rim of what was observed, and the rim must not creep inward; "free" holds nothing.  Vertices no
    usable face names do not move.  topology: a MeshTopology of these very faces (built when None); one built from another face
    list raises ValueError.  -> the same kind of dict: colours, faces and every other key pass through, vertices are new (the
    caller's are not written), bounds is recomputed, smooth = dict(iterations, lam, mu, boundary, fixed_vertices).  iterations = 0
    returns the same bits.  Normals do not survive it: recompute vertex_normals.  Host reads: the topology's one, and the bounds.
    A cloud raises ValueError."""
    iterations, lam, mu = int(iterations), float(lam), float(mu)
    if iterations < 0:
        raise ValueError("smooth: iterations must be >= 0, got %d" % iterations)
    if boundary not in _BOUNDARY_MODES:
        raise ValueError("smooth: boundary must be one of %s, got %r" % (_BOUNDARY_MODES, boundary))
    vertices, _, faces = _check_mesh(m, "smooth")
    topology = _own_topology("smooth", topology, vertices, faces)
    fixed = topology.vertex_boundary if boundary == "fixed" else None
    cur = vertices
    if iterations > 0 and vertices.shape[0] > 0:
        spare = [torch.empty_like(vertices), torch.empty_like(vertices)]      # ping-pong: the caller's buffer is only ever read
        for factor in ([lam] if mu == 0.0 else [lam, mu]) * iterations:
            cur = topology.smooth_pass(cur, factor, fixed, out=spare[0])
            spare.reverse()
    else:
        cur = vertices.clone()
    if cur.shape[0] > 0:
        bounds = torch.stack([cur.amin(0), cur.amax(0)]).cpu().numpy().astype(np.float32)
    else:
        bounds = np.array([[np.inf] * 3, [-np.inf] * 3], np.float32)
    out = {k: v for k, v in m.items() if k not in ("vertices", "bounds", "smooth")}
    out.update(vertices=cur, bounds=bounds, smooth=dict(iterations=iterations, lam=lam, mu=mu, boundary=boundary,
                                                        fixed_vertices=topology.boundary_vertices if fixed is not None else 0))
    return out


# ------------------------------------------------------------------------------------------------ mesh boundary loops and hole filling
_LOOP_REPORT_KEYS = ("boundary", "loops", "open", "irregular_vertices", "longest")


class BoundaryLoops:
    """The boundary edges of a mesh dict as ordered loops (include/spann3r_hip.h "Mesh boundary loops and hole filling"): the class-0
    edges of its MeshTopology (built when topology is None; a foreign one raises ValueError) are the elements 0..B-1 in ascending
    edge number, each directed as its one face walks it; an element's successor is the element leaving its end vertex where exactly
    one leaves and one enters, so bow-ties, non-manifold edges and flipped windings end a chain instead of being guessed through.
    The closed cycles are the loops, numbered by their smallest element (the head); list ranking by pointer doubling,
    ceil(log2(max(B, 2))) rounds of one launch each.  ONE host read after the last launch, the 64 bytes behind `report`; it sizes
    the CSR.  B = 0 launches nothing and gives empty tables.  A cloud raises ValueError.
    Attributes, on the device, int32: edge, half_edge, src, dst, next (-1: the chain ends), loop, rank (-1 on an open chain), all
    [B]; loop_first [L + 1], loop_members [B - open] (row l: the elements of loop l in walk order from its head).  On the host:
    topology, n_boundary, n_loops, rounds, report = dict(boundary, loops, open (elements on open chains), irregular_vertices,
    longest (the longest loop, 0 without one))."""

    def __init__(self, m, topology=None):
        vertices, _, faces = _check_mesh(m, "BoundaryLoops")
        topology = _own_topology("BoundaryLoops", topology, vertices, faces)
        nv, nf, dev, b = vertices.shape[0], faces.shape[0], faces.device, topology.report["boundary"]
        self.topology, self.n_boundary, self.rounds = topology, b, 0
        i32 = dict(dtype=torch.int32, device=dev)
        self.edge, self.half_edge, self.src, self.dst, self.next, self.loop, self.rank = (torch.empty(b, **i32) for _ in range(7))
        host = [0] * 5
        if b > 0:
            lib, e, st = L.load(), topology.n_edges, L.stream_ptr()
            vout, vin, vleave = (torch.empty(nv, **i32) for _ in range(3))
            info = torch.zeros(16, **i32)
            ws = _ws(lib.sp3_mesh_boundary_elements_ws_bytes(e), dev)
            L.check(lib.sp3_mesh_boundary_elements(faces.data_ptr(), nf, nv, topology.edge_class.data_ptr(), topology.edge_first.data_ptr(),
                                                   topology.half_edges.data_ptr(), e, b, ws.data_ptr(), self.edge.data_ptr(),
                                                   self.half_edge.data_ptr(), self.src.data_ptr(), self.dst.data_ptr(), vout.data_ptr(),
                                                   vin.data_ptr(), vleave.data_ptr(), st), "sp3_mesh_boundary_elements")
            L.check(lib.sp3_mesh_boundary_link(self.dst.data_ptr(), b, vout.data_ptr(), vin.data_ptr(), vleave.data_ptr(), nv,
                                               self.next.data_ptr(), info.data_ptr(), st), "sp3_mesh_boundary_link")
            self.rounds = int(lib.sp3_mesh_boundary_rounds(b))
            state = torch.empty((b, 4), **i32)
            ws_rank = _ws(lib.sp3_mesh_boundary_rank_ws_bytes(b), dev)
            L.check(lib.sp3_mesh_boundary_rank(self.next.data_ptr(), b, ws_rank.data_ptr(), state.data_ptr(), st), "sp3_mesh_boundary_rank")
            first, members = torch.empty(b + 1, **i32), torch.empty(b, **i32)
            ws_loops = _ws(lib.sp3_mesh_boundary_loops_ws_bytes(b), dev)
            L.check(lib.sp3_mesh_boundary_loops(self.next.data_ptr(), state.data_ptr(), b, ws_loops.data_ptr(), self.loop.data_ptr(), self.rank.data_ptr(),
                                                first.data_ptr(), members.data_ptr(), info.data_ptr(), st), "sp3_mesh_boundary_loops")
            host = info.cpu().tolist()[:6]                       # the one read
            if host[0] != b or host[5] != b - host[2]:
                raise RuntimeError("BoundaryLoops: %d elements, %d on open chains and %d on loops do not add up to B = %d" %
                                   (host[0], host[2], host[5], b))
            # (copies, so that the CSR does not hold its B + 1 capacity alive)
            self.loop_first, self.loop_members = first[:host[1] + 1].clone(), members[:host[5]].clone()
        else:
            self.loop_first, self.loop_members = torch.zeros(1, **i32), torch.empty(0, **i32)
        self.n_loops = host[1]
        self.report = dict(zip(_LOOP_REPORT_KEYS, [b] + host[1:5]))


def boundary_loops(m, topology=None):
    """BoundaryLoops(m, topology): the boundary elements, their loops and the loop report of a mesh dict, on the device."""
    return BoundaryLoops(m, topology)


def fill_holes(m, max_edges, topology=None, loops=None):
    """Closes every boundary loop of at most max_edges >= 3 edges of a mesh dict (include/spann3r_hip.h "Mesh boundary loops and hole
    filling"): a loop of 3 gets one face, a longer one a new vertex at the mean of its vertices (summed in walk order in fp64; the
    colour is the rounded integer mean per channel) and a fan of len faces, all wound like their neighbours.  New vertices follow the
    old ones in loop order, new faces in (loop, rank) order.  Open chains (bow-ties, non-manifold or inconsistent neighbourhoods) and
    longer loops stay open -- choose max_edges below the rim of what was observed.  loops: the BoundaryLoops of this mesh (built when
    None, from `topology` when that is given); one of another face list raises ValueError.  -> the same kind of dict: vertices,
    colors (when present) and faces are new tensors (the caller's are not written), bounds is unchanged (a mean lies inside the box
    of its loop), normals are dropped (recompute vertex_normals), every other key passes through, fill = dict(max_edges, loops,
    filled, vertices_added, faces_added, open).  With nothing to fill it returns equal bits.  Host reads: those of the topology and
    the loops where they are built here, and one more of 64 bytes, the totals.  A cloud raises ValueError."""
    max_edges = int(max_edges)
    if max_edges < 3:
        raise ValueError("fill_holes: max_edges must be >= 3 (the shortest loop), got %d" % max_edges)
    vertices, rgba, faces = _check_mesh(m, "fill_holes")
    if loops is None:
        loops = BoundaryLoops(dict(vertices=vertices, faces=faces), topology)
    elif not isinstance(loops, BoundaryLoops):
        raise TypeError("fill_holes: loops must be a BoundaryLoops, got %s" % type(loops).__name__)
    else:
        _own_topology("fill_holes", loops.topology, vertices, faces)
        if topology is not None and topology is not loops.topology:
            _own_topology("fill_holes", topology, vertices, faces)
    nv, nf, nl, dev = vertices.shape[0], faces.shape[0], loops.n_loops, faces.device
    added_v = added_f = filled = 0
    if nl > 0:
        lib, st = L.load(), L.stream_ptr()
        vertex_at, face_at = torch.empty(nl, dtype=torch.int32, device=dev), torch.empty(nl, dtype=torch.int32, device=dev)
        info = torch.zeros(16, dtype=torch.int32, device=dev)
        ws = _ws(lib.sp3_mesh_fill_count_ws_bytes(nl), dev)
        L.check(lib.sp3_mesh_fill_count(loops.loop_first.data_ptr(), nl, min(max_edges, 2 ** 31 - 1), ws.data_ptr(), vertex_at.data_ptr(),
                                        face_at.data_ptr(), info.data_ptr(), st), "sp3_mesh_fill_count")
        added_v, added_f, filled = info.cpu().tolist()[:3]       # the one read
    if nv + added_v >= 2 ** 31 - 1 or 3 * (nf + added_f) >= 2 ** 31:
        raise ValueError("fill_holes: %d + %d vertices, %d + %d faces: the filled mesh must keep int32 indices and half-edges" %
                         (nv, added_v, nf, added_f))
    new_v = torch.empty((nv + added_v, 3), dtype=torch.float32, device=dev)
    new_f = torch.empty((nf + added_f, 3), dtype=torch.int32, device=dev)
    new_c = torch.empty(nv + added_v, dtype=torch.int32, device=dev) if rgba is not None else None
    new_v[:nv].copy_(vertices)
    new_f[:nf].copy_(faces)
    if new_c is not None:
        new_c[:nv].copy_(rgba)
    if added_f > 0:
        L.check(lib.sp3_mesh_fill_emit(vertices.data_ptr(), L.ptr(rgba), nv, nf, loops.src.data_ptr(), loops.dst.data_ptr(),
                                       loops.loop.data_ptr(), loops.rank.data_ptr(), loops.loop_first.data_ptr(), loops.loop_members.data_ptr(),
                                       nl, loops.loop_members.shape[0], vertex_at.data_ptr(), face_at.data_ptr(), added_v, added_f,
                                       new_v.data_ptr(), L.ptr(new_c), new_f.data_ptr(), st), "sp3_mesh_fill_emit")
    out = {k: v for k, v in m.items() if k not in ("vertices", "colors", "faces", "normals", "fill")}
    out.update(vertices=new_v, faces=new_f)
    if "colors" in m:
        out["colors"] = None if new_c is None else new_c.view(torch.uint8).reshape(-1, 4)
    out["fill"] = dict(max_edges=max_edges, loops=nl, filled=filled, vertices_added=added_v, faces_added=added_f, open=loops.report["open"])
    return out


# ------------------------------------------------------------------------------------------------ mesh distance
PAIRS_PER_FACE_CAP = 8          # (cell, face) references a TriangleGrid may hold per face before its cells are made larger
FACES_PER_CELL = 0.5            # what cell_grid.choose_grid aims the cell edge at: a surface leaves most cells of its box empty
DIST_RING_BUDGET = 3            # rings walked before a query is handed to the brute-force kernels


def _tri_cell_counts(lib, vertices, faces, g):
    """sp3_mesh_tri_cell_count: -> int64 [F] on the device, the number of cells every face is registered in (0: not usable)"""
    counts = torch.empty(faces.shape[0], dtype=torch.int64, device=faces.device)
    L.check(lib.sp3_mesh_tri_cell_count(L.ptr(vertices) if vertices.shape[0] else 0, vertices.shape[0], L.ptr(faces) if faces.shape[0] else 0,
                                        faces.shape[0], C.byref(g), L.ptr(counts) if faces.shape[0] else 0, L.stream_ptr()),
            "sp3_mesh_tri_cell_count")
    return counts


def _usable_faces(lib, v, f, what, tail, count=None):
    """the number of usable faces of a mesh -- `count`, or one per face registered in a grid of one cell (one 8-byte host read) --
    or the ValueError of a mesh that has none"""
    if count is None:
        count = int(_tri_cell_counts(lib, v, f, G.one_cell()).sum().item()) if f.shape[0] else 0
    if count == 0:
        raise ValueError("%s: %d faces over %d vertices, none valid, finite and with an area: %s" % (what, f.shape[0], v.shape[0], tail))
    return count


def _finite_vertex_box(v):
    """the box of the finite coordinates of v [V, 3] -> float64 numpy [2, 3] (one 48-byte host read); zeros without vertices"""
    if v.shape[0] == 0:
        return np.zeros((2, 3))
    fin = torch.isfinite(v)
    inf = torch.tensor(math.inf, device=v.device)
    return G.finite_box(torch.where(fin, v, inf).amin(0), torch.where(fin, v, -inf).amax(0))


def _ptrs(out, *keys):
    return tuple(out[k].data_ptr() for k in keys)


def _mesh_args(a):
    """(vertices, nverts, faces, nfaces) of a structure as the query entry points take them"""
    return L.ptr(a.vertices), a.vertices.shape[0], a.faces.data_ptr(), a.faces.shape[0]


_DIST_OUT = ("dist", "closest", "face", "region")
_RAY_OUT = ("t", "face", "bary", "point", "side")

# What a query asks a mesh through -- TriangleGrid, TriangleBVH, _AllFaces -- has one surface: vertices, faces, query_order(q),
# dist_query(q, out, ring_budget) and ray_query(o, d, t_min, t_max, cull, out) for n >= 1 queries, ray_views(table, table_d, T,
# pixel_offset) for T >= 1 views, stats() (what the structure reports of itself) and read_stats(ws) (what a call counted: the one
# 32-byte host read).  Every method owns its workspace and its one library call, and returns the workspace -- or None when the
# call counted nothing worth reading (the brute-force kernels).


class _AllFaces:
    """method="brute": every query against every face (sp3_mesh_dist_brute / sp3_mesh_ray_brute), also what a TriangleGrid of one
    cell answers point and ray queries with.  grid: the TriangleGrid whose dims, h and pairs stats() reports, if there is one."""

    def __init__(self, vertices, faces, grid=None):
        self.vertices, self.faces, self.grid = vertices, faces, grid

    def stats(self):
        return dict(grid=(1, 1, 1), h=None, pairs=0) if self.grid is None else self.grid.stats()

    def dist_query(self, q, out, ring_budget=None):
        lib, n = L.load(), q.shape[0]
        ws = _ws(lib.sp3_mesh_dist_query_ws_bytes(n), q.device)
        L.check(lib.sp3_mesh_dist_brute(q.data_ptr(), n, *_mesh_args(self), ws.data_ptr(), *_ptrs(out, *_DIST_OUT), L.stream_ptr()), "sp3_mesh_dist_brute")

    def ray_query(self, o, d, t_min, t_max, cull, out):
        lib, n = L.load(), o.shape[0]
        ws = _ws(lib.sp3_mesh_ray_ws_bytes(n), o.device)
        L.check(lib.sp3_mesh_ray_brute(o.data_ptr(), d.data_ptr(), n, *_mesh_args(self), t_min, t_max, cull, ws.data_ptr(), *_ptrs(out, *_RAY_OUT),
                                       L.stream_ptr()), "sp3_mesh_ray_brute")

    def ray_occluded(self, o, d, t_min, t_max, cull, occluded):
        """(no brute-force occlusion kernel: the closest hit of every ray, then face >= 0)"""
        n, dev = o.shape[0], o.device
        out = dict(t=torch.empty(n, dtype=torch.float32, device=dev), face=torch.empty(n, dtype=torch.int32, device=dev),
                   bary=torch.empty((n, 3), dtype=torch.float32, device=dev), point=torch.empty((n, 3), dtype=torch.float32, device=dev),
                   side=torch.empty(n, dtype=torch.uint8, device=dev))
        self.ray_query(o, d, t_min, t_max, cull, out)
        occluded.copy_(out["face"] >= 0)


class TriangleGrid(G.Grid):
    """The faces of a mesh dict registered in a cell grid (include/spann3r_hip.h "Mesh distance"): built once, reused for any number
    of query sets by point_mesh_distance.  The cell edge starts from cell_grid.choose_grid on the box of the finite vertices with the
    number of usable faces and grows by 1.25 while the (cell, face) references exceed PAIRS_PER_FACE_CAP per face; a grid of one cell
    holds no references and is answered by the brute-force kernels.  Host reads: 8 bytes for the usable faces, 48 for the box, 8 per
    try of h (one for near-uniform faces such as marching tetrahedra's).  h: start from this cell edge instead of choose_grid's.  A
    mesh without a usable face raises ValueError; a cloud too.
    Attributes: g (lib.NnGrid), dims, h, usable, pairs, tries, pair_face int32 [pairs], cell_start int32 [cells + 1]."""

    def __init__(self, m, h=None):
        lib = L.load()
        self.vertices, _, self.faces = _check_mesh(m, "TriangleGrid")
        v, f = self.vertices, self.faces
        nf, dev = f.shape[0], v.device
        self.usable = _usable_faces(lib, v, f, "TriangleGrid", "no surface to measure against")
        box = _finite_vertex_box(v)
        ext = box[1] - box[0]
        if h is None:
            h, dims = G.choose_grid(box[0], box[1], self.usable, occupancy=FACES_PER_CELL)
        else:                                        # the caller's first cell edge (experiments; a huge one gives the one-cell grid)
            h, dims = G.grow_to_cap(ext, float(h))
        self.tries = 0
        while True:
            self.tries += 1
            g = G.make_grid(box, h, dims)
            if dims == (1, 1, 1):
                counts, pairs = None, 0
                break
            counts = _tri_cell_counts(lib, v, f, g)
            pairs = int(counts.sum().item())
            if pairs <= min(PAIRS_PER_FACE_CAP * nf, 2 ** 31 - 2):
                break
            h, dims = G.grow_to_cap(ext, h * 1.25)
        self.g, self.h, self.dims, self.pairs = g, h, dims, pairs
        self.pair_face = self.cell_start = None
        if pairs:
            offsets = torch.cumsum(counts, 0) - counts
            cell = torch.empty(pairs, dtype=torch.int32, device=dev)
            face = torch.empty(pairs, dtype=torch.int32, device=dev)
            L.check(lib.sp3_mesh_tri_cell_fill(v.data_ptr(), v.shape[0], f.data_ptr(), nf, C.byref(g), offsets.data_ptr(), pairs, cell.data_ptr(),
                                               face.data_ptr(), L.stream_ptr()), "sp3_mesh_tri_cell_fill")
            order, self.cell_start = G.cell_table(cell, dims[0] * dims[1] * dims[2])
            self.pair_face = face[order].contiguous()

    def stats(self):
        return dict(grid=tuple(self.dims), h=self.h, pairs=self.pairs)

    def read_stats(self, ws):
        return dict(zip(("fallback_queries", "cells_visited", "faces_evaluated"), G.read_head(ws)))

    def _grid_args(self):
        return L.ptr(self.pair_face), self.pairs, L.ptr(self.cell_start), C.byref(self.g)

    def dist_query(self, q, out, ring_budget=DIST_RING_BUDGET):
        if self.pairs == 0:
            return _AllFaces(self.vertices, self.faces, self).dist_query(q, out)
        lib, n = L.load(), q.shape[0]
        ws = _ws(lib.sp3_mesh_dist_query_ws_bytes(n), q.device)
        L.check(lib.sp3_mesh_dist_query(q.data_ptr(), self.query_order(q).data_ptr(), n, *_mesh_args(self), *self._grid_args(), int(ring_budget),
                                        ws.data_ptr(), *_ptrs(out, *_DIST_OUT), L.stream_ptr()), "sp3_mesh_dist_query")
        return ws

    def ray_query(self, o, d, t_min, t_max, cull, out):
        if self.pairs == 0:
            return _AllFaces(self.vertices, self.faces, self).ray_query(o, d, t_min, t_max, cull, out)
        lib, n = L.load(), o.shape[0]
        ws = _ws(lib.sp3_mesh_ray_ws_bytes(n), o.device)
        L.check(lib.sp3_mesh_ray_query(o.data_ptr(), d.data_ptr(), self.query_order(o).data_ptr(), n, *_mesh_args(self), *self._grid_args(), t_min,
                                       t_max, cull, ws.data_ptr(), *_ptrs(out, *_RAY_OUT), L.stream_ptr()), "sp3_mesh_ray_query")
        return ws

    def ray_views(self, table, table_d, T, pixel_offset):
        """(a grid of one cell goes to sp3_mesh_ray_views too: its kernel then scans every face)"""
        lib = L.load()
        ws = _ws(lib.sp3_mesh_ray_ws_bytes(0), table_d.device)
        L.check(lib.sp3_mesh_ray_views(table, table_d.data_ptr(), T, pixel_offset, *_mesh_args(self), *self._grid_args(), ws.data_ptr(),
                                       L.stream_ptr()), "sp3_mesh_ray_views")
        return ws

    def ray_occluded(self, o, d, t_min, t_max, cull, occluded):
        if self.pairs == 0:
            return _AllFaces(self.vertices, self.faces, self).ray_occluded(o, d, t_min, t_max, cull, occluded)
        lib, n = L.load(), o.shape[0]
        ws = _ws(32, o.device)
        L.check(lib.sp3_mesh_ray_occluded(o.data_ptr(), d.data_ptr(), self.query_order(o).data_ptr(), n, *_mesh_args(self), *self._grid_args(), t_min,
                                          t_max, cull, ws.data_ptr(), occluded.data_ptr(), L.stream_ptr()), "sp3_mesh_ray_occluded")
        return ws

    def point_views(self, table, table_d, T, pixel_offset, bias, cull, p, count, mask):
        """(a grid of one cell goes to sp3_mesh_point_views too: its kernel then scans every face)"""
        ws = _ws(32, p.device)
        L.check(L.load().sp3_mesh_point_views(table, table_d.data_ptr(), T, pixel_offset, bias, cull, p.data_ptr(), self.query_order(p).data_ptr(),
                                              p.shape[0], *_mesh_args(self), *self._grid_args(), ws.data_ptr(), count.data_ptr(), L.ptr(mask),
                                              L.stream_ptr()), "sp3_mesh_point_views")
        return ws


_KEY_NONE = 2 ** 63 - 1          # sp3_mesh_bvh_keys: an item that is not usable


class TriangleBVH:
    """A bounding-volume hierarchy over the faces of a mesh dict (include/spann3r_hip.h "Mesh BVH"): built once, reused for any
    number of query sets through the bvh= keyword of point_mesh_distance, ray_mesh_intersect and render_depth_maps, which then return
    what they return with a TriangleGrid, bit for bit.  The usable faces are sorted by the Morton key of their box centres, cell_grid.
    BVH_LEAF of them make a leaf and BVH_ARITY nodes a node of the level above (cell_grid.bvh_levels: no pointers, index arithmetic
    and a table of level offsets); one launch builds each level.  Unlike the grid it has no cell edge to choose -- faces 64-fold
    apart in size cost no retries -- and a query far from the surface costs a walk of the tree's depth instead of the brute-force
    kernels.  Host reads: 8 bytes for the usable faces, 48 for the box.  A mesh without a usable face raises ValueError; a cloud too.
    Attributes: vertices, faces, usable, order int32 [usable] (the usable faces in key order), levels, level_sizes, level_offsets,
    node_lo / node_hi fp32 [nodes, 3] (level l at level_offsets[l] .. level_offsets[l + 1]), slack, b (lib.MeshBvh)."""

    def __init__(self, m):
        lib = L.load()
        self.vertices, _, self.faces = _check_mesh(m, "TriangleBVH")
        v, f = self.vertices, self.faces
        nf, dev = f.shape[0], v.device
        box = _finite_vertex_box(v)
        self._box = (C.c_float * 6)(*box.astype(np.float32).reshape(6).tolist())      # (fp32 vertices: their box is exact in fp32)
        keys = self._keys(lib, v, f, nf) if nf else None
        self.usable = _usable_faces(lib, v, f, "TriangleBVH", "no surface to measure against",
                                    count=int((keys != _KEY_NONE).sum().item()) if nf else 0)
        self.order = torch.sort(keys, stable=True)[1][:self.usable].to(torch.int32)
        self.b, self.level_sizes, self.level_offsets = G.make_bvh(box, self.usable)
        self.levels, self.slack = self.b.levels, float(self.b.slack)
        self.node_lo = torch.empty((self.level_offsets[-1], 3), dtype=torch.float32, device=dev)
        self.node_hi = torch.empty((self.level_offsets[-1], 3), dtype=torch.float32, device=dev)
        L.check(lib.sp3_mesh_bvh_build(L.ptr(v), v.shape[0], f.data_ptr(), nf, self.order.data_ptr(), C.byref(self.b), self.node_lo.data_ptr(),
                                       self.node_hi.data_ptr(), L.stream_ptr()), "sp3_mesh_bvh_build")

    def _keys(self, lib, points, faces, n):
        """sp3_mesh_bvh_keys of n faces, or (faces None) of the n points: int64 [n] on the device"""
        keys = torch.empty(n, dtype=torch.int64, device=points.device)
        L.check(lib.sp3_mesh_bvh_keys(L.ptr(points) if points.shape[0] else 0, points.shape[0], None if faces is None else L.ptr(faces) if n else 0,
                                      n, self._box, L.ptr(keys) if n else 0, L.stream_ptr()), "sp3_mesh_bvh_keys")
        return keys

    def query_order(self, q):
        """the queries sorted by their own Morton key in the tree's box: the lanes of a wave then descend through the same nodes"""
        return torch.sort(self._keys(L.load(), q, None, q.shape[0]), stable=True)[1]

    def tree_args(self):
        """(order, node_lo, node_hi, descriptor) as the query entry points take them"""
        return self.order.data_ptr(), self.node_lo.data_ptr(), self.node_hi.data_ptr(), C.byref(self.b)

    def stats(self):
        return dict(grid=(1, 1, 1), h=None, pairs=0, nodes_visited=0, levels=self.levels, nodes=self.level_offsets[-1])

    def read_stats(self, ws):
        _, nodes, faces = G.read_head(ws)
        return dict(nodes_visited=nodes, faces_evaluated=faces)

    def dist_query(self, q, out, ring_budget=None):
        """(no ring budget: no query falls back)"""
        ws = _ws(32, q.device)                       # the 32-byte head alone
        L.check(L.load().sp3_mesh_bvh_dist_query(q.data_ptr(), self.query_order(q).data_ptr(), q.shape[0], *_mesh_args(self), *self.tree_args(),
                                                 ws.data_ptr(), *_ptrs(out, *_DIST_OUT), L.stream_ptr()), "sp3_mesh_bvh_dist_query")
        return ws

    def ray_query(self, o, d, t_min, t_max, cull, out):
        ws = _ws(32, o.device)
        L.check(L.load().sp3_mesh_bvh_ray_query(o.data_ptr(), d.data_ptr(), self.query_order(o).data_ptr(), o.shape[0], *_mesh_args(self),
                                                *self.tree_args(), t_min, t_max, cull, ws.data_ptr(), *_ptrs(out, *_RAY_OUT), L.stream_ptr()),
                "sp3_mesh_bvh_ray_query")
        return ws

    def ray_views(self, table, table_d, T, pixel_offset):
        lib = L.load()
        ws = _ws(lib.sp3_mesh_ray_ws_bytes(0), table_d.device)
        L.check(lib.sp3_mesh_bvh_ray_views(table, table_d.data_ptr(), T, pixel_offset, *_mesh_args(self), *self.tree_args(), ws.data_ptr(),
                                           L.stream_ptr()), "sp3_mesh_bvh_ray_views")
        return ws

    def ray_occluded(self, o, d, t_min, t_max, cull, occluded):
        ws = _ws(32, o.device)
        L.check(L.load().sp3_mesh_bvh_ray_occluded(o.data_ptr(), d.data_ptr(), self.query_order(o).data_ptr(), o.shape[0], *_mesh_args(self),
                                                   *self.tree_args(), t_min, t_max, cull, ws.data_ptr(), occluded.data_ptr(), L.stream_ptr()),
                "sp3_mesh_bvh_ray_occluded")
        return ws

    def point_views(self, table, table_d, T, pixel_offset, bias, cull, p, count, mask):
        ws = _ws(32, p.device)
        L.check(L.load().sp3_mesh_bvh_point_views(table, table_d.data_ptr(), T, pixel_offset, bias, cull, p.data_ptr(),
                                                  self.query_order(p).data_ptr(), p.shape[0], *_mesh_args(self), *self.tree_args(), ws.data_ptr(),
                                                  count.data_ptr(), L.ptr(mask), L.stream_ptr()), "sp3_mesh_bvh_point_views")
        return ws


def _accel(m, grid, bvh, method, what, tail="no surface to hit"):
    """What a call is to ask: a TriangleBVH (bvh = True: built on m, or one built on this mesh), else the caller's TriangleGrid, else
    -- method "brute" -- every face, else a new TriangleGrid.  `tail` ends the ValueError of a mesh without a usable face."""
    if bvh is not None and bvh is not False:
        if grid is not None or method != "grid":
            raise ValueError("%s: bvh= replaces the grid: leave grid=None and method at its default, got grid %s, method %r" %
                             (what, "given" if grid is not None else "None", method))
        if bvh is True:
            return TriangleBVH(m)
        if not isinstance(bvh, TriangleBVH):
            raise ValueError("%s: bvh must be None, True or a TriangleBVH, got %s" % (what, type(bvh).__name__))
        return bvh
    if method == "brute":
        if grid is not None:                         # its mesh, and its dims in the stats; none of its cells
            return _AllFaces(grid.vertices, grid.faces, grid)
        v, _, f = _check_mesh(m, what)               # no grid to build: only the count of usable faces, for the same ValueError
        _usable_faces(L.load(), v, f, what, tail)
        return _AllFaces(v, f)
    return TriangleGrid(m) if grid is None else grid


def point_mesh_distance(points, m, grid=None, method="grid", return_stats=False, ring_budget=DIST_RING_BUDGET, bvh=None):
    """The exact unsigned distance from every point fp32 [N, 3] (device) to the surface of a mesh dict (include/spann3r_hip.h "Mesh
    distance"; sp3_mesh_dist_query / sp3_mesh_dist_brute) -> dict(dist fp32 [N], closest fp32 [N, 3], face int32 [N] (the face the
    closest point lies on, the smallest index among equals), region uint8 [N] (0..6: A, B, edge AB, C, edge AC, edge BC, inside)),
    tensors on the device.  A non-finite query gets +inf, itself, -1, 255.  The result is a function of the inputs alone: the same
    bits for either method, for any grid and every run.
    method: "grid" (a TriangleGrid -- pass one as `grid` to reuse it, it must have been built on this mesh -- walked ring by ring,
    the brute-force kernels for what `ring_budget` rings leave open or when the grid is one cell) or "brute" (every query against
    every face: the in-tree cross-check).  return_stats: also `stats` = dict(fallback_queries, cells_visited, faces_evaluated, grid,
    h, pairs), one 32-byte host read.  A mesh without a usable face raises ValueError; N = 0 launches nothing.
    bvh: a TriangleBVH built on this mesh, or True to build one: the queries walk the tree instead (sp3_mesh_bvh_dist_query) and no
    query falls back, however far from the surface it lies; `grid` must then be None and `method` its default, else ValueError.
    stats gains nodes_visited, levels and nodes; fallback_queries and cells_visited are 0, grid (1, 1, 1)."""
    if method not in ("grid", "brute"):
        raise ValueError("point_mesh_distance: method must be 'grid' or 'brute', got %r" % (method,))
    q = _dev(points, "point_mesh_distance: points")
    if q.dim() != 2 or q.shape[1] != 3 or q.dtype != torch.float32:
        raise RuntimeError("point_mesh_distance: points must be fp32 [N, 3], got %s %s" % (q.dtype, tuple(q.shape)))
    q = q.contiguous()
    acc = _accel(m, grid, bvh, method, "point_mesh_distance", "no surface to measure against")
    n, dev = q.shape[0], q.device
    out = dict(dist=torch.empty(n, dtype=torch.float32, device=dev), closest=torch.empty((n, 3), dtype=torch.float32, device=dev),
               face=torch.empty(n, dtype=torch.int32, device=dev), region=torch.empty(n, dtype=torch.uint8, device=dev))
    stats = dict(fallback_queries=0, cells_visited=0, faces_evaluated=0, **acc.stats())
    if n > 0:
        ws = acc.dist_query(q, out, ring_budget)
        if ws is None:                               # nothing counted: every query went to the brute-force kernels
            stats["fallback_queries"] = n
        elif return_stats:
            stats.update(acc.read_stats(ws))
    if return_stats:
        out["stats"] = stats
    return out


# ------------------------------------------------------------------------------------------------ mesh rays
_CULL = {None: 0, "back": 1, "front": 2}


def _ray_args(what, origins, directions, t_min, t_max, cull, method):
    """the argument checks of ray_mesh_intersect and ray_mesh_occluded -> (origins, directions contiguous on the device, t_min, t_max floats)"""
    if method not in ("grid", "brute"):
        raise ValueError("%s: method must be 'grid' or 'brute', got %r" % (what, method))
    if cull not in _CULL:
        raise ValueError("%s: cull must be None, 'back' or 'front', got %r" % (what, cull))
    t_min, t_max = float(t_min), float(t_max)
    if not (0.0 <= t_min <= t_max):
        raise ValueError("%s: 0 <= t_min <= t_max, got t_min %r, t_max %r" % (what, t_min, t_max))
    o, d = _dev(origins, what + ": origins"), _dev(directions, what + ": directions")
    for name, x in (("origins", o), ("directions", d)):
        if x.dim() != 2 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise RuntimeError("%s: %s must be fp32 [N, 3], got %s %s" % (what, name, x.dtype, tuple(x.shape)))
    if o.shape != d.shape:
        raise RuntimeError("%s: %d origins and %d directions" % (what, o.shape[0], d.shape[0]))
    return o.contiguous(), d.contiguous(), t_min, t_max


def ray_mesh_intersect(origins, directions, m, grid=None, t_min=0.0, t_max=math.inf, cull=None, method="grid", return_stats=False, bvh=None):
    """What every ray hits first on the surface of a mesh dict (include/spann3r_hip.h "Mesh rays"; sp3_mesh_ray_query /
    sp3_mesh_ray_brute): origins, directions fp32 [N, 3] (device; directions need no normalising: t is in units of |d|) ->
    dict(t fp32 [N] (+inf: a miss), face int32 [N] (-1; the smallest index among faces hit at the same t), bary fp32 [N, 3] (the
    weights of the face's corners A, B, C), point fp32 [N, 3] (o + t d), side uint8 [N] (0: the ray's origin sees the face
    counter-clockwise, 1: clockwise, 255: a miss)), tensors on the device.  Hits lie in t_min <= t <= t_max.  The test is watertight:
    no ray passes between two faces that share an edge.  A ray with a non-finite component or d = 0 hits nothing.  The result is a
    function of the inputs alone: the same bits for either method, for any grid and every run.
    cull: None, "back" (hits with side 1 are ignored) or "front" (side 0).  method: "grid" (a TriangleGrid -- pass one as `grid` to
    reuse it, it must have been built on this mesh -- walked cell by cell along the ray, rays served in the order of
    grid.query_order(origins); the brute-force kernels when the grid is one cell) or "brute" (every ray against every face: the
    in-tree cross-check).  return_stats: also `stats` = dict(cells_visited, faces_evaluated, grid, h, pairs), one 32-byte host read.
    A mesh without a usable face raises ValueError; N = 0 launches nothing.
    bvh: a TriangleBVH built on this mesh, or True to build one: the rays walk the tree instead (sp3_mesh_bvh_ray_query), served in
    the order of bvh.query_order(origins); `grid` must then be None and `method` its default, else ValueError.  stats gains
    nodes_visited, levels and nodes; cells_visited is 0, grid (1, 1, 1)."""
    o, d, t_min, t_max = _ray_args("ray_mesh_intersect", origins, directions, t_min, t_max, cull, method)
    acc = _accel(m, grid, bvh, method, "ray_mesh_intersect")
    n, dev = o.shape[0], o.device
    out = dict(t=torch.empty(n, dtype=torch.float32, device=dev), face=torch.empty(n, dtype=torch.int32, device=dev),
               bary=torch.empty((n, 3), dtype=torch.float32, device=dev), point=torch.empty((n, 3), dtype=torch.float32, device=dev),
               side=torch.empty(n, dtype=torch.uint8, device=dev))
    stats = dict(cells_visited=0, faces_evaluated=0, **acc.stats())
    if n > 0:
        ws = acc.ray_query(o, d, t_min, t_max, _CULL[cull], out)
        if return_stats and ws is not None:
            stats.update((k, x) for k, x in acc.read_stats(ws).items() if k in stats)      # (no ray falls back: that count is not reported)
    if return_stats:
        out["stats"] = stats
    return out


def _camera_args(what, intrinsics, cam2world, size, near, far, pixel_offset, opengl):
    """the camera arguments of render_depth_maps and point_visibility, checked -> (h, w, near, far, pixel_offset, cam2world float64
    [T, 4, 4] with opengl undone, (fu, fv, cu, cv) float64 [T, 4], world-to-camera fp32 [T, 12]: fusion.camera_tables')"""
    from .fusion import _host_array, camera_tables
    h, w = (int(x) for x in size)
    if h < 1 or w < 1:
        raise ValueError("%s: size %s must be (h, w) >= 1" % (what, size))
    near, far, pixel_offset = float(near), float(far), float(pixel_offset)
    if not (0.0 <= near <= far):
        raise ValueError("%s: 0 <= near <= far, got near %r, far %r" % (what, near, far))
    if not math.isfinite(pixel_offset):
        raise ValueError("%s: pixel_offset must be finite, got %r" % (what, pixel_offset))
    P = _host_array(cam2world)
    P = P[None] if P.ndim == 2 else P.reshape(-1, 4, 4) if P.size == 0 else P
    if P.ndim != 3 or P.shape[1:] != (4, 4):
        raise ValueError("%s: cam2world %s must be [4, 4] or [T, 4, 4]" % (what, P.shape))
    if opengl:
        P = P * np.array([1.0, -1.0, -1.0, 1.0])
    fk, w2c = camera_tables(intrinsics, P, P.shape[0])
    if not (fk[:, :2] != 0).all():
        raise ValueError("%s: intrinsics with a zero focal length" % what)
    return h, w, near, far, pixel_offset, P, fk, w2c


def render_depth_maps(m, intrinsics, cam2world, size, near=0.0, far=math.inf, grid=None, pixel_offset=0.0, opengl=False, return_faces=False,
                      return_stats=False, bvh=None):
    """Depth maps of a mesh dict seen from T cameras in ONE launch (include/spann3r_hip.h "Mesh rays"; sp3_mesh_ray_views) -- what
    spann3r/tools/render_dtu.py:54-80 render_depth_maps obtains from pyrender: intrinsics [3, 3] or [T, 3, 3], cam2world [T, 4, 4] (or
    one [4, 4]), size = (h, w) -> dict(depth fp32 [T, h, w]: camera z of the first surface along the ray of every pixel, 0 where
    the ray hits nothing between near and far (camera z, held as fp32)), device tensors; return_faces: also face int32 [T, h, w] (-1: a miss) and
    bary fp32 [T, h, w, 3].  Pixel centres lie at integer coordinates, the package's convention: the ray of pixel (u, v) has the
    camera-frame direction ((u + pixel_offset - cx) / fx, (v + pixel_offset - cy) / fy, 1).  pyrender samples at pixel centres + 0.5,
    so pixel_offset=0.5 reproduces its sampling (pyrender is not available to test against: that parity is unpinned).
    opengl=True: the poses are the ones render_dtu.py hands to pyrender -- camera looking down -z, y up: columns 1 and 2 negated --
    and that is undone here.  Both faces of the surface are seen.  grid: a TriangleGrid built on this mesh, to reuse it.  Skewed
    intrinsics and non-finite or singular poses are refused as fusion.camera_tables refuses them.  return_stats: also `stats` as
    ray_mesh_intersect's (one 32-byte host read); otherwise nothing synchronises beyond the grid's build.
    bvh: a TriangleBVH built on this mesh, or True to build one: the rays walk the tree instead (sp3_mesh_bvh_ray_views), the same
    maps bit for bit; `grid` must then be None, else ValueError."""
    h, w, near, far, pixel_offset, P, fk, _ = _camera_args("render_depth_maps", intrinsics, cam2world, size, near, far, pixel_offset, opengl)
    T = P.shape[0]                                               # (the inverse is only computed for its checks)
    acc = _accel(m, grid, bvh, "grid", "render_depth_maps")
    dev = acc.vertices.device
    out = dict(depth=torch.empty((T, h, w), dtype=torch.float32, device=dev))
    if return_faces:
        out["face"] = torch.empty((T, h, w), dtype=torch.int32, device=dev)
        out["bary"] = torch.empty((T, h, w, 3), dtype=torch.float32, device=dev)
    stats = dict(cells_visited=0, faces_evaluated=0, **acc.stats())
    if T > 0:
        table = (L.MeshRayView * T)()
        for i in range(T):
            e = table[i]
            e.depth = out["depth"][i].data_ptr()
            e.face = out["face"][i].data_ptr() if return_faces else None
            e.bary = out["bary"][i].data_ptr() if return_faces else None
            e.row_stride, e.w, e.h = w, w, h
            e.fu, e.fv, e.cu, e.cv = (float(x) for x in fk[i])
            e.c2w[:] = P[i, :3].reshape(12).astype(np.float32).tolist()
            e.near, e.far = near, far
        table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        ws = acc.ray_views(table, table_d, T, pixel_offset)
        if return_stats:
            stats.update((k, x) for k, x in acc.read_stats(ws).items() if k in stats)
    if return_stats:
        out["stats"] = stats
    return out


# ------------------------------------------------------------------------------------------------ mesh visibility
def ray_mesh_occluded(origins, directions, m, grid=None, t_min=0.0, t_max=math.inf, cull=None, method="grid", return_stats=False, bvh=None):
    """Whether every ray hits ANYTHING on the surface of a mesh dict (include/spann3r_hip.h "Mesh visibility"; sp3_mesh_ray_occluded /
    sp3_mesh_bvh_ray_occluded) -> bool [N] on the device, exactly ray_mesh_intersect(...)["face"] >= 0 for the same arguments -- a
    pure function of the inputs -- at the cost of a walk that stops at the first hit and one byte per ray.  Arguments, their checks
    and the choice of the structure are ray_mesh_intersect's; method="brute" (and a grid of one cell) IS ray_mesh_intersect's
    brute-force route followed by the comparison.  return_stats: -> (the mask, stats as ray_mesh_intersect's).  A ray that hits
    nothing walks what the closest-hit walk walks; only hits are cheaper."""
    o, d, t_min, t_max = _ray_args("ray_mesh_occluded", origins, directions, t_min, t_max, cull, method)
    acc = _accel(m, grid, bvh, method, "ray_mesh_occluded")
    n = o.shape[0]
    occluded = torch.empty(n, dtype=torch.bool, device=o.device)
    stats = dict(cells_visited=0, faces_evaluated=0, **acc.stats())
    if n > 0:
        ws = acc.ray_occluded(o, d, t_min, t_max, _CULL[cull], occluded)
        if return_stats and ws is not None:
            stats.update((k, x) for k, x in acc.read_stats(ws).items() if k in stats)
    return (occluded, stats) if return_stats else occluded


def point_visibility(points, m, intrinsics, cam2world, size, near=0.0, far=math.inf, bias=1e-3, pixel_offset=0.0, opengl=False, cull=None,
                     grid=None, bvh=None, return_mask=False, return_stats=False):
    """How many of T cameras see every point fp32 [N, 3] (device) past the surface of a mesh dict, in ONE launch (include/
    spann3r_hip.h "Mesh visibility"; sp3_mesh_point_views / sp3_mesh_bvh_point_views) -> dict(count int32 [N], views = T;
    return_mask: mask bool [T, N]; return_stats: stats as ray_mesh_intersect's), device tensors.  A camera sees a point when the point lies in front
    of it with near <= camera z <= far, projects into the image -- pixel centres at integer coordinates + pixel_offset, a pixel
    reaching half a unit either side -- and the segment from the camera to the point hits no face between camera z = near and
    (1 - bias) of the way.  bias is a RELATIVE DEPTH TOLERANCE, a convention and not an error bound: it drops the hit of a mesh's
    vertex on its own faces (t = 1 to fp32 rounding); widen it for unwelded sheets that overlap within noise; it must lie in
    [0, 1).  Surfaces in front of the near plane do not occlude, as render_depth_maps does not draw them.  A non-finite point is seen
    by nobody.  Cameras (intrinsics, cam2world, size = (h, w), opengl) are render_depth_maps' and are refused as it refuses them.
    cull: None, "back" or "front", which hits occlude (ray_mesh_intersect's).  grid / bvh: a TriangleGrid / TriangleBVH built on
    this mesh (bvh=True builds one); the counts are the same bits either way.  For many views of a large mesh prefer bvh=: its walk
    is the cheaper one per shadow ray (profiles/mesh_visibility.txt).  N = 0 or T = 0 launches nothing."""
    h, w, near, far, pixel_offset, P, fk, w2c = _camera_args("point_visibility", intrinsics, cam2world, size, near, far, pixel_offset, opengl)
    bias = float(bias)
    if not (0.0 <= bias < 1.0) or not (0.0 <= float(np.float32(bias)) < 1.0):
        raise ValueError("point_visibility: bias %r must lie in [0, 1)" % (bias,))
    if cull not in _CULL:
        raise ValueError("point_visibility: cull must be None, 'back' or 'front', got %r" % (cull,))
    p = _dev(points, "point_visibility: points")
    if p.dim() != 2 or p.shape[1] != 3 or p.dtype != torch.float32:
        raise RuntimeError("point_visibility: points must be fp32 [N, 3], got %s %s" % (p.dtype, tuple(p.shape)))
    p = p.contiguous()
    acc = _accel(m, grid, bvh, "grid", "point_visibility", "no surface to hide behind")
    T, n, dev = P.shape[0], p.shape[0], p.device
    out = dict(count=torch.zeros(n, dtype=torch.int32, device=dev), views=T)
    mask = torch.zeros((T, n), dtype=torch.uint8, device=dev) if return_mask else None
    stats = dict(cells_visited=0, faces_evaluated=0, **acc.stats())
    if T > 0 and n > 0:
        table = (L.MeshVisView * T)()
        for i in range(T):
            e = table[i]
            e.w, e.h = w, h
            e.fu, e.fv, e.cu, e.cv = (float(x) for x in fk[i])
            e.near, e.far = near, far
            e.c2w[:] = P[i, :3].reshape(12).astype(np.float32).tolist()
            e.w2c[:] = w2c[i].tolist()
        table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        ws = acc.point_views(table, table_d, T, pixel_offset, bias, _CULL[cull], p, out["count"], mask)
        if return_stats:
            stats.update((k, x) for k, x in acc.read_stats(ws).items() if k in stats)
    if return_mask:
        out["mask"] = mask.bool()
    if return_stats:
        out["stats"] = stats
    return out


def vertex_visibility(m, intrinsics, cam2world, size, **kw):
    """point_visibility of a mesh dict's own vertices against its own surface: count int32 [V] = the cameras that see each vertex"""
    vertices, _, _ = _check_mesh(m, "vertex_visibility")
    return point_visibility(vertices, m, intrinsics, cam2world, size, **kw)


_VIS_MODE = {"any": 0, "all": 1}


def cull_to_views(m, intrinsics, cam2world, size, near=0.0, far=math.inf, bias=1e-3, pixel_offset=0.0, opengl=False, cull=None, grid=None,
                  bvh=None, mode="any", min_views=1, return_map=False):
    """The part of a mesh that T cameras could see -- the cull_mesh step NICE-SLAM-style evaluations apply to both meshes before
    accuracy and completion (include/spann3r_hip.h "Mesh visibility"): vertex_visibility, then a vertex is SEEN when at least
    min_views cameras see it, and a face is kept when its indices are valid and (mode="any") one of its vertices or (mode="all") all
    three are seen (sp3_mesh_vis_face_class, sp3_mesh_select_faces).  m is the dict scene_mesh / extract_mesh return; -> the same
    kind of dict -- vertices, colors, faces, bounds recomputed (compact_vertices drops what no kept face names), everything else
    carried as filter_components carries it -- plus visibility = dict(views, vertices_seen, faces_in, faces_kept); return_map: also
    vertex_views int32 [V of the input] (the count per input vertex).  Kept faces and vertices stay in their order and rotation,
    positions and colours bit for bit; everything culled gives an empty mesh, not an error; a cloud raises ValueError.  The camera
    and structure arguments are point_visibility's.  Two host reads (the counts, compact_vertices' own) beyond the structure's."""
    if mode not in _VIS_MODE:
        raise ValueError("cull_to_views: mode must be 'any' or 'all', got %r" % (mode,))
    min_views = int(min_views)
    if min_views < 0:
        raise ValueError("cull_to_views: min_views must be >= 0, got %r" % (min_views,))
    vertices, rgba, faces = _check_mesh(m, "cull_to_views")
    vis = point_visibility(vertices, m, intrinsics, cam2world, size, near=near, far=far, bias=bias, pixel_offset=pixel_offset, opengl=opengl,
                           cull=cull, grid=grid, bvh=bvh)
    count = vis["count"]
    lib, nv, nf, dev = L.load(), vertices.shape[0], faces.shape[0], faces.device
    cls = torch.empty(nf, dtype=torch.int32, device=dev)
    L.check(lib.sp3_mesh_vis_face_class(faces.data_ptr(), nf, nv, L.ptr(count) if nv else 0, min_views, _VIS_MODE[mode], cls.data_ptr(),
                                        L.stream_ptr()), "sp3_mesh_vis_face_class")
    keep = torch.tensor([0, 1], dtype=torch.uint8, device=dev)
    kept = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int32, device=dev)                  # [0]: faces kept, [1]: vertices seen
    ws = _ws(lib.sp3_mesh_select_faces_ws_bytes(nf), dev)
    L.check(lib.sp3_mesh_select_faces(faces.data_ptr(), cls.data_ptr(), nf, keep.data_ptr(), 2, ws.data_ptr(), kept.data_ptr(), info.data_ptr(),
                                      L.stream_ptr()), "sp3_mesh_select_faces")
    info[1] = (count >= min_views).sum()
    nkept, seen = info.cpu().tolist()
    kept = kept[:nkept]
    # (`kept` is this function's own buffer, never the caller's faces: compact_vertices rewrites its indices in place)
    pos, col, bounds = compact_vertices(vertices, rgba, faces=kept)
    out = {k: v for k, v in m.items() if k not in ("vertices", "colors", "faces", "bounds", "visibility", "vertex_views")}
    out.update(vertices=pos, faces=kept[:0] if pos.shape[0] == 0 else kept, bounds=bounds,
               visibility=dict(views=vis["views"], vertices_seen=seen, faces_in=nf, faces_kept=nkept))
    if "colors" in m:
        out["colors"] = None if col is None else col.contiguous().view(torch.uint8).reshape(-1, 4)
    if return_map:
        out["vertex_views"] = count
    return out


def pts3d_to_mesh(img, pts3d, valid=None):
    """app.py:68-105 (pts3d_to_trimesh) for device tensors img, pts3d [h, w, 3] and valid bool [h, w]: dict(vertices [h w, 3],
    faces int64 [F, 3], face_colors [F, 3]) with the reference's order: four blocks (tl, tr, bl), (bl, tr, tl), (tr, bl, br), (br, bl, tr),
    row-major over the cells, faces with an invalid vertex removed; the first two blocks take the cell's top-left colour, the last
    two its bottom-right colour."""
    img, pts3d = _dev(img, "pts3d_to_mesh: img"), _dev(pts3d, "pts3d_to_mesh: pts3d")
    if img.dim() != 3 or img.shape[-1] != 3 or img.shape != pts3d.shape:
        raise RuntimeError("pts3d_to_mesh: img %s and pts3d %s must both be [h, w, 3]" % (tuple(img.shape), tuple(pts3d.shape)))
    h, w = img.shape[:2]
    if valid is not None:
        if _dev(valid, "pts3d_to_mesh: valid").shape != (h, w):
            raise RuntimeError("pts3d_to_mesh: valid %s does not match the %d x %d pointmap" % (tuple(valid.shape), h, w))
        valid = valid.to(torch.uint8).contiguous()
    faces, colour_px, _ = build_faces(1, h, w, img.device, valid=valid)
    return dict(vertices=pts3d.reshape(-1, 3), faces=faces.long(), face_colors=img.reshape(-1, 3)[colour_px.long()])


def cat_meshes(meshes):
    """app.py:38-47: one mesh of several, the faces of mesh i shifted by the vertices before it (the inputs stay as they are; the
    reference shifts them in place)"""
    if len(meshes) == 0:
        raise ValueError("cat_meshes: no meshes")
    offs = np.cumsum([0] + [len(m["vertices"]) for m in meshes])
    return dict(vertices=torch.cat([m["vertices"] for m in meshes]), face_colors=torch.cat([m["face_colors"] for m in meshes]),
                faces=torch.cat([m["faces"] + int(o) for m, o in zip(meshes, offs)]))


def scene_mesh(pts_all, images_all, conf_all, conf_thresh, as_pointcloud=False):
    """app.py:132-167 in one call for device tensors pts_all, images_all [t, h, w, 3] (colours in [0, 1]) and conf_all [t, h, w]:
    the pixels with (conf - 1) / conf > conf_thresh (and a finite point), as one mesh of all frames or, with as_pointcloud, as a cloud.
    Positions are 10 x the points (app.py:143) under the transform of app.py:165-167, which evaluates to diag(-1, -1, 1, 1).
    -> dict(vertices fp32 [V, 3], colors uint8 [V, 4], faces int32 [F, 3] (forward windings only; None for a cloud), bounds float32
    numpy [2, 3] = per-axis min and max of the vertices), vertices / colors / faces on the device.  Only referenced vertices are kept."""
    pts_all, images_all, conf_all = (_dev(x, "scene_mesh: " + n) for x, n in ((pts_all, "pts_all"), (images_all, "images_all"), (conf_all, "conf_all")))
    if pts_all.dim() != 4 or pts_all.shape[-1] != 3 or images_all.shape != pts_all.shape or conf_all.shape != pts_all.shape[:3]:
        raise RuntimeError("scene_mesh: mismatched shapes: pts_all %s and images_all %s must be [t, h, w, 3], conf_all %s [t, h, w]" %
                           (tuple(pts_all.shape), tuple(images_all.shape), tuple(conf_all.shape)))
    t, h, w = conf_all.shape
    n = t * h * w
    pts, conf = pts_all.float().contiguous(), conf_all.float().contiguous()
    rgba = torch.empty(n, dtype=torch.int32, device=pts.device)
    L.check(L.load().sp3_pack_rgba8(images_all.float().contiguous().data_ptr(), n, rgba.data_ptr(), L.stream_ptr()), "sp3_pack_rgba8")
    faces = None
    if as_pointcloud:
        pos, col, bounds = compact_vertices(pts.reshape(-1, 3), rgba, conf=conf, conf_thresh=conf_thresh, scale=SCALE, transform=TRANSFORM)
    else:
        faces, _, _ = build_faces(t, h, w, pts.device, conf=conf, conf_thresh=conf_thresh, pts=pts, both_windings=False)
        pos, col, bounds = compact_vertices(pts.reshape(-1, 3), rgba, faces=faces, scale=SCALE, transform=TRANSFORM)
    return dict(vertices=pos, colors=col.view(torch.uint8).reshape(-1, 4), faces=faces, bounds=bounds)


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def write_glb(path, vertices, colors, faces=None, bounds=None, normals=None):
    """A glTF 2.0 binary file of one primitive: POSITION fp32 VEC3 (with min / max; `bounds` [2, 3] if already known), COLOR_0
    normalised unsigned byte VEC4 (uint8 [V, 3] gets alpha 255), and with faces [F, 3] uint32 indices, mode 4 (TRIANGLES) and a
    doubleSided material; without faces mode 0 (POINTS).  With normals (fp32 [V, 3], finite: vertex_normals) a NORMAL fp32 VEC3
    accessor is added, its buffer view appended after the others; without them the file is what it always was, byte for byte.
    One buffer, every chunk and buffer view 4-byte aligned.  Tensors are copied to the host.  Returns the file length."""
    v = np.ascontiguousarray(_host(vertices), dtype="<f4")
    c = _host(colors)
    if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] == 0:
        raise ValueError("write_glb: vertices %s must be [V, 3] with V >= 1 (a glTF accessor cannot be empty)" % (v.shape,))
    if c.dtype != np.uint8 or c.ndim != 2 or c.shape[1] not in (3, 4):
        raise ValueError("write_glb: colors must be uint8 [V, 3] or [V, 4], got %s %s" % (c.dtype, c.shape))
    if c.shape[0] != v.shape[0]:
        raise ValueError("write_glb: mismatched lengths: %d vertices, %d colours" % (v.shape[0], c.shape[0]))
    if c.shape[1] == 3:
        c = np.concatenate([c, np.full((len(c), 1), 255, np.uint8)], axis=1)
    c = np.ascontiguousarray(c)
    if not np.isfinite(v).all():
        raise ValueError("write_glb: non-finite vertex position")
    lo, hi = (v.min(0), v.max(0)) if bounds is None else np.asarray(bounds, np.float32).reshape(2, 3)
    views = [dict(buffer=0, byteOffset=0, byteLength=v.nbytes, target=34962),
             dict(buffer=0, byteOffset=v.nbytes, byteLength=c.nbytes, target=34962)]
    accessors = [dict(bufferView=0, componentType=5126, count=len(v), type="VEC3", min=[float(x) for x in lo], max=[float(x) for x in hi]),
                 dict(bufferView=1, componentType=5121, normalized=True, count=len(v), type="VEC4")]
    chunks = [v.tobytes(), c.tobytes()]
    prim = dict(attributes=dict(POSITION=0, COLOR_0=1), mode=0)
    doc = dict(asset=dict(version="2.0", generator="spann3r_amd.mesh"), scene=0, scenes=[dict(nodes=[0])], nodes=[dict(mesh=0)])
    if faces is not None:
        f = _host(faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] == 0:
            raise ValueError("write_glb: faces %s must be [F, 3] with F >= 1" % (f.shape,))
        if f.min() < 0 or f.max() >= len(v):
            raise ValueError("write_glb: face index outside 0..%d" % (len(v) - 1))
        f = np.ascontiguousarray(f, dtype="<u4")
        views.append(dict(buffer=0, byteOffset=v.nbytes + c.nbytes, byteLength=f.nbytes, target=34963))
        accessors.append(dict(bufferView=2, componentType=5125, count=f.size, type="SCALAR"))
        chunks.append(f.tobytes())
        prim.update(indices=2, mode=4, material=0)
        doc["materials"] = [dict(doubleSided=True, pbrMetallicRoughness=dict(metallicFactor=0.0, roughnessFactor=1.0))]
    if normals is not None:
        nrm = np.ascontiguousarray(_host(normals), dtype="<f4")
        if nrm.shape != v.shape:
            raise ValueError("write_glb: normals %s must match the vertices %s" % (nrm.shape, v.shape))
        if not np.isfinite(nrm).all():
            raise ValueError("write_glb: non-finite vertex normal")
        views.append(dict(buffer=0, byteOffset=sum(len(ch) for ch in chunks), byteLength=nrm.nbytes, target=34962))
        accessors.append(dict(bufferView=len(views) - 1, componentType=5126, count=len(nrm), type="VEC3"))
        chunks.append(nrm.tobytes())
        prim["attributes"]["NORMAL"] = len(accessors) - 1
    binary = b"".join(chunks)                          # (12 V + 4 V + 12 F bytes: every view starts and ends on a multiple of 4)
    doc.update(meshes=[dict(primitives=[prim])], buffers=[dict(byteLength=len(binary))], bufferViews=views, accessors=accessors)
    text = json.dumps(doc, separators=(",", ":")).encode()
    text += b" " * (-len(text) % 4)
    binary += b"\0" * (-len(binary) % 4)
    total = 12 + 8 + len(text) + 8 + len(binary)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<4sII", b"glTF", 2, total))
        fh.write(struct.pack("<I4s", len(text), b"JSON"))
        fh.write(text)
        fh.write(struct.pack("<I4s", len(binary), b"BIN\0"))
        fh.write(binary)
    return total


def sequence_tensors(preds, batch):
    """model.forward's outputs as app.py:132-144 stacks them: pts_all [t, h, w, 3] (unscaled), images_all in [0, 1], conf_all [t, h, w]"""
    pts_all = torch.cat([p["pts3d" if j == 0 else "pts3d_in_other_view"] for j, p in enumerate(preds)]).float()
    conf_all = torch.cat([p["conf"] for p in preds]).float()
    images_all = (torch.cat([v["img"] for v in batch]).to(pts_all.device).permute(0, 2, 3, 1).float() + 1.0) / 2.0
    if images_all.shape[1:3] != pts_all.shape[1:3]:
        images_all = images_all.swapaxes(1, 2)                                    # portrait frames were rectified to landscape
    return pts_all, images_all, conf_all


def export_glb(path, preds, batch, conf_thresh=1e-3, as_pointcloud=False):
    """app.py:132-171: the GLB of a reconstruction from model.forward's `preds` and its `batch`.  -> dict(vertices, faces, bytes)."""
    pts_all, images_all, conf_all = sequence_tensors(preds, batch)
    scene = scene_mesh(pts_all, images_all, conf_all, conf_thresh, as_pointcloud)
    nv, nf = scene["vertices"].shape[0], 0 if scene["faces"] is None else scene["faces"].shape[0]
    if nv == 0 or (not as_pointcloud and nf == 0):
        raise RuntimeError("export_glb: nothing passes conf_thresh %g: no %s to write" % (conf_thresh, "point" if as_pointcloud else "face"))
    size = write_glb(path, scene["vertices"], scene["colors"], scene["faces"], bounds=scene["bounds"])
    return dict(vertices=nv, faces=nf, bytes=size)
