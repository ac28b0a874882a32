"""Numpy restatement of the rules of include/spann3r_hip.h, "Pointmap meshes": the face list (sp3_mesh_faces), the vertex compaction
(sp3_mesh_compact_vertices) and the triangle rasteriser (sp3_render_tris).  It is the pin of spann3r_amd.mesh and of
PointRenderer.add_mesh in tests/test_mesh_gpu.py; the face list is itself checked against the reference's own output
(tests/golden/mesh_faces.npz) in tests/test_mesh_cpu.py.  The rasteriser is a restatement of its own rule, not of any viewer.

The rasteriser runs in float64 by default; with dtype=np.float32 every operation is rounded to fp32 in the header's order, which is
how the tests measure what the number format alone costs in depth."""
import numpy as np


# ------------------------------------------------------------------------------------------------ faces
def faces_ref(valid, both_windings=True):
    """valid bool [t, h, w] -> (faces int64 [F, 3] of global vertex indices, colour_px int64 [F], counts [1 + blocks * t])"""
    valid = np.asarray(valid, bool)
    t, h, w = valid.shape
    idx = np.arange(h * w).reshape(h, w)
    tl, tr, bl, br = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    blocks = [(np.c_[tl, tr, bl], tl), (np.c_[bl, tr, tl], tl), (np.c_[tr, bl, br], br), (np.c_[br, bl, tr], br)]
    if not both_windings:
        blocks = [blocks[0], blocks[2]]
    faces, colour, counts = [], [], []
    for f in range(t):
        v = valid[f].ravel()
        for fc, col in blocks:
            keep = v[fc].all(axis=1) if len(fc) else np.zeros(0, bool)
            faces.append(fc[keep] + f * h * w)
            colour.append(col[keep] + f * h * w)
            counts.append(int(keep.sum()))
    faces = np.concatenate(faces).reshape(-1, 3).astype(np.int64)
    return faces, np.concatenate(colour).astype(np.int64), [len(faces)] + counts


def conf_valid(conf, conf_thresh):
    """(c - 1) / c > conf_thresh in fp32"""
    c = np.asarray(conf, np.float32)
    with np.errstate(all="ignore"):
        return (c - np.float32(1)) / c > np.float32(conf_thresh)


# ------------------------------------------------------------------------------------------------ vertices
def transform_ref(pts, scale, transform):
    """fp32 [n, 3]: M (scale * x), every operation rounded to fp32, ((m0 x + m1 y) + m2 z) + m3 per row"""
    p = np.asarray(pts, np.float32).reshape(-1, 3) * np.float32(scale)
    m = np.asarray(transform, np.float32).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], axis=1).astype(np.float32)


def compact_ref(pts, faces=None, keep=None, scale=1.0, transform=np.eye(4)):
    """-> (positions fp32 [V, 3], kept vertex indices int64 [V], remapped faces or None, bounds [2, 3]).  The kept set is what the
    faces reference, or `keep` (bool [n]) for a cloud."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    if faces is not None:
        keep = np.zeros(len(pts), bool)
        keep[np.asarray(faces).ravel()] = True
    keep = np.asarray(keep, bool).ravel()
    kept = np.flatnonzero(keep)
    remap = np.full(len(pts), -1, np.int64)
    remap[kept] = np.arange(len(kept))
    pos = transform_ref(pts[kept], scale, transform)
    bounds = np.stack([pos.min(0), pos.max(0)]) if len(pos) else np.array([[np.inf] * 3, [-np.inf] * 3], np.float32)
    return pos, kept, None if faces is None else remap[np.asarray(faces)], bounds


# ------------------------------------------------------------------------------------------------ rasteriser
def project(pts, cam, dtype=np.float64):
    """sp3_render_splat's projection in `dtype`, the header's order -> (u, v, z, ok).  cam: tests/render_ref.Cam"""
    X = np.asarray(pts, dtype).reshape(-1, 3)
    R, t = cam.R.astype(dtype), cam.t.astype(dtype)
    fx, fy, cx, cy = (dtype(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy))
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(all="ignore"):
        xc = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + t[0]
        yc = ((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + t[1]
        zc = ((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + t[2]
        ok = np.isfinite(X).all(1) & np.isfinite(xc) & np.isfinite(yc) & np.isfinite(zc)
        ok &= np.where(ok, zc, 0) > dtype(cam.z_near)
        zs = np.where(ok, zc, 1)
        u = fx * xc / zs + cx
        v = fy * yc / zs + cy
    return u, v, zc, ok


def snap(u, v, ok):
    """-> (X, Y int64 in 1/16 pixel, ok): floor(16 c + 0.5), culled outside +-2^20"""
    dt = u.dtype.type
    with np.errstate(all="ignore"):
        sx, sy = np.floor(dt(16) * u + dt(0.5)), np.floor(dt(16) * v + dt(0.5))
        lim = 2.0 ** 20
        ok = ok & (sx >= -lim) & (sx <= lim) & (sy >= -lim) & (sy <= lim)
    return np.where(ok, sx, 0).astype(np.int64), np.where(ok, sy, 0).astype(np.int64), ok


def snap_boundary_distance(pts, cam):
    """per projected vertex, the distance in 1/16 pixel of its float64 coordinates from the nearest snapping boundary (k + 0.5) / 16;
    inf where culled"""
    u, v, _, ok = project(pts, cam)
    d = np.full(len(u), np.inf)
    for c in (u, v):
        fr = 16 * c[ok] + 0.5 - np.floor(16 * c[ok] + 0.5)
        d[ok] = np.minimum(d[ok], np.minimum(fr, 1 - fr))
    return d


def _top_left(dx, dy):
    return dy < 0 or (dy == 0 and dx > 0)


def raster(pts, faces, colour_px, cam, max_bbox_px=4096, dtype=np.float64, index_base=0):
    """-> (index int64 [H, W] (-1: empty), depth `dtype` [H, W] (+inf: empty), culled_big).  Nearest wins, then the lowest index."""
    dt = dtype
    u, v, z, ok = project(pts, cam, dt)
    X, Y, ok = snap(u, v, ok)
    H, W = cam.height, cam.width
    index = np.full((H, W), -1, np.int64)
    depth = np.full((H, W), np.inf, dt)
    culled_big = 0
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    for i, (a, b, c) in enumerate(faces):
        col = int(a if colour_px is None else colour_px[i])
        if not (ok[a] and ok[b] and ok[c]):
            continue
        area = int((X[b] - X[a]) * (Y[c] - Y[a]) - (X[c] - X[a]) * (Y[b] - Y[a]))
        if area == 0:
            continue
        if area < 0:
            b, c, area = c, b, -area
        xs, ys = [int(X[a]), int(X[b]), int(X[c])], [int(Y[a]), int(Y[b]), int(Y[c])]
        px0, px1 = max(-(-min(xs) // 16), 0), min(max(xs) // 16, W - 1)
        py0, py1 = max(-(-min(ys) // 16), 0), min(max(ys) // 16, H - 1)
        if px0 > px1 or py0 > py1:
            continue
        if (px1 - px0 + 1) * (py1 - py0 + 1) > max_bbox_px:
            culled_big += 1
            continue
        edges = [(1, 2), (2, 0), (0, 1)]
        iz = [dt(1) / dt(z[k]) for k in (a, b, c)]
        for py in range(py0, py1 + 1):
            for px in range(px0, px1 + 1):
                e = []
                for p, q in edges:
                    dx, dy = xs[q] - xs[p], ys[q] - ys[p]
                    ev = dx * (16 * py - ys[p]) - dy * (16 * px - xs[p])
                    e.append(ev if ev > 0 or (ev == 0 and _top_left(dx, dy)) else None)
                if None in e:
                    continue
                with np.errstate(all="ignore"):
                    s = (dt(e[0]) * iz[0] + dt(e[1]) * iz[1]) + dt(e[2]) * iz[2]
                    d = dt(area) / s
                if not np.isfinite(d):
                    continue
                g = index_base + col
                if d < depth[py, px] or (d == depth[py, px] and g < index[py, px]):
                    depth[py, px], index[py, px] = d, g
    return index, depth, culled_big


def merge(layers):
    """[(index, depth), ...] of one image size -> the (index, depth) of all in one buffer: nearest, then lowest index"""
    index, depth = (np.array(x) for x in layers[0])
    for i2, d2 in layers[1:]:
        take = (d2 < depth) | ((d2 == depth) & (i2 >= 0) & ((index < 0) | (i2 < index)))
        index, depth = np.where(take, i2, index), np.where(take, d2, depth)
    return index, depth
