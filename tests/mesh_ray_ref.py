"""The rule of include/spann3r_hip.h "Mesh rays" in plain numpy: the anchor of every device comparison in
tests/test_mesh_ray_gpu.py, itself checked in tests/test_mesh_ray_cpu.py against a pair-by-pair loop over Python floats (bit for
bit) and against a second formulation in exact rationals (fractions.Fraction: Moeller-Trumbore on the fp32 inputs).  pyrender,
trimesh and Embree are not available: parity with them is unpinned.

The rule.  vertices fp32 [V, 3], faces int32 [F, 3]; a ray is o fp32 [3], d fp32 [3] (not normalised) and 0 <= t_min <= t_max;
everything is converted to fp64 and every operation is rounded on its own (numpy's elementwise ufuncs do not fuse).
1. A ray with a non-finite component, or d = 0, hits nothing.
2. A face is usable as in mesh_distance_ref.usable.
3. Woop, Benthin and Wald's watertight test: kz = the axis of the largest |d| (the lowest among equals), kx = kz + 1, ky = kx + 1
   cyclic, swapped when d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]; per vertex P = vertex - o,
   X = P[kx] - Sx P[kz], Y = P[ky] - Sy P[kz], Z = Sz P[kz]; U = Xc Yb - Yc Xb, V = Xa Yc - Ya Xc, W = Xb Ya - Yb Xa; a miss when one
   of U, V, W is < 0 and one is > 0; det = (U + V) + W, a miss when det == 0; T = (U Za + V Zb) + W Zc, t = T / det, -0 stored as +0;
   a hit when t_min <= t <= t_max.  side = 0 (front: the origin sees A, B, C counter-clockwise) when det > 0, 1 when det < 0;
   cull "back" drops side 1, "front" side 0.
4. Per ray the lexicographic minimum of (t, face index) over the hits, from (+inf, none) with a strict <; NaN and +inf never win.
   t fp32, face int32, bary fp32 = (U, V, W) / det, point fp32 = o + t d (a product, a sum), side uint8; a miss: +inf, -1, 0, o, 255.

The camera rule of mesh.render_depth_maps (sp3_mesh_ray_views): pixel (u, v), x = ((u + off) - cx) / fx, y = ((v + off) - cy) / fy in
fp64 from the fp32 intrinsics, d_i = fp32((R_i0 x + R_i1 y) + R_i2) from the fp32 cam2world, o = its translation column."""
import math
from fractions import Fraction

import numpy as np

import mesh_distance_ref as DR

MISS_SIDE = 255
CULL = {None: 0, "back": 1, "front": 2}

usable = DR.usable


def ray_frame(o, d):
    """o, d fp64 [..., 3] -> dict(ok bool [...], kx, ky, kz int [...], Sx, Sy, Sz fp64 [...])"""
    with np.errstate(all="ignore"):
        ok = np.isfinite(o).all(-1) & np.isfinite(d).all(-1) & (d != 0).any(-1)
        kz = np.argmax(np.abs(np.where(np.isnan(d), 0.0, d)), -1)          # the first maximum: the lowest axis among equals
        kx, ky = (kz + 1) % 3, (kz + 2) % 3
        take = lambda x, k: np.take_along_axis(x, k[..., None], -1)[..., 0]
        dz = take(d, kz)
        kx, ky = np.where(dz < 0, ky, kx), np.where(dz < 0, kx, ky)
        return dict(ok=ok, kx=kx, ky=ky, kz=kz, Sx=take(d, kx) / dz, Sy=take(d, ky) / dz, Sz=1.0 / dz)


def hit_pairs(o, d, a, b, c, t_min=0.0, t_max=math.inf, cull=None):
    """elementwise over broadcastable fp64 [..., 3] arrays (o, d must carry every leading axis of the result or broadcast to it)
    -> dict(hit bool [...], t, U, V, W, det fp64 [...])"""
    o, d, a, b, c = (np.asarray(x, np.float64) for x in (o, d, a, b, c))
    full = np.broadcast_shapes(o.shape, d.shape, a.shape, b.shape, c.shape)
    o, d = np.broadcast_to(o, full), np.broadcast_to(d, full)
    fr = ray_frame(o, d)
    with np.errstate(all="ignore"):
        X, Y, Z = [], [], []
        for vtx in (a, b, c):
            P = np.broadcast_to(vtx, full) - o
            pk = lambda k: np.take_along_axis(P, k[..., None], -1)[..., 0]
            px, py, pz = pk(fr["kx"]), pk(fr["ky"]), pk(fr["kz"])
            X.append(px - fr["Sx"] * pz)
            Y.append(py - fr["Sy"] * pz)
            Z.append(fr["Sz"] * pz)
        U = X[2] * Y[1] - Y[2] * X[1]
        V = X[0] * Y[2] - Y[0] * X[2]
        W = X[1] * Y[0] - Y[1] * X[0]
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        T = (U * Z[0] + V * Z[1]) + W * Z[2]
        t = T / det
        t = np.where(t == 0, 0.0, t)
        hit = fr["ok"] & ~mixed & (det != 0) & (t_min <= t) & (t <= t_max)
        if CULL[cull] == 1:
            hit &= ~(det < 0)
        elif CULL[cull] == 2:
            hit &= ~(det > 0)
    return dict(hit=hit, t=t, U=U, V=V, W=W, det=det)


def hit_pair_loop(o, d, a, b, c, t_min=0.0, t_max=math.inf):
    """one pair, Python floats (IEEE doubles, one rounding per operation), the rule read top to bottom -> (hit, t, (U, V, W), det)"""
    o, d, a, b, c = ([float(np.float64(v)) for v in x] for x in (o, d, a, b, c))
    div = lambda x, y: x / y if y != 0 else (math.nan if x == 0 or x != x else math.copysign(math.inf, x) * math.copysign(1.0, y))
    if not all(math.isfinite(v) for v in o + d) or d == [0.0, 0.0, 0.0]:
        return False, math.nan, (math.nan,) * 3, math.nan
    kz = 0
    if abs(d[1]) > abs(d[0]):
        kz = 1
    if abs(d[2]) > max(abs(d[0]), abs(d[1])):
        kz = 2
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    if d[kz] < 0:
        kx, ky = ky, kx
    Sx, Sy, Sz = div(d[kx], d[kz]), div(d[ky], d[kz]), div(1.0, d[kz])
    X, Y, Z = [], [], []
    for vtx in (a, b, c):
        P = [vtx[k] - o[k] for k in range(3)]
        X.append(P[kx] - Sx * P[kz])
        Y.append(P[ky] - Sy * P[kz])
        Z.append(Sz * P[kz])
    U = X[2] * Y[1] - Y[2] * X[1]
    V = X[0] * Y[2] - Y[0] * X[2]
    W = X[1] * Y[0] - Y[1] * X[0]
    if (U < 0 or V < 0 or W < 0) and (U > 0 or V > 0 or W > 0):
        return False, math.nan, (U, V, W), math.nan
    det = (U + V) + W
    if det == 0:
        return False, math.nan, (U, V, W), det
    T = (U * Z[0] + V * Z[1]) + W * Z[2]
    t = div(T, det)
    if t == 0:
        t = 0.0
    return bool(t_min <= t <= t_max), t, (U, V, W), det


def exact_hit(o, d, a, b, c):
    """Moeller-Trumbore for one pair in exact rationals on the fp32 inputs: a second formulation, no rounding at all.
    -> (t, (wa, wb, wc)) as Fractions, the barycentric weights of A, B, C (any sign), or None when the ray is parallel to the plane"""
    O, D, A, B, C = ([Fraction(float(v)) for v in x] for x in (o, d, a, b, c))
    sub = lambda u, v: [u[0] - v[0], u[1] - v[1], u[2] - v[2]]
    dot = lambda u, v: u[0] * v[0] + u[1] * v[1] + u[2] * v[2]
    cross = lambda u, v: [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    e1, e2 = sub(B, A), sub(C, A)
    pv = cross(D, e2)
    den = dot(e1, pv)
    if den == 0:
        return None
    tv = sub(O, A)
    u = dot(tv, pv) / den
    qv = cross(tv, e1)
    v = dot(D, qv) / den
    return dot(e2, qv) / den, (1 - u - v, u, v)


def intersect(origins, directions, vertices, faces, t_min=0.0, t_max=math.inf, cull=None, chunk=256):
    """-> dict(t fp32 [N], face int32 [N], bary fp32 [N, 3], point fp32 [N, 3], side uint8 [N], t64 fp64 [N] (+inf: a miss))"""
    o32 = np.asarray(origins, np.float32).reshape(-1, 3)
    d32 = np.asarray(directions, np.float32).reshape(-1, 3)
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    use = np.flatnonzero(usable(vertices, faces))
    n = len(o32)
    out = dict(t=np.full(n, np.inf, np.float32), face=np.full(n, -1, np.int32), bary=np.zeros((n, 3), np.float32), point=o32.copy(),
               side=np.full(n, MISS_SIDE, np.uint8), t64=np.full(n, np.inf))
    if n == 0 or len(use) == 0:
        return out
    a, b, c = (v[f[use, k]][None] for k in range(3))
    for s in range(0, n, chunk):
        o = o32[s:s + chunk].astype(np.float64)[:, None]
        d = d32[s:s + chunk].astype(np.float64)[:, None]
        r = hit_pairs(o, d, a, b, c, t_min, t_max, cull)
        t = np.where(r["hit"], r["t"], np.inf)
        j = np.argmin(t, 1)                                       # the first minimum: the smallest index (use ascends)
        rows = np.arange(len(j))
        best = t[rows, j]
        won = best < np.inf
        w, rw, jw = s + rows[won], rows[won], j[won]
        with np.errstate(all="ignore"):
            det = r["det"][rw, jw]
            out["t64"][w] = best[won]
            out["t"][w] = best[won].astype(np.float32)
            out["face"][w] = use[jw].astype(np.int32)
            out["bary"][w] = np.stack([r[k][rw, jw] / det for k in "UVW"], 1).astype(np.float32)
            out["point"][w] = (o[rw, 0] + best[won][:, None] * d[rw, 0]).astype(np.float32)
            out["side"][w] = np.where(det > 0, 0, 1).astype(np.uint8)
    return out


def camera_rays(intrinsics, cam2world, size, pixel_offset=0.0):
    """one camera: intrinsics [3, 3], cam2world [4, 4] (rounded to fp32 first, as the descriptor holds them), size = (h, w)
    -> (origins fp32 [h w, 3], directions fp32 [h w, 3]), row-major over the pixels"""
    K = np.asarray(intrinsics, np.float64).astype(np.float32).astype(np.float64)
    P = np.asarray(cam2world, np.float64).astype(np.float32).astype(np.float64)
    h, w = size
    off = float(np.float32(pixel_offset))
    vv, uu = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    x = ((uu + off) - K[0, 2]) / K[0, 0]
    y = ((vv + off) - K[1, 2]) / K[1, 1]
    d = np.stack([((P[i, 0] * x + P[i, 1] * y) + P[i, 2]).astype(np.float32) for i in range(3)], -1).reshape(-1, 3)
    o = np.broadcast_to(P[:3, 3].astype(np.float32), d.shape).copy()
    return o, d


# ------------------------------------------------------------------------------------------------ scenes the tests share
def icosphere(level=3):
    """the unit icosphere by midpoint subdivision -> (vertices fp32 [V, 3], faces int32 [F, 3]): level 3 = 642 vertices, 1 280 faces,
    counter-clockwise seen from outside"""
    p = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    v = [tuple(np.asarray(x, np.float64) / np.linalg.norm(x)) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = (np.asarray(v[i]) + np.asarray(v[j])) / 2.0
                v.append(tuple(m / np.linalg.norm(m)))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def sphere_rays(verts, faces, origin, n_random=2048, seed=3):
    """directions fp32 from `origin` through every vertex, every fp32 edge midpoint, every fp32 centroid, and n_random random ones"""
    v = verts.astype(np.float32)
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e = np.unique(np.sort(e, 1), axis=0)
    mid = ((v[e[:, 0]] + v[e[:, 1]]) * np.float32(0.5)).astype(np.float32)
    cen = ((v[faces[:, 0]] + v[faces[:, 1]] + v[faces[:, 2]]) / np.float32(3)).astype(np.float32)
    rnd = np.random.default_rng(seed).normal(size=(n_random, 3)).astype(np.float32)
    o = np.asarray(origin, np.float32)
    d = np.concatenate([v - o, mid - o, cen - o, rnd]).astype(np.float32)
    return np.broadcast_to(o, d.shape).copy(), d


SPHERE_ORIGINS = ((0.0, 0.0, 0.0), (0.3, -0.2, 0.1))


def sphere_radial_bounds(verts, faces):
    """every point of the level-3 icosphere lies at a radius in [sqrt(r_min^2 - e_max^2 / 3), r_max]: the [1 - s, max |v|] of the
    distance test's sphere bound (tests/test_mesh_distance_gpu.py), the fp32 rounding of the vertices written in"""
    v64 = verts.astype(np.float64)
    edges = np.concatenate([v64[faces[:, i]] - v64[faces[:, (i + 1) % 3]] for i in range(3)])
    e_max = np.linalg.norm(edges, axis=1).max()
    rv = np.linalg.norm(v64, axis=1)
    return math.sqrt(rv.min() ** 2 - e_max ** 2 / 3), rv.max()


def plane(n=9, z=2.0, half=1.5):
    """the plane z = `z` over [-half, half]^2 as an n x n grid of vertices, 2 (n - 1)^2 faces, counter-clockwise seen from above (the
    normal is +z) -> (vertices fp32, faces int32)"""
    xs = np.linspace(-half, half, n).astype(np.float32)
    yy, xx = np.meshgrid(xs, xs, indexing="ij")
    v = np.stack([xx, yy, np.full_like(xx, z)], -1).reshape(-1, 3).astype(np.float32)
    tl = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None]).reshape(-1)
    return v, np.concatenate([np.stack([tl, tl + 1, tl + n], 1), np.stack([tl + 1, tl + n + 1, tl + n], 1)]).astype(np.int32)


def bumpy_sheet(n=32):
    """the n x n bumpy sheet of tests/test_mesh_distance_gpu.py, rebuilt -> (vertices fp32 [n n, 3], faces int32 [2 (n - 1)^2, 3])"""
    y, x = np.mgrid[:n, :n]
    verts = np.stack([x / (n - 1) + 0.003, y / (n - 1) - 0.5, 0.05 * np.sin(x * 0.9) * np.cos(y * 0.7)], -1).reshape(-1, 3).astype(np.float32)
    tl = (y[:-1, :-1] * n + x[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([tl, tl + 1, tl + n], 1), np.stack([tl + 1, tl + n + 1, tl + n], 1)]).astype(np.int32)
    return verts, faces
