"""The rule of include/spann3r_hip.h "Mesh distance" in plain numpy: the anchor of every device comparison in
tests/test_mesh_distance_gpu.py, itself checked in tests/test_mesh_distance_cpu.py against a pair-by-pair loop over Python floats
(bit for bit) and against a second formulation in exact rationals (fractions.Fraction: project onto the plane; inside, the plane
distance; outside, the nearest of the three clamped segment distances).  Open3D's RaycastingScene.compute_closest_points and
trimesh's ProximityQuery are not available: parity with them is unpinned.

The rule.  vertices fp32 [V, 3], faces int32 [F, 3], queries fp32 [Q, 3]; everything is converted to fp64 and every operation is
rounded on its own (numpy's elementwise ufuncs do not fuse); dot(u, v) = (ux vx + uy vy) + uz vz.
1. A face is usable when its three indices lie in 0..V-1 and the d of mesh_sample_ref.face_frames is > 0 (finite by its rule).
2. Closest point c of (A, B, C) to p (Ericson's Voronoi regions): ab = B - A, ac = C - A, ap = p - A, bp = p - B, cp = p - C,
   d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp),
   vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, e = d4 - d3, g = d5 - d6; the first test that holds decides:
     0 A   d1 <= 0 and d2 <= 0               c = A
     1 B   d3 >= 0 and d4 <= d3              c = B
     2 AB  vc <= 0 and d1 >= 0 and d3 <= 0   c = A + d1 / (d1 - d3) ab
     3 C   d6 >= 0 and d5 <= d6              c = C
     4 AC  vb <= 0 and d2 >= 0 and d6 <= 0   c = A + d2 / (d2 - d6) ac
     5 BC  va <= 0 and e >= 0 and g >= 0     c = B + e / (e + g) (C - B)
     6 inside, otherwise                     den = 1 / ((va + vb) + vc), c = A + (ab (vb den) + ac (vc den))
   and the squared distance is (dx dx + dy dy) + dz dz of p - c.
3. Per query the lexicographic minimum of (d2, face index) over the usable faces, from (+inf, none) with a strict <: the smallest
   index among equal d2; NaN and +inf never win.  dist = fp32(sqrt(d2)), closest = fp32(c), face int32, region uint8; no winner:
   +inf, the query itself, -1, 255."""
import math
from fractions import Fraction

import numpy as np

import mesh_sample_ref as SR

NO_REGION = 255


def usable(vertices, faces):
    """bool [F]: the d > 0 of the face frames (valid indices, finite, with an area)"""
    return SR.face_frames(vertices, faces)["d"] > 0


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def closest_pairs(p, a, b, c):
    """elementwise over broadcastable fp64 [..., 3] arrays -> (d2 fp64 [...], closest fp64 [..., 3], region uint8 [...])"""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e, g = d4 - d3, d5 - d6
        tests = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e >= 0) & (g >= 0)]
        region = np.full(np.broadcast(d1, d2).shape, 6, np.uint8)
        for r in range(5, -1, -1):
            region = np.where(tests[r], np.uint8(r), region)
        den = 1.0 / ((va + vb) + vc)
        s, t = (vb * den)[..., None], (vc * den)[..., None]
        full = np.broadcast_shapes(p.shape, a.shape, b.shape, c.shape)
        points = [np.broadcast_to(a, full), np.broadcast_to(b, full), a + (d1 / (d1 - d3))[..., None] * ab, np.broadcast_to(c, full),
                  a + (d2 / (d2 - d6))[..., None] * ac, b + (e / (e + g))[..., None] * (c - b), a + (ab * s + ac * t)]
        q = points[6]
        for r in range(5, -1, -1):
            q = np.where((region == r)[..., None], points[r], q)
        d = p - q
        dist2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return dist2, q, region


def closest_pair_loop(p, a, b, c):
    """one pair, Python floats (IEEE doubles, one rounding per operation), the rule read top to bottom -> (d2, (x, y, z), region)"""
    p, a, b, c = ([float(np.float64(v)) for v in x] for x in (p, a, b, c))
    sub = lambda u, v: [u[0] - v[0], u[1] - v[1], u[2] - v[2]]
    dot = lambda u, v: (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]
    div = lambda x, y: x / y if y != 0 else (math.nan if x == 0 or x != x else math.copysign(math.inf, x) * math.copysign(1.0, y))
    ab, ac, ap, bp, cp = sub(b, a), sub(c, a), sub(p, a), sub(p, b), sub(p, c)
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    e, g = d4 - d3, d5 - d6
    if d1 <= 0 and d2 <= 0:
        region, q = 0, a
    elif d3 >= 0 and d4 <= d3:
        region, q = 1, b
    elif vc <= 0 and d1 >= 0 and d3 <= 0:
        t = div(d1, d1 - d3)
        region, q = 2, [a[k] + t * ab[k] for k in range(3)]
    elif d6 >= 0 and d5 <= d6:
        region, q = 3, c
    elif vb <= 0 and d2 >= 0 and d6 <= 0:
        t = div(d2, d2 - d6)
        region, q = 4, [a[k] + t * ac[k] for k in range(3)]
    elif va <= 0 and e >= 0 and g >= 0:
        t = div(e, e + g)
        region, q = 5, [b[k] + t * (c[k] - b[k]) for k in range(3)]
    else:
        den = div(1.0, (va + vb) + vc)
        s, t = vb * den, vc * den
        region, q = 6, [a[k] + (ab[k] * s + ac[k] * t) for k in range(3)]
    d = sub(p, q)
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], tuple(q), region


def exact_d2(p, a, b, c):
    """the squared distance of one pair as a Fraction: a second formulation (plane projection, then segments), no rounding at all"""
    P, A, B, C = ([Fraction(float(v)) for v in x] for x in (p, a, b, c))
    sub = lambda u, v: [u[0] - v[0], u[1] - v[1], u[2] - v[2]]
    dot = lambda u, v: u[0] * v[0] + u[1] * v[1] + u[2] * v[2]
    cross = lambda u, v: [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
    ab, ac, ap = sub(B, A), sub(C, A), sub(P, A)
    n = cross(ab, ac)
    nn = dot(n, n)
    if nn != 0:
        h = dot(ap, n)
        foot = [P[k] - h / nn * n[k] for k in range(3)]
        # barycentric coordinates of the foot from signed sub-areas along n
        fa, fb, fc = sub(A, foot), sub(B, foot), sub(C, foot)
        u, v, w = dot(cross(fb, fc), n), dot(cross(fc, fa), n), dot(cross(fa, fb), n)
        if u >= 0 and v >= 0 and w >= 0:
            return h * h / nn

    def segment(X, Y):
        xy, xp = sub(Y, X), sub(P, X)
        ll = dot(xy, xy)
        t = Fraction(0) if ll == 0 else min(max(dot(xp, xy) / ll, Fraction(0)), Fraction(1))
        d = [xp[k] - t * xy[k] for k in range(3)]
        return dot(d, d)

    return min(segment(A, B), segment(B, C), segment(C, A))


def query(points, vertices, faces, chunk=256):
    """-> dict(dist fp32 [Q], closest fp32 [Q, 3], face int32 [Q], region uint8 [Q], d2 fp64 [Q] (+inf without a winner))"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    use = np.flatnonzero(usable(vertices, faces))
    n = len(pts)
    out = dict(dist=np.full(n, np.inf, np.float32), closest=pts.copy(), face=np.full(n, -1, np.int32), region=np.full(n, NO_REGION, np.uint8),
               d2=np.full(n, np.inf))
    if n == 0 or len(use) == 0:
        return out
    a, b, c = (v[f[use, k]][None] for k in range(3))
    for s in range(0, n, chunk):
        p = pts[s:s + chunk].astype(np.float64)[:, None]
        d2, q, region = closest_pairs(p, a, b, c)
        d2 = np.where(np.isnan(d2), np.inf, d2)
        j = np.argmin(d2, 1)                                      # the first minimum: the smallest index (use ascends)
        rows = np.arange(len(j))
        best = d2[rows, j]
        won = best < np.inf
        w = s + rows[won]
        out["d2"][w] = best[won]
        out["dist"][w] = np.sqrt(best[won]).astype(np.float32)
        out["closest"][w] = q[rows[won], j[won]].astype(np.float32)
        out["face"][w] = use[j[won]].astype(np.int32)
        out["region"][w] = region[rows[won], j[won]]
    return out
