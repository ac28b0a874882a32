"""The rule of include/spann3r_hip.h "Mesh visibility" in plain numpy: the anchor of every device comparison in
tests/test_mesh_visibility_gpu.py, itself checked on hand-built scenes in tests/test_mesh_visibility_cpu.py.  Open3D, trimesh and the
NICE-SLAM cull_mesh script are not available: parity with them is unpinned.

The rule.
1. A ray (o, d, t_min, t_max, cull) is OCCLUDED iff some usable face is a hit by rule 3 of "Mesh rays": mesh_ray_ref.intersect(...)
   ["face"] >= 0.  (`occluded` below takes a range per ray, which intersect does not: it asks mesh_ray_ref.hit_pairs, the function
   intersect is built on, whether any usable face hits; the CPU tests check the two against each other.)
2. A view holds w, h, fu, fv, cu, cv, near, far, c2w[12] and w2c[12], all fp32; w2c is the fp64 inverse of the pose rounded to fp32.
   For a point p fp32 [3], everything in fp64 from the fp32 fields, every operation rounded on its own:
     x = ((W00 p0 + W01 p1) + W02 p2) + W03, y, z likewise;   in range: z > 0 and near <= z <= far;
     u = (x / z) fu + cu, v = (y / z) fv + cv;   in the image: 0 <= (u - pixel_offset) + 0.5 < w, 0 <= (v - pixel_offset) + 0.5 < h;
     the shadow ray: o = the translation of c2w, d = fp32(p - o), t_min = near / z, t_max = 1 - bias (bias fp32 in [0, 1));
   visible = in range, in the image, not occluded.  A non-finite p is visible from nowhere.
3. count [N] = the views that see the point; mask [T, N].
4. A vertex is seen iff count >= min_views; a face is kept iff its indices lie in 0..V-1 and one ("any") or all three ("all") of its
   vertices are seen; kept faces stay in order and rotation; the vertices nothing names are dropped, the others keep their order."""
import math

import numpy as np

import mesh_ray_ref as R


def make_views(intrinsics, cam2world, size, near=0.0, far=math.inf, opengl=False):
    """intrinsics [3, 3] or [T, 3, 3], cam2world [4, 4] or [T, 4, 4], size = (h, w) -> a list of T views as the descriptor holds
    them: dict(w, h, fu, fv, cu, cv, near, far fp32 scalars; c2w, w2c fp32 [12])"""
    P = np.asarray(cam2world, np.float64)
    P = P[None] if P.ndim == 2 else P
    K = np.asarray(intrinsics, np.float64)
    K = np.broadcast_to(K, (len(P), 3, 3))
    if opengl:
        P = P * np.array([1.0, -1.0, -1.0, 1.0])
    h, w = size
    f32 = np.float32
    inv = np.linalg.inv(P) if len(P) else P
    return [dict(w=int(w), h=int(h), fu=f32(K[i, 0, 0]), fv=f32(K[i, 1, 1]), cu=f32(K[i, 0, 2]), cv=f32(K[i, 1, 2]), near=f32(near), far=f32(far),
                 c2w=P[i, :3].reshape(12).astype(f32), w2c=inv[i, :3].reshape(12).astype(f32)) for i in range(len(P))]


def project(points, view, pixel_offset=0.0):
    """points fp32 [N, 3] -> dict(z, u, v fp64 [N], in_range, in_image, finite bool [N])"""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    W = view["w2c"].astype(np.float64).reshape(3, 4)
    off = float(np.float32(pixel_offset))
    with np.errstate(all="ignore"):
        x, y, z = (((W[i, 0] * p[:, 0] + W[i, 1] * p[:, 1]) + W[i, 2] * p[:, 2]) + W[i, 3] for i in range(3))
        in_range = (z > 0) & (float(view["near"]) <= z) & (z <= float(view["far"]))
        u = (x / z) * float(view["fu"]) + float(view["cu"])
        v = (y / z) * float(view["fv"]) + float(view["cv"])
        su, sv = (u - off) + 0.5, (v - off) + 0.5
        in_image = (su >= 0) & (su < view["w"]) & (sv >= 0) & (sv < view["h"])
    return dict(z=z, u=u, v=v, in_range=in_range, in_image=in_image, finite=np.isfinite(p).all(1))


def shadow_rays(points, view, z, bias):
    """-> (origins fp32 [N, 3], directions fp32 [N, 3], t_min fp64 [N], t_max float)"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    o = np.broadcast_to(view["c2w"].reshape(3, 4)[:, 3].astype(np.float32), p.shape).copy()
    with np.errstate(all="ignore"):
        d = (p.astype(np.float64) - o.astype(np.float64)).astype(np.float32)
        t_min = float(view["near"]) / z
    return o, d, t_min, 1.0 - float(np.float32(bias))


def occluded(origins, directions, vertices, faces, t_min=0.0, t_max=math.inf, cull=None, chunk=256):
    """rule 1 -> bool [N].  t_min, t_max: scalars (then exactly mesh_ray_ref.intersect(...)["face"] >= 0) or one per ray."""
    o32 = np.asarray(origins, np.float32).reshape(-1, 3)
    d32 = np.asarray(directions, np.float32).reshape(-1, 3)
    if np.ndim(t_min) == 0 and np.ndim(t_max) == 0:
        if not float(t_min) <= float(t_max):
            return np.zeros(len(o32), bool)
        return R.intersect(o32, d32, vertices, faces, t_min=float(t_min), t_max=float(t_max), cull=cull)["face"] >= 0
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    use = np.flatnonzero(R.usable(vertices, faces))
    out = np.zeros(len(o32), bool)
    if len(o32) == 0 or len(use) == 0:
        return out
    a, b, c = (v[f[use, k]][None] for k in range(3))
    lo = np.broadcast_to(np.asarray(t_min, np.float64), (len(o32),))
    hi = np.broadcast_to(np.asarray(t_max, np.float64), (len(o32),))
    for s in range(0, len(o32), chunk):
        r = R.hit_pairs(o32[s:s + chunk].astype(np.float64)[:, None], d32[s:s + chunk].astype(np.float64)[:, None], a, b, c,
                        lo[s:s + chunk, None], hi[s:s + chunk, None], cull)
        out[s:s + chunk] = r["hit"].any(1)
    return out


def point_visibility(points, vertices, faces, views, bias=1e-3, pixel_offset=0.0, cull=None):
    """rules 2 and 3 -> dict(count int32 [N], mask bool [T, N])"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    mask = np.zeros((len(views), len(p)), bool)
    for i, view in enumerate(views):
        pr = project(p, view, pixel_offset)
        cand = np.flatnonzero(pr["finite"] & pr["in_range"] & pr["in_image"])
        if len(cand) == 0:
            continue
        o, d, t_min, t_max = shadow_rays(p[cand], view, pr["z"][cand], bias)
        lo = 0.0 if float(view["near"]) == 0.0 else t_min          # (near = 0: one range for every ray, the route through intersect)
        mask[i, cand] = ~occluded(o, d, vertices, faces, lo, t_max, cull)
    return dict(count=mask.sum(0).astype(np.int32), mask=mask)


def cull_to_views(vertices, faces, count, mode="any", min_views=1):
    """rule 4 from the counts of the vertices -> dict(vertices fp32 [V', 3], faces int32 [K, 3] re-indexed, face_index int64 [K] (the
    kept faces of the input), vertex_index int64 [V'] (the kept vertices of the input))"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    seen = np.asarray(count) >= min_views
    valid = ((f >= 0) & (f < len(v))).all(1)
    s = seen[np.clip(f, 0, max(len(v) - 1, 0))] if len(v) else np.zeros(f.shape, bool)
    keep = valid & (s.all(1) if mode == "all" else s.any(1))
    fi = np.flatnonzero(keep)
    vi = np.unique(f[fi])
    remap = np.full(len(v), -1, np.int64)
    remap[vi] = np.arange(len(vi))
    return dict(vertices=v[vi], faces=remap[f[fi]].astype(np.int32).reshape(-1, 3), face_index=fi, vertex_index=vi)


# ------------------------------------------------------------------------------------------------ scenes the tests share
K32 = np.array([[10.0, 0, 15.5], [0, 10.0, 15.5], [0, 0, 1]])          # a 32 x 32 camera
SIZE32 = (32, 32)


def look_at(eye, target=(0.0, 0.0, 0.0)):
    """a cam2world [4, 4] at `eye` whose +z axis points at `target` (x right, y down: the package's camera frame)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, np.cross(z, x), z, eye
    return P


def two_triangles():
    """a small triangle in the plane z = 2 in front of a large one in z = 4, both with the normal +z, two cameras on the z axis
    facing each other (camera 0 at the origin looking down +z sees the backs, camera 1 at z = 6 looking down -z the fronts), and points
    before, between and behind them -> dict(vertices, faces, poses [2, 4, 4], points fp32 [5, 3], visible bool [2, 5] as geometry says)"""
    verts = np.array([(-1, -1, 2), (1, -1, 2), (0, 1, 2), (-3, -3, 4), (3, -3, 4), (0, 3, 4)], np.float32)
    faces = np.array([(0, 1, 2), (3, 4, 5)], np.int32)
    poses = np.stack([np.eye(4), np.diag([-1.0, 1.0, -1.0, 1.0])])
    poses[1, :3, 3] = (0, 0, 6)
    # on the axis before, between and behind both; off the axis between them, past the small triangle's shadow; on the large triangle
    points = np.array([(0, 0, 1), (0, 0, 3), (0, 0, 5), (2, -2, 3), (0, 0, 4)], np.float32)
    visible = np.array([[True, False, False, True, False],          # camera 0: the small triangle hides what lies behind it on the axis
                        [False, False, True, False, True]])         # camera 1: the large one hides everything below z = 4
    return dict(vertices=verts, faces=faces, poses=poses, points=points, visible=visible)


SPHERE_EYE = (1.7, -1.1, 2.2)                                          # one camera outside the unit icosphere, no symmetry
SPHERE_AXES = ((3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, -3, 0), (0, 0, 3), (0, 0, -3))
K64 = np.array([[40.0, 0, 31.5], [0, 40.0, 31.5], [0, 0, 1]])          # 64 x 64: the sphere fills half the image from 3 radii away
SIZE64 = (64, 64)


def facing(verts, faces, eye):
    """per face: +1 when `eye` lies on the side the normal points to (a front face of the icosphere), -1 on the other, fp64"""
    v = np.asarray(verts, np.float64)
    a, b, c = (v[faces[:, k]] for k in range(3))
    return np.sign(np.einsum("ij,ij->i", np.cross(b - a, c - a), np.asarray(eye, np.float64) - a))


def vertex_facing(verts, faces, eye):
    """-> (all_front bool [V], all_back bool [V]): every incident face of the vertex faces the eye / faces away"""
    s = facing(verts, faces, eye)
    front, back = np.ones(len(verts), bool), np.ones(len(verts), bool)
    for k in range(3):
        np.logical_and.at(front, faces[:, k], s > 0)
        np.logical_and.at(back, faces[:, k], s < 0)
    return front, back


BORDER_K = np.array([[8.0, 0, 4.0], [0, 8.0, 4.0], [0, 0, 1]])          # dyadic: u = 8 x / z + 4 is exact for the points below
BORDER_SIZE = (8, 8)
BORDER_NEAR, BORDER_FAR = 1.0, 2.0


def frustum_border(pixel_offset):
    """an identity camera of 8 x 8 pixels with near = 1, far = 2 and exact fp32 points on and around every border of its frustum; the
    only face lies far behind the far plane -> dict(vertices, faces, points fp32 [N, 3], visible bool [N])"""
    verts = np.array([(-50, -50, 100), (50, -50, 100), (0, 50, 100)], np.float32)
    faces = np.array([(0, 1, 2)], np.int32)
    lo, hi = (pixel_offset - 0.5 - 4.0) / 8.0, (8 + pixel_offset - 0.5 - 4.0) / 8.0      # x / z with u at the first and past the last border
    eps = 2.0 ** -20
    rows = [((lo, 0, 1), True), ((hi, 0, 1), False), ((lo - eps, 0, 1), False), ((hi - eps, 0, 1), True),
            ((0, lo, 1), True), ((0, hi, 1), False), ((0, lo - eps, 1), False), ((0, hi - eps, 1), True),
            ((2 * lo, 0, 2), True), ((2 * hi, 0, 2), False),                                      # the same borders at z = far
            ((0, 0, 1), True), ((0, 0, 2), True), ((0, 0, 1 - 2.0 ** -24), False), ((0, 0, 2 + 2.0 ** -22), False),      # z = near, z = far are in
            ((0, 0, 0), False), ((0, 0, -1.5), False),                                            # z <= 0
            ((np.nan, 0, 1.5), False), ((0, np.inf, 1.5), False), ((0, 0, np.inf), False), ((0, 0, -np.inf), False), ((0, 0, np.nan), False)]
    pts = np.array([r[0] for r in rows], np.float32)
    assert np.array_equal(pts.astype(np.float64), np.array([r[0] for r in rows], np.float64), equal_nan=True)      # exact fp32 inputs
    return dict(vertices=verts, faces=faces, points=pts, visible=np.array([r[1] for r in rows]))


def cases():
    """every scene of tests/test_mesh_visibility_cpu.py as arguments of point_visibility: a list of dict(name, vertices, faces, points,
    K, poses, size, kw) -- the device tests run the same list through the kernels"""
    tt = two_triangles()
    sv, sf = R.icosphere(3)
    out = []
    for cull in (None, "back", "front"):
        for bias in (1e-3, 0.0, 0.25):
            out.append(dict(name="two triangles, cull %s, bias %g" % (cull, bias), vertices=tt["vertices"], faces=tt["faces"],
                            points=np.concatenate([tt["points"], tt["vertices"]]), K=K32, poses=tt["poses"], size=SIZE32, kw=dict(cull=cull, bias=bias)))
    for off in (0.0, 0.5):
        fb = frustum_border(off)
        out.append(dict(name="frustum borders, offset %g" % off, vertices=fb["vertices"], faces=fb["faces"], points=fb["points"], K=BORDER_K,
                        poses=np.eye(4)[None], size=BORDER_SIZE, kw=dict(near=BORDER_NEAR, far=BORDER_FAR, pixel_offset=off)))
    out.append(dict(name="icosphere, one camera", vertices=sv, faces=sf, points=sv, K=K64, poses=look_at(SPHERE_EYE)[None], size=SIZE64, kw={}))
    out.append(dict(name="icosphere, six cameras", vertices=sv, faces=sf, points=sv, K=K64, poses=np.stack([look_at(e) for e in SPHERE_AXES]),
                    size=SIZE64, kw={}))
    return out


def run_case(c):
    """the restatement on one entry of cases() -> dict(count, mask)"""
    kw = dict(c["kw"])
    views = make_views(c["K"], c["poses"], c["size"], near=kw.pop("near", 0.0), far=kw.pop("far", math.inf), opengl=kw.pop("opengl", False))
    return point_visibility(c["points"], c["vertices"], c["faces"], views, **kw)
