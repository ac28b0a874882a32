"""Numpy restatement of the rules of include/spann3r_hip.h, "TSDF fusion": the integration of depth maps or world pointmaps into a
truncated signed distance volume (sp3_tsdf_integrate) and the marching-tetrahedra extraction of its zero level as a welded, indexed
mesh (sp3_tsdf_extract).  It is the pin of spann3r_amd.fusion in tests/test_fusion_gpu.py; tests/test_fusion_cpu.py checks the
restatement itself (closed oriented manifolds, Euler characteristic, interpolation error).  There is no reference implementation
of either stage: these are restatements of the header's own rules.

Both run in float64 by default; with dtype=np.float32 every operation is rounded to fp32 in the header's order, which is what the
kernels are compared with bit for bit.  No torch."""
import numpy as np

# ------------------------------------------------------------------------------------------------ the header's tables
TET = ((0, 1, 3, 7), (0, 5, 1, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 6, 4, 7))      # corner code = dx + 2 dy + 4 dz
SLOT_CODE = (1, 2, 4, 3, 6, 5, 7)                          # +x, +y, +z, +x+y, +y+z, +x+z, +x+y+z
SLOT_OF = {c: s for s, c in enumerate(SLOT_CODE)}


def _even(p):
    return sum(p[i] > p[j] for i in range(len(p)) for j in range(i + 1, len(p))) % 2 == 0


def tet_case(case):
    """the triangles of one tetrahedron, bit m of `case` = vertex m is inside: a list of triangles, each three edges (x, y) of
    tetrahedron vertex positions, by the header's rule"""
    ins = [m for m in range(4) if (case >> m) & 1]
    out = [m for m in range(4) if not (case >> m) & 1]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 2:
        (m, n), (q, r) = ins, out
        if not _even((m, n, q, r)):
            q, r = r, q
        return [[(m, q), (m, r), (n, r)], [(m, q), (n, r), (n, q)]]
    lone, (a, b, c) = (ins[0], out) if len(ins) == 1 else (out[0], ins)
    if not _even((lone, a, b, c)):
        b, c = c, b
    if len(ins) == 3:
        b, c = c, b
    return [[(lone, a), (lone, b), (lone, c)]]


CASES = [tet_case(c) for c in range(16)]


def corner_offset(code):
    return code & 1, (code >> 1) & 1, code >> 2


# ------------------------------------------------------------------------------------------------ integration
def centres(origin, voxel, dims, dtype=np.float64):
    """voxel centres per axis: origin + dtype(i) * voxel, one rounded multiply and one rounded add"""
    dt = dtype
    return [dt(origin[a]) + np.arange(dims[a]).astype(dt) * dt(voxel) for a in range(3)]


def integrate_ref(tsdf, weight, rgb, frames, origin, voxel, trunc, dtype=np.float64):
    """tsdf, weight [nz, ny, nx], rgb [nz, ny, nx, 3] or None; frames: dicts with `depth` fp32 [h, w] or `pts` fp32 [h, w, 3], optional
    `valid`, `pixel_weight`, `rgba` (uint32 [h, w]), `fu`, `fv`, `cu`, `cv` and `w2c` (12 numbers, row-major 3 x 4).  -> the new
    (tsdf, weight, rgb) in `dtype`.  The frames are walked in order."""
    dt = dtype
    D, W = np.array(tsdf, dt), np.array(weight, dt)
    col = None if rgb is None else np.array(rgb, dt)
    nz, ny, nx = D.shape
    cx, cy, cz = centres(origin, voxel, (nx, ny, nz), dt)
    x, y, z = cx[None, None, :], cy[None, :, None], cz[:, None, None]
    tr = dt(trunc)
    with np.errstate(all="ignore"):
        for fr in frames:
            m = np.asarray(fr["w2c"], np.float32).astype(dt).reshape(12)
            fu, fv, cu, cv = (dt(np.float32(fr[k])) for k in ("fu", "fv", "cu", "cv"))
            src = fr["depth"] if fr.get("depth") is not None else fr["pts"]
            h, w = src.shape[:2]
            zc = ((m[8] * x + m[9] * y) + m[10] * z) + m[11]
            xc = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]
            yc = ((m[4] * x + m[5] * y) + m[6] * z) + m[7]
            ok = zc > 0
            zs = np.where(ok, zc, dt(1))
            u, v = fu * xc / zs + cu, fv * yc / zs + cv
            fpx, fpy = np.floor(u + dt(0.5)), np.floor(v + dt(0.5))
            ok &= (fpx >= 0) & (fpx < w) & (fpy >= 0) & (fpy < h)
            px, py = np.where(ok, fpx, 0).astype(np.int64), np.where(ok, fpy, 0).astype(np.int64)
            if fr.get("valid") is not None:
                ok &= np.asarray(fr["valid"])[py, px] != 0
            if fr.get("depth") is not None:
                d = np.asarray(fr["depth"], np.float32).astype(dt)[py, px]
            else:
                P = np.asarray(fr["pts"], np.float32).astype(dt)[py, px]
                d = ((m[8] * P[..., 0] + m[9] * P[..., 1]) + m[10] * P[..., 2]) + m[11]
            ok &= np.isfinite(d) & (d > 0)
            s = d - zc
            ok &= ~(s < -tr)
            f = np.minimum(dt(1), s / tr)
            if fr.get("pixel_weight") is not None:
                a = np.asarray(fr["pixel_weight"], np.float32).astype(dt)[py, px]
            else:
                a = np.ones(D.shape, dt)
            ok &= (a > 0) & np.isfinite(a)
            a = np.where(ok, a, dt(1))
            Wn = W + a
            D = np.where(ok, (W * D + a * f) / Wn, D)
            if col is not None:
                word = np.asarray(fr["rgba"]).astype(np.uint32)[py, px]
                for ch in range(3):
                    q = ((word >> np.uint32(8 * ch)) & np.uint32(255)).astype(dt) / dt(255)
                    col[..., ch] = np.where(ok, (W * col[..., ch] + a * q) / Wn, col[..., ch])
            W = np.where(ok, Wn, W)
    return D, W, col


# ------------------------------------------------------------------------------------------------ extraction
def _unorm8(c):
    with np.errstate(all="ignore"):
        s = np.floor(c * c.dtype.type(255) + c.dtype.type(0.5))
    return np.where(s >= 255, 255, np.where(s > 0, s, 0)).astype(np.uint32)


def extract_ref(tsdf, weight, rgb, origin, voxel, min_weight=1.0, dtype=np.float64):
    """-> (vertices `dtype` [V, 3], rgba uint32 [V], faces int64 [F, 3]): the vertices in (owner index, slot) order, the faces in
    (cell index, tetrahedron, triangle) order, by the header's rule."""
    dt = dtype
    D = np.asarray(tsdf, np.float32).astype(dt)
    nz, ny, nx = D.shape
    n = nx * ny * nz
    obs = np.asarray(weight, np.float32) >= np.float32(min_weight)
    inside = D < 0
    flags = np.zeros((nz, ny, nx, 7), bool)
    for s, code in enumerate(SLOT_CODE):
        dx, dy, dz = corner_offset(code)
        a = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        b = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        flags[a + (s,)] = obs[a] & obs[b] & (inside[a] != inside[b])
    flags = flags.reshape(n, 7)
    cnt = flags.sum(1)
    voff = np.cumsum(cnt) - cnt
    vidx = voff[:, None] + np.cumsum(flags, axis=1) - flags          # row of the vertex of (owner, slot), where flagged
    owner, slot = np.nonzero(flags)
    code = np.asarray(SLOT_CODE)[slot]
    i, j, k = owner % nx, (owner // nx) % ny, owner // (nx * ny)
    di, dj, dk = code & 1, (code >> 1) & 1, code >> 2
    other = owner + di + nx * (dj + ny * dk)
    flat = D.reshape(n)
    ta, tb = flat[owner], flat[other]
    with np.errstate(all="ignore"):
        t = ta / (ta - tb)
        verts = np.empty((len(owner), 3), dt)
        for ax, (ia, d) in enumerate(((i, di), (j, dj), (k, dk))):
            pa = dt(origin[ax]) + ia.astype(dt) * dt(voxel)
            pb = dt(origin[ax]) + (ia + d).astype(dt) * dt(voxel)
            verts[:, ax] = pa + t * (pb - pa)
        rgba = np.full(len(owner), 0xffffffff, np.uint32)
        if rgb is not None:
            col = np.asarray(rgb, np.float32).astype(dt).reshape(n, 3)
            rgba[:] = np.uint32(255) << np.uint32(24)
            for ch in range(3):
                ca, cb = col[owner, ch], col[other, ch]
                rgba |= _unorm8(ca + t * (cb - ca)) << np.uint32(8 * ch)
    # faces
    live = np.zeros((nz, ny, nx), bool)
    bits = np.zeros((nz, ny, nx), np.int64)
    if nx > 1 and ny > 1 and nz > 1:
        live[:-1, :-1, :-1] = True
        for c in range(8):
            dx, dy, dz = corner_offset(c)
            b = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
            live[:-1, :-1, :-1] &= obs[b]
            bits[:-1, :-1, :-1] |= inside[b].astype(np.int64) << c
    live, bits = live.reshape(n), bits.reshape(n)
    out = np.full((n, 6, 2, 3), -1, np.int64)
    has = np.zeros((n, 6, 2), bool)
    for ti, tet in enumerate(TET):
        cs = sum(((bits >> tet[m]) & 1) << m for m in range(4))
        for case in range(1, 15):
            sel = np.flatnonzero(live & (cs == case))
            if len(sel) == 0:
                continue
            for q, tri in enumerate(CASES[case]):
                has[sel, ti, q] = True
                for xk, (p0, p1) in enumerate(tri):
                    lo, hi = sorted((tet[p0], tet[p1]))
                    dx, dy, dz = corner_offset(lo)
                    own = sel + dx + nx * (dy + ny * dz)
                    out[sel, ti, q, xk] = vidx[own, SLOT_OF[hi - lo]]
    faces = out[has]
    return verts, rgba, faces.reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ helpers of the tests
def sphere_volume(dims, origin, voxel, centre, radius, trunc):
    """(tsdf, weight) fp32 [nz, ny, nx] sampled from the analytic distance to a sphere, truncated to [-1, 1], every voxel seen once"""
    cx, cy, cz = centres(origin, voxel, dims)
    r = np.sqrt((cx[None, None, :] - centre[0]) ** 2 + (cy[None, :, None] - centre[1]) ** 2 + (cz[:, None, None] - centre[2]) ** 2)
    return np.clip((r - radius) / trunc, -1, 1).astype(np.float32), np.ones(r.shape, np.float32)


def directed_edges(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def manifold_report(faces):
    """-> dict: `closed` (every undirected edge in exactly two faces, once per direction), `euler` = V - E + F over the referenced
    vertices, `boundary` = the undirected edges used by exactly one face [B, 2], `bad` = edges used more than twice or twice in the
    same direction"""
    e = directed_edges(faces)
    if len(e) == 0:
        return dict(closed=True, euler=0, boundary=np.zeros((0, 2), np.int64), bad=0)
    und, inv, cnt = np.unique(np.sort(e, axis=1), axis=0, return_inverse=True, return_counts=True)
    _, dcnt = np.unique(e, axis=0, return_counts=True)
    bad = int((cnt > 2).sum() + (dcnt > 1).sum())
    nv = len(np.unique(e))
    return dict(closed=bool((cnt == 2).all() and bad == 0), euler=nv - len(und) + len(np.asarray(faces).reshape(-1, 3)),
                boundary=und[cnt == 1], bad=bad)


# ------------------------------------------------------------------------------------------------ the synthetic scene of the tests
SCENE = dict(dims=(21, 18, 13), origin=(-0.84, -0.72, -0.2), voxel=0.08, trunc=0.24, sphere=((0.0, 0.0, 0.45), 0.45), h=24, w=32)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """cam2world float64 [4, 4] of a camera at `eye` looking at `target` (OpenCV axes: +z forward, +y down)"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    zf = target - eye
    zf /= np.linalg.norm(zf)
    xr = np.cross(zf, up)
    xr /= np.linalg.norm(xr)
    yd = np.cross(zf, xr)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = xr, yd, zf, eye
    return P


SCENE_EYES = [((0.1, -1.5, 1.1), (0.0, 0.0, 0.2)), ((1.4, 0.3, 0.9), (0.0, 0.0, 0.3)), ((0.55, -0.45, 0.6), (-0.3, 0.2, 0.0)),
              ((-1.3, -0.8, 1.2), (0.0, 0.0, 0.2)), ((-0.4, 1.5, 0.8), (0.0, 0.0, 0.3))]


def analytic_depth(P, fu, fv, cu, cv, h, w, centre, radius):
    """camera z of the nearer of the plane z = 0 and the sphere, seen through cam2world P: (depth float64 [h, w] (0: nothing hit), the
    world ray per unit camera z [h, w, 3], the eye)"""
    ys, xs = np.mgrid[0:h, 0:w]
    dirs = np.stack([(xs - cu) / fu, (ys - cv) / fv, np.ones((h, w))], -1) @ P[:3, :3].T
    o, c, r = P[:3, 3], np.asarray(centre, np.float64), radius
    with np.errstate(all="ignore"):
        tp = np.where(dirs[..., 2] < 0, -o[2] / dirs[..., 2], np.inf)                                # the plane z = 0
        A, B, Cq = (dirs ** 2).sum(-1), 2 * (dirs * (o - c)).sum(-1), ((o - c) ** 2).sum() - r * r
        disc = B * B - 4 * A * Cq
        ts = np.where(disc > 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), np.inf)
        ts = np.where(ts > 0, ts, np.inf)
    d = np.minimum(tp, ts)
    return np.where(np.isfinite(d), d, 0.0), dirs, o


def scene_frames(seed=0, n=5):
    """n frames of SCENE (a sphere resting on the plane z = 0) with analytic depth: dicts with depth, pts (world, fp32), valid (an invalid
    rim and random holes), pixel_weight (frame 1 only; it holds a zero, an inf and a NaN), images (fp32 [h, w, 3], multiples of 1 / 255),
    rgba, K, cam2world.  Frame 0's depth holds zeros, one NaN and one negative value; frame 2 sits inside the volume, so voxels lie
    behind it."""
    rng = np.random.default_rng(seed)
    h, w = SCENE["h"], SCENE["w"]
    (c, r) = SCENE["sphere"]
    c = np.asarray(c)
    frames = []
    for i in range(n):
        P = look_at(*SCENE_EYES[i])
        fu, fv, cu, cv = 26.0 + i, 25.0 + 0.5 * i, (w - 1) / 2 + 0.25, (h - 1) / 2 - 0.5
        K = np.array([[fu, 0, cu], [0, fv, cv], [0, 0, 1]])
        d, dirs, o = analytic_depth(P, fu, fv, cu, cv, h, w, c, r)
        depth = d.astype(np.float32)
        valid = np.ones((h, w), np.uint8)
        valid[0, :] = valid[-1, :] = valid[:, 0] = valid[:, -1] = 0
        valid[rng.integers(1, h - 1, 6), rng.integers(1, w - 1, 6)] = 0
        if i == 0:
            depth[5, 7] = depth[11, 20] = depth[17, 3] = 0.0
            depth[9, 14] = np.nan
            depth[13, 9] = -1.0
        pts = (o + dirs * depth.astype(np.float64)[..., None]).astype(np.float32)
        fr = dict(depth=depth, pts=pts, valid=valid, pixel_weight=None, K=K, cam2world=P, fu=fu, fv=fv, cu=cu, cv=cv)
        if i == 1:
            a = rng.uniform(0.5, 2.0, (h, w)).astype(np.float32)
            a[6, 6], a[7, 15], a[12, 12] = 0.0, np.inf, np.nan
            fr["pixel_weight"] = a
        byte = rng.integers(0, 256, (h, w, 3))
        fr["images"] = (byte / 255.0).astype(np.float32)
        fr["rgba"] = (byte[..., 0] | byte[..., 1] << 8 | byte[..., 2] << 16 | 255 << 24).astype(np.uint32)
        fr["w2c"] = np.linalg.inv(P)[:3].reshape(12).astype(np.float32)
        frames.append(fr)
    return frames


def as_path(frames, path):
    """the frames with only `depth` or only `pts` as their source"""
    return [{**f, "depth": f["depth"] if path == "depth" else None, "pts": f["pts"] if path == "pts" else None} for f in frames]


def empty_volume(dims, color=True):
    nx, ny, nz = dims
    return np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx, 3), np.float32) if color else None
