"""Numpy restatement of the rules of include/spann3r_hip.h, "TSDF ray-casting and frame-to-model tracking": the ray-caster of the
volume's zero level (sp3_tsdf_raycast), the normal equations of projective point-to-plane registration of one frame against the
ray-cast maps (sp3_tsdf_track_accum) and the host loop around them (spann3r_amd.fusion.track_frame), plus the scene the tests use.
It is the pin of those in tests/test_raycast_gpu.py; tests/test_raycast_cpu.py checks the restatement itself (against the analytic
depth of the scene, and that tracking recovers a known rigid motion).  There is no reference implementation of either stage.

The ray-caster runs in float64 by default; with dtype=np.float32 every operation is rounded to fp32 in the header's order, which is
what the kernel is compared with bit for bit.  The accumulation is float64 always.  No torch."""
import math

import numpy as np

import fusion_ref as FR


# ------------------------------------------------------------------------------------------------ ray-casting
def march_cap(dims, voxel, step):
    """the hard bound of samples per ray, computed in double from the fp32 voxel and step"""
    return int(math.ceil(2.0 * (dims[0] + dims[1] + dims[2]) * float(np.float32(voxel)) / float(np.float32(step))))


def _lerp(a, b, t):
    return a + t * (b - a)


class _Volume:
    def __init__(self, tsdf, weight, rgb, origin, voxel, min_weight, dt):
        self.dt = dt
        D = np.asarray(tsdf, np.float32)
        self.nz, self.ny, self.nx = D.shape
        self.n = D.size
        self.D = D.astype(dt).reshape(-1)
        self.obs = (np.asarray(weight, np.float32) >= np.float32(min_weight)).reshape(-1)
        self.col = None if rgb is None else np.asarray(rgb, np.float32).astype(dt).reshape(-1, 3)
        self.origin = [dt(np.float32(o)) for o in origin]
        self.voxel = dt(np.float32(voxel))

    def cell(self, p, full=False):
        """the cell of the points p [m, 3]: (valid [m], value [m]) and with `full` also (gradient [m, 3], colour [m, 3] or None)"""
        dt = self.dt
        dims = (self.nx, self.ny, self.nz)
        g = [(p[:, a] - self.origin[a]) / self.voxel for a in range(3)]
        fi = [np.floor(x) for x in g]
        ok = np.ones(len(p), bool)
        for a in range(3):
            ok &= (fi[a] >= 0) & (fi[a] <= dims[a] - 2)                      # (a NaN fails)
        i, j, k = (np.where(ok, fi[a], 0).astype(np.int64) for a in range(3))
        tx, ty, tz = (g[a] - fi[a] for a in range(3))
        base = np.where(ok, (k * self.ny + j) * self.nx + i, 0)
        idx = {}
        for c in range(8):
            dx, dy, dz = FR.corner_offset(c)
            q = np.where(ok, base + dx + self.nx * (dy + self.ny * dz), 0)
            idx[dx, dy, dz] = q
            ok &= self.obs[q]
        v = {c: self.D[q] for c, q in idx.items()}

        def tri(v):
            e = {(b, c): _lerp(v[0, b, c], v[1, b, c], tx) for b in (0, 1) for c in (0, 1)}
            f = {c: _lerp(e[0, c], e[1, c], ty) for c in (0, 1)}
            return _lerp(f[0], f[1], tz)

        val = tri(v)
        if not full:
            return ok, val
        dX = {(b, c): v[1, b, c] - v[0, b, c] for b in (0, 1) for c in (0, 1)}       # along x: lerp y, then z
        gx = _lerp(_lerp(dX[0, 0], dX[1, 0], ty), _lerp(dX[0, 1], dX[1, 1], ty), tz)
        dY = {(a, c): v[a, 1, c] - v[a, 0, c] for a in (0, 1) for c in (0, 1)}       # along y: lerp x, then z
        gy = _lerp(_lerp(dY[0, 0], dY[1, 0], tx), _lerp(dY[0, 1], dY[1, 1], tx), tz)
        dZ = {(a, b): v[a, b, 1] - v[a, b, 0] for a in (0, 1) for b in (0, 1)}       # along z: lerp x, then y
        gz = _lerp(_lerp(dZ[0, 0], dZ[1, 0], tx), _lerp(dZ[0, 1], dZ[1, 1], tx), ty)
        col = None
        if self.col is not None:
            col = np.stack([tri({c: self.col[q, ch] for c, q in idx.items()}) for ch in range(3)], -1)
        return ok, val, np.stack([gx, gy, gz], -1), col


def raycast_ref(tsdf, weight, rgb, origin, voxel, view, min_weight=1.0, step=None, dtype=np.float64):
    """One view of the volume by the header's rule.  view: dict with w, h, fu, fv, cu, cv, c2w (12 numbers, row-major 3 x 4) and
    optional near, far.  step: metric (default one voxel).  -> dict(depth [h, w], vertex [h, w, 3], normal [h, w, 3] in `dtype`,
    rgba uint32 [h, w] (zeros without rgb), hit bool [h, w])."""
    dt = dtype
    vol = _Volume(tsdf, weight, rgb, origin, voxel, min_weight, dt)
    step = dt(np.float32(vol.voxel if step is None else step))
    h, w = int(view["h"]), int(view["w"])
    fu, fv, cu, cv = (dt(np.float32(view[k])) for k in ("fu", "fv", "cu", "cv"))
    m = np.asarray(view["c2w"], np.float32).astype(dt).reshape(3, 4)
    near, far = dt(np.float32(view.get("near", 0.0))), dt(np.float32(view.get("far", np.inf)))
    cap = march_cap((vol.nx, vol.ny, vol.nz), vol.voxel, step)
    ys, xs = np.mgrid[0:h, 0:w]
    n = h * w
    with np.errstate(all="ignore"):
        xn, yn = (xs.reshape(-1).astype(dt) - cu) / fu, (ys.reshape(-1).astype(dt) - cv) / fv
        d = [(m[r, 0] * xn + m[r, 1] * yn) + m[r, 2] for r in range(3)]
        eye = [m[r, 3] for r in range(3)]
        length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        dl = step / length
        enter, leave = np.full(n, -np.inf, dt), np.full(n, np.inf, dt)
        alive = np.ones(n, bool)
        for a, na in enumerate((vol.nx, vol.ny, vol.nz)):
            lo, hi = vol.origin[a], vol.origin[a] + dt(na - 1) * vol.voxel
            zero = d[a] == 0
            alive &= ~zero | ((lo <= eye[a]) & (eye[a] <= hi))
            da = np.where(zero, dt(1), d[a])
            q1, q2 = (lo - eye[a]) / da, (hi - eye[a]) / da
            small, large = np.where(q2 < q1, q2, q1), np.where(q2 < q1, q1, q2)
            enter = np.where(~zero & (small > enter), small, enter)
            leave = np.where(~zero & (large < leave), large, leave)
        lam0 = np.where(near > enter, near, enter)
        lam1 = np.where(far < leave, far, leave)
        alive &= lam0 <= lam1
        prev_valid = np.zeros(n, bool)
        f_prev = np.zeros(n, dt)
        hit = np.zeros(n, bool)
        lam_star = np.zeros(n, dt)
        for i in range(cap):
            lam = lam0 + dt(i) * dl
            alive &= lam <= lam1
            if not alive.any():
                break
            p = np.stack([eye[r] + d[r] * lam for r in range(3)], -1)
            ok, f = vol.cell(p)
            cross = alive & ok & prev_valid
            front = cross & (f_prev >= 0) & (f < 0)
            back = cross & (f_prev < 0) & (f >= 0)
            lam_prev = lam0 + dt(i - 1) * dl
            lam_star = np.where(front, lam_prev + dl * (f_prev / (f_prev - f)), lam_star)
            hit |= front
            alive &= ~(front | back)
            f_prev = np.where(alive & ok, f, f_prev)
            prev_valid = np.where(alive, ok, prev_valid)
        ps = np.stack([eye[r] + d[r] * lam_star for r in range(3)], -1)
        ok, _, grad, col = vol.cell(np.where(hit[:, None], ps, dt(np.nan)), full=True)
        glen = np.sqrt((grad[:, 0] * grad[:, 0] + grad[:, 1] * grad[:, 1]) + grad[:, 2] * grad[:, 2])
        hit &= ok & (glen > 0) & np.isfinite(glen)
        normal = grad / np.where(hit, glen, dt(1))[:, None]
        rgba = np.zeros(n, np.uint32)
        if col is not None:
            rgba[:] = np.uint32(255) << np.uint32(24)
            for ch in range(3):
                rgba |= FR._unorm8(np.where(hit, col[:, ch], dt(0))) << np.uint32(8 * ch)
    z = dt(0)
    return dict(depth=np.where(hit, lam_star, z).reshape(h, w), vertex=np.where(hit[:, None], ps, z).reshape(h, w, 3),
                normal=np.where(hit[:, None], normal, z).reshape(h, w, 3), rgba=np.where(hit, rgba, np.uint32(0)).reshape(h, w),
                hit=hit.reshape(h, w))


# ------------------------------------------------------------------------------------------------ tracking
UPPER = [(a, b) for a in range(6) for b in range(a, 6)]


def track_accum_ref(pts, valid, T, model, w2c, dist_max, return_abs=False):
    """The normal equations of sp3_tsdf_track_accum in float64: pts [n, 3], valid [n] or None, T [4, 4] the correction, model the
    dict of raycast_ref (depth, vertex, normal), w2c [4, 4] of the model view with fu, fv, cu, cv in `model`.  -> out29 (and with
    return_abs the sum of the absolute values of the terms of every entry, for the rounding bound of a reordered sum)."""
    p = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    depth = np.asarray(model["depth"]).astype(np.float64)
    h, w = depth.shape
    fu, fv, cu, cv = (float(np.float32(model[k])) for k in ("fu", "fv", "cu", "cv"))
    with np.errstate(all="ignore"):
        y = p @ T[:3, :3].T + T[:3, 3]
        ok = np.isfinite(p).all(1)
        if valid is not None:
            ok &= np.asarray(valid).reshape(-1) != 0
        yc = y @ w2c[:3, :3].T + w2c[:3, 3]
        ok &= yc[:, 2] > 0
        zs = np.where(ok, yc[:, 2], 1.0)
        u, v = fu * yc[:, 0] / zs + cu, fv * yc[:, 1] / zs + cv
        fx, fy = np.floor(u + 0.5), np.floor(v + 0.5)
        ok &= (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)
        px, py = np.where(ok, fx, 0).astype(np.int64), np.where(ok, fy, 0).astype(np.int64)
        ok &= depth[py, px] != 0
        q = np.asarray(model["vertex"]).astype(np.float64)[py, px]
        nrm = np.asarray(model["normal"]).astype(np.float64)[py, px]
        d = y - q
        ok &= (d * d).sum(1) <= float(dist_max) ** 2
    y, nrm, d = y[ok], nrm[ok], d[ok]
    r = (nrm * d).sum(1)
    J = np.concatenate([np.cross(y, nrm), nrm], 1)
    terms = np.concatenate([np.stack([J[:, a] * J[:, b] for a, b in UPPER], 1), J * r[:, None], (r * r)[:, None], np.ones((len(r), 1))], 1)
    out = terms.sum(0)
    return (out, np.abs(terms).sum(0)) if return_abs else out


def expm_so3(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def solve_step(out29):
    """the host step of track_frame: -> the 4 x 4 update exp(xi), or None for a non-finite or rank-deficient system"""
    H = np.zeros((6, 6))
    for e, (a, b) in enumerate(UPPER):
        H[a, b] = H[b, a] = out29[e]
    g = out29[21:27]
    if not (np.isfinite(H).all() and np.isfinite(g).all()):
        return None
    s = np.linalg.svd(H, compute_uv=False)
    if not (s[0] > 0 and s[-1] >= 1e-9 * s[0]):
        return None
    xi = np.linalg.lstsq(H, -g, rcond=None)[0]
    U = np.eye(4)
    U[:3, :3], U[:3, 3] = expm_so3(xi[:3]), xi[3:]
    return U


def track_frame_ref(state, origin, voxel, trunc, pts, valid, K, cam2world, iterations=10, recasts=2, dist_max=None, min_pairs=64,
                    step_voxels=1.0, min_weight=1.0, relative_rmse=1e-6, dtype=np.float64, trace=None):
    """spann3r_amd.fusion.track_frame restated: state = (tsdf, weight, rgb).  -> (T [4, 4], info).  trace: a list that receives one
    dict(T, model, w2c, out29, abs29) per accumulate call."""
    tsdf, weight, _ = state
    h, w = pts.shape[:2]
    dist_max = float(np.float32(trunc)) if dist_max is None else float(dist_max)
    step = np.float32(np.float32(step_voxels) * np.float32(voxel))
    T = np.eye(4)
    info = dict(tracked=False, pairs=0, rmse=float("nan"), iterations=0)
    for _ in range(recasts):
        P = T @ np.asarray(cam2world, np.float64)
        view = dict(w=w, h=h, fu=K[0, 0], fv=K[1, 1], cu=K[0, 2], cv=K[1, 2], c2w=P[:3].reshape(12).astype(np.float32))
        model = raycast_ref(tsdf, weight, None, origin, voxel, view, min_weight, step, dtype)
        model.update(fu=K[0, 0], fv=K[1, 1], cu=K[0, 2], cv=K[1, 2])
        w2c = np.linalg.inv(P)
        last = None
        for _ in range(iterations):
            out, ab = track_accum_ref(pts, valid, T, model, w2c, dist_max, return_abs=True)
            if trace is not None:
                trace.append(dict(T=T.copy(), model=model, w2c=w2c, out29=out, abs29=ab))
            info["iterations"] += 1
            info["pairs"] = int(out[28])
            if out[28] < min_pairs:
                return np.eye(4), dict(info, tracked=False)
            rmse = math.sqrt(out[27] / out[28])
            info["rmse"] = rmse
            if last is not None and abs(rmse - last) < relative_rmse:
                break
            last = rmse
            U = solve_step(out)
            if U is None:
                return np.eye(4), dict(info, tracked=False)
            T = U @ T
    info["tracked"] = True
    return T, info


# ------------------------------------------------------------------------------------------------ the scene of the tests
# A room corner with two spheres: rotation about every axis and translation along every axis are observable (fusion_ref.SCENE, a
# sphere on a plane, leaves the rotation about the vertical unobservable).  The room lies on the +z, -y and +x sides of its planes.
SCENE = dict(dims=(41, 35, 23), origin=(-0.84, -0.72, -0.12), voxel=0.04, trunc=0.12, h=48, w=64,
             planes=((2, 0.0, -1), (1, 0.56, +1), (0, -0.72, -1)),          # (axis, offset, sign of the ray component that reaches it)
             spheres=(((0.0, 0.0, 0.45), 0.45), ((0.45, -0.35, 0.2), 0.2)), target=(-0.05, 0.05, 0.25), centre=(0.0, 0.0, 0.3))
N_FRAMES = 6


def scene_camera(i):
    P = FR.look_at((0.95 - 0.12 * i, -1.25 + 0.05 * i, 0.85 + 0.03 * i), SCENE["target"])
    K = np.array([[40.0 + i, 0, 31.75], [0, 39.0 + 0.5 * i, 23.0], [0, 0, 1]])
    return K, P


def analytic_depth(K, P, h, w):
    """camera z of the nearest surface of SCENE through cam2world P: (depth float64 [h, w], the world ray per unit camera z, the eye)"""
    ys, xs = np.mgrid[0:h, 0:w]
    dirs = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones((h, w))], -1) @ P[:3, :3].T
    o = P[:3, 3]
    best = np.full((h, w), np.inf)
    with np.errstate(all="ignore"):
        for axis, off, sign in SCENE["planes"]:
            t = np.where(dirs[..., axis] * sign > 0, (off - o[axis]) / dirs[..., axis], np.inf)
            best = np.minimum(best, np.where(t > 0, t, np.inf))
        for c, r in SCENE["spheres"]:
            c = np.asarray(c)
            A, B, Cq = (dirs ** 2).sum(-1), 2 * (dirs * (o - c)).sum(-1), ((o - c) ** 2).sum() - r * r
            disc = B * B - 4 * A * Cq
            t = np.where(disc > 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), np.inf)
            best = np.minimum(best, np.where(t > 0, t, np.inf))
    return np.where(np.isfinite(best), best, 0.0), dirs, o


def scene_frames(seed=0):
    """the six frames of SCENE: dicts with depth (analytic, fp32), pts (world, fp32), valid, images / rgba (seeded bytes), K,
    cam2world, fu, fv, cu, cv, w2c (fp32 [12], inverted in float64)"""
    rng = np.random.default_rng(seed)
    h, w = SCENE["h"], SCENE["w"]
    frames = []
    for i in range(N_FRAMES):
        K, P = scene_camera(i)
        d, dirs, o = analytic_depth(K, P, h, w)
        depth = d.astype(np.float32)
        pts = (o + dirs * depth.astype(np.float64)[..., None]).astype(np.float32)
        byte = rng.integers(0, 256, (h, w, 3))
        frames.append(dict(depth=depth, pts=pts, valid=(depth > 0).astype(np.uint8), pixel_weight=None, K=K, cam2world=P, fu=K[0, 0], fv=K[1, 1],
                           cu=K[0, 2], cv=K[1, 2], images=(byte / 255.0).astype(np.float32),
                           rgba=(byte[..., 0] | byte[..., 1] << 8 | byte[..., 2] << 16 | 255 << 24).astype(np.uint32),
                           w2c=np.linalg.inv(P)[:3].reshape(12).astype(np.float32)))
    return frames


def fuse_ref(frames, color=True, dtype=np.float32):
    """the frames integrated through the `pts` path into SCENE's volume: (tsdf, weight, rgb)"""
    S = SCENE
    return FR.integrate_ref(*FR.empty_volume(S["dims"], color), FR.as_path(frames, "pts"), np.float32(S["origin"]), np.float32(S["voxel"]),
                            np.float32(S["trunc"]), dtype)


def scene_view(fr, **kw):
    return dict(w=SCENE["w"], h=SCENE["h"], fu=fr["fu"], fv=fr["fv"], cu=fr["cu"], cv=fr["cv"],
                c2w=np.asarray(fr["cam2world"])[:3].reshape(12).astype(np.float32), **kw)


def smooth_mask(depth, tol):
    """pixels that are not on a depth discontinuity or a crease: no miss in the 3 x 3 neighbourhood, and the second difference of
    `depth` across the pixel stays below tol along the row, the column and both diagonals"""
    h, w = depth.shape
    pad = np.pad(depth, 1, mode="edge")
    nb = {(a, b): pad[1 + a:1 + a + h, 1 + b:1 + b + w] for a in (-1, 0, 1) for b in (-1, 0, 1)}
    ok = np.min(list(nb.values()), axis=0) > 0
    for a, b in ((0, 1), (1, 0), (1, 1), (1, -1)):
        ok &= np.abs(nb[-a, -b] - 2 * depth + nb[a, b]) < tol
    return ok


def perturbations(seed, n=N_FRAMES):
    """one rigid motion per frame 1..n-1 (frame 0: identity): 2 degrees about a random axis through SCENE's centre plus one voxel in a
    random direction; default_rng(seed), per frame the axis first, then the direction, both rng.normal(size=3) normalised"""
    rng = np.random.default_rng(seed)
    c = np.asarray(SCENE["centre"])
    out = [np.eye(4)]
    for _ in range(1, n):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        push = rng.normal(size=3)
        push /= np.linalg.norm(push)
        M = np.eye(4)
        M[:3, :3] = expm_so3(axis * np.deg2rad(2.0))
        M[:3, 3] = c - M[:3, :3] @ c + SCENE["voxel"] * push
        out.append(M)
    return out


def perturbed_frames(frames, motions):
    """every frame's pointmap and pose moved by its motion (float64, the pointmap rounded to fp32)"""
    out = []
    for fr, M in zip(frames, motions):
        pts = (fr["pts"].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
        P = M @ fr["cam2world"]
        out.append({**fr, "pts": pts, "cam2world": P, "depth": None, "w2c": np.linalg.inv(P)[:3].reshape(12).astype(np.float32)})
    return out


def motion_size(E):
    """(rotation angle in degrees, norm of the translation) of a rigid 4 x 4"""
    c = min(max((np.trace(E[:3, :3]) - 1) * 0.5, -1.0), 1.0)
    return math.degrees(math.acos(c)), float(np.linalg.norm(E[:3, 3]))


def track_sequence_ref(frames, dtype=np.float64, **kw):
    """fuse_pointmaps(track=True) restated on SCENE's volume: integrate frame 0; track, move and integrate every later frame.
    -> (corrections [n] of 4 x 4, infos, final state)"""
    S = SCENE
    origin, voxel, trunc = np.float32(S["origin"]), np.float32(S["voxel"]), np.float32(S["trunc"])
    state = FR.empty_volume(S["dims"], False)
    Ts, infos = [], []
    for i, fr in enumerate(frames):
        T, info = np.eye(4), dict(tracked=True, pairs=0, rmse=0.0, iterations=0)
        if i > 0:
            T, info = track_frame_ref(state, origin, voxel, trunc, fr["pts"], fr["valid"], fr["K"], fr["cam2world"], dtype=dtype, **kw)
        pts = fr["pts"] if i == 0 else (fr["pts"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        P = T @ fr["cam2world"]
        moved = dict(fr, pts=pts, depth=None, w2c=np.linalg.inv(P)[:3].reshape(12).astype(np.float32))
        state = FR.integrate_ref(*state, [moved], origin, voxel, trunc, np.float32)
        Ts.append(T)
        infos.append(info)
    return Ts, infos, state
