"""Numpy restatement of the rules of include/spann3r_hip.h, "Multi-view consistency": every pixel's world point looked up in every
other frame (sp3_multiview_counts) and the confidence clipped where another frame looks through it (sp3_multiview_clean).  It is the
pin of spann3r_amd.multiview in tests/test_multiview_gpu.py; tests/test_multiview_cpu.py checks the restatement itself (against a
pixel-by-pixel loop over fp32 scalars, on pinned totals and on a fronto-parallel wall whose counts can be read off).  The rule is
DUSt3R's BasePCOptimizer.clean_pointcloud with the lookup of sp3_tsdf_integrate; parity with that method is unpinned (dust3r.cloud_opt
cannot be imported here), so this restatement of the header's own rule is the anchor.

Every operation is rounded to fp32 in the header's order, which is what the kernel is compared with bit for bit.  No torch.

Frames are the dicts of tests/fusion_ref.py: `pts` fp32 [h, w, 3], optional `valid`, `fu`, `fv`, `cu`, `cv`, `w2c` (12 numbers).  The
confidences are passed separately, as a list of fp32 [h, w] (None: a frame without one); a frame's `pixel_weight` is not looked at."""
import numpy as np

F = np.float32
SEEN, AGREE, FRONT, STRONGER = 0, 1, 2, 3


def _cam(fr):
    return np.asarray(fr["w2c"], F).reshape(12), F(fr["fu"]), F(fr["fv"]), F(fr["cu"]), F(fr["cv"])


# ------------------------------------------------------------------------------------------------ vectorised
def lookup(X, fr, tol):
    """world points X fp32 [..., 3] looked up in frame `fr` -> (seen, front, agree bool [...], py, px int64 [...] (0 where not seen))"""
    m, fu, fv, cu, cv = _cam(fr)
    P = np.asarray(fr["pts"], F)
    h, w = P.shape[:2]
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    with np.errstate(all="ignore"):
        zc = ((m[8] * x + m[9] * y) + m[10] * z) + m[11]
        ok = zc > 0
        xc = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]
        yc = ((m[4] * x + m[5] * y) + m[6] * z) + m[7]
        zs = np.where(ok, zc, F(1))
        u, v = fu * xc / zs + cu, fv * yc / zs + cv
        fpx, fpy = np.floor(u + F(0.5)), np.floor(v + F(0.5))
        ok &= (fpx >= 0) & (fpx < F(w)) & (fpy >= 0) & (fpy < F(h))
        px, py = np.where(ok, fpx, 0).astype(np.int64), np.where(ok, fpy, 0).astype(np.int64)
        if fr.get("valid") is not None:
            ok &= np.asarray(fr["valid"])[py, px] != 0
        Q = P[py, px]
        d = ((m[8] * Q[..., 0] + m[9] * Q[..., 1]) + m[10] * Q[..., 2]) + m[11]
        ok &= np.isfinite(d) & (d > 0)
        lo, hi = (F(1.0) - F(tol)) * d, (F(1.0) + F(tol)) * d
        front = ok & (zc < lo)
        agree = ok & ~front & ~(zc > hi)
    return ok, front, agree, np.where(ok, py, 0), np.where(ok, px, 0)


def _valid_of(fr, own_valid=True):
    h, w = np.asarray(fr["pts"]).shape[:2]
    return np.ones((h, w), bool) if fr.get("valid") is None or not own_valid else np.asarray(fr["valid"]) != 0


def counts_ref(frames, conf, tol, own_valid=True):
    """-> list of int32 [h, w, 4] = (seen, agree, front, stronger) per frame, against the ORIGINAL confidences.
    own_valid=False leaves out the rule's first line (valid_i[q] == 0 gives zeros) and keeps `valid` at the target only: not the
    rule, but the computation the totals of the issue's table were taken from (tests/test_multiview_cpu.py pins both)."""
    conf = [None] * len(frames) if conf is None else conf
    out = []
    for i, fi in enumerate(frames):
        X = np.asarray(fi["pts"], F)
        own = _valid_of(fi, own_valid)
        c = np.zeros(X.shape[:2] + (4,), np.int32)
        for j, fj in enumerate(frames):
            if j == i:
                continue
            seen, front, agree, py, px = lookup(X, fj, tol)
            seen, front, agree = seen & own, front & own, agree & own
            c[..., SEEN] += seen
            c[..., AGREE] += agree
            c[..., FRONT] += front
            if conf[i] is not None and conf[j] is not None:
                with np.errstate(invalid="ignore"):
                    c[..., STRONGER] += front & (np.asarray(conf[i], F) < np.asarray(conf[j], F)[py, px])
        out.append(c)
    return out


def clip(conf, bad, max_bad_conf):
    """min(conf, max_bad_conf) where bad (conf < max_bad_conf ? conf : max_bad_conf), the input bits elsewhere"""
    conf = np.asarray(conf, F)
    with np.errstate(invalid="ignore"):
        return np.where(bad, np.where(conf < F(max_bad_conf), conf, F(max_bad_conf)), conf).astype(F)


def clean_ref(frames, conf, tol, max_bad_conf=0.0, order="sequence", own_valid=True):
    """-> list of fp32 [h, w]: the cleaned confidences.  parallel: every frame is judged against the original confidences; sequence:
    frames are processed in order and frame i is judged against the cleaned confidences of j < i and the original ones of j > i.
    own_valid: as counts_ref."""
    assert order in ("parallel", "sequence")
    orig = [np.asarray(c, F) for c in conf]
    out = []
    for i, fi in enumerate(frames):
        X = np.asarray(fi["pts"], F)
        own = _valid_of(fi, own_valid)
        bad = np.zeros(X.shape[:2], bool)
        for j, fj in enumerate(frames):
            if j == i:
                continue
            cj = out[j] if (order == "sequence" and j < i) else orig[j]
            _, front, _, py, px = lookup(X, fj, tol)
            with np.errstate(invalid="ignore"):
                bad |= front & own & (orig[i] < cj[py, px])
        out.append(clip(orig[i], bad, max_bad_conf))
    return out


def behind(c):
    return c[..., SEEN] - c[..., AGREE] - c[..., FRONT]


def totals(counts):
    """-> dict of the five totals over all frames"""
    t = sum(c.reshape(-1, 4).astype(np.int64).sum(0) for c in counts)
    return dict(seen=int(t[SEEN]), agree=int(t[AGREE]), front=int(t[FRONT]), stronger=int(t[STRONGER]),
                behind=int(t[SEEN] - t[AGREE] - t[FRONT]))


# ------------------------------------------------------------------------------------------------ pixel by pixel
def lookup_scalar(X, fr, tol):
    """one world point (three np.float32) in frame fr, the header's steps on fp32 scalars -> None (skipped) or (py, px, class) with
    class 'front', 'behind' or 'agree'"""
    m, fu, fv, cu, cv = _cam(fr)
    P = fr["pts"]
    h, w = P.shape[:2]
    x, y, z = F(X[0]), F(X[1]), F(X[2])
    with np.errstate(all="ignore"):
        zc = F(F(F(m[8] * x) + F(m[9] * y)) + F(m[10] * z)) + m[11]
        if not zc > 0:
            return None
        xc = F(F(F(m[0] * x) + F(m[1] * y)) + F(m[2] * z)) + m[3]
        yc = F(F(F(m[4] * x) + F(m[5] * y)) + F(m[6] * z)) + m[7]
        u = F(F(F(fu * xc) / zc) + cu)
        v = F(F(F(fv * yc) / zc) + cv)
        fpx, fpy = np.floor(F(u + F(0.5))), np.floor(F(v + F(0.5)))
        if not (fpx >= 0 and fpx < F(w) and fpy >= 0 and fpy < F(h)):
            return None
        px, py = int(fpx), int(fpy)
        if fr.get("valid") is not None and fr["valid"][py, px] == 0:
            return None
        Q = P[py, px]
        d = F(F(F(m[8] * F(Q[0])) + F(m[9] * F(Q[1]))) + F(m[10] * F(Q[2]))) + m[11]
        if not (np.isfinite(d) and d > 0):
            return None
        lo, hi = F(F(1.0) - F(tol)) * d, F(F(1.0) + F(tol)) * d
        cls = "front" if zc < lo else ("behind" if zc > hi else "agree")
    return py, px, cls


def counts_loop(frames, conf, tol):
    conf = [None] * len(frames) if conf is None else conf
    out = []
    for i, fi in enumerate(frames):
        h, w = fi["pts"].shape[:2]
        c = np.zeros((h, w, 4), np.int32)
        for qy in range(h):
            for qx in range(w):
                if fi.get("valid") is not None and fi["valid"][qy, qx] == 0:
                    continue
                for j, fj in enumerate(frames):
                    if j == i:
                        continue
                    r = lookup_scalar(fi["pts"][qy, qx], fj, tol)
                    if r is None:
                        continue
                    py, px, cls = r
                    c[qy, qx, SEEN] += 1
                    c[qy, qx, AGREE] += cls == "agree"
                    c[qy, qx, FRONT] += cls == "front"
                    if cls == "front" and conf[i] is not None and conf[j] is not None and F(conf[i][qy, qx]) < F(conf[j][py, px]):
                        c[qy, qx, STRONGER] += 1
        out.append(c)
    return out


def clean_loop(frames, conf, tol, max_bad_conf=0.0, order="sequence"):
    orig = [np.asarray(c, F) for c in conf]
    out = []
    for i, fi in enumerate(frames):
        h, w = fi["pts"].shape[:2]
        o = orig[i].copy()
        for qy in range(h):
            for qx in range(w):
                if fi.get("valid") is not None and fi["valid"][qy, qx] == 0:
                    continue
                bad = False
                for j, fj in enumerate(frames):
                    if j == i:
                        continue
                    r = lookup_scalar(fi["pts"][qy, qx], fj, tol)
                    if r is None or r[2] != "front":
                        continue
                    cj = out[j] if (order == "sequence" and j < i) else orig[j]
                    bad = bad or bool(orig[i][qy, qx] < cj[r[0], r[1]])
                if bad and not orig[i][qy, qx] < F(max_bad_conf):
                    o[qy, qx] = F(max_bad_conf)
        out.append(o)
    return out


# ------------------------------------------------------------------------------------------------ the scenes of the tests
def scene_conf(n=5, h=24, w=32):
    """the confidences of the pinned totals: one generator, frames 0..n-1 drawn in order"""
    rng = np.random.default_rng(1)
    return [(1 + rng.uniform(0, 9, (h, w))).astype(F) for _ in range(n)]


WALL_EYES = ((0.0, 0.0, 2.0), (0.25, 0.0, 2.0), (0.0, 0.1875, 2.0), (-0.25, -0.125, 2.0))
WALL = dict(h=24, w=32, fu=32.0, fv=32.0, cu=15.5, cv=11.5, depth=2.0, conf=3.0, patch=(1, slice(10, 14), slice(12, 16)))


def wall_pose(eye):
    """cam2world float64 [4, 4]: rotation columns (1, 0, 0), (0, -1, 0), (0, 0, -1) -- looking down at the plane z = 0"""
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = (1, 0, 0), (0, -1, 0), (0, 0, -1), eye
    return P


def wall_frames(eyes=WALL_EYES, patch_conf=None, cu=None, cv=None):
    """the fronto-parallel wall z = 0 seen from `eyes`: (frames, conf).  Every number is exact in fp32.  patch_conf: the 4 x 4 patch of
    frame 1 (rows 10..13, columns 12..15) is pulled to half its depth along its rays and given that confidence.  cu, cv: another
    principal point than WALL's."""
    g = dict(WALL, cu=WALL["cu"] if cu is None else cu, cv=WALL["cv"] if cv is None else cv)
    h, w = g["h"], g["w"]
    ys, xs = np.mgrid[0:h, 0:w]
    frames, conf = [], []
    for i, eye in enumerate(eyes):
        P = wall_pose(eye)
        depth = np.full((h, w), g["depth"], np.float64)
        c = np.full((h, w), g["conf"], F)
        if patch_conf is not None and i == g["patch"][0]:
            depth[g["patch"][1:]] = g["depth"] / 2
            c[g["patch"][1:]] = patch_conf
        cam = np.stack([(xs - g["cu"]) / g["fu"] * depth, (ys - g["cv"]) / g["fv"] * depth, depth], -1)
        pts = (cam @ P[:3, :3].T + P[:3, 3]).astype(F)
        K = np.array([[g["fu"], 0, g["cu"]], [0, g["fv"], g["cv"]], [0, 0, 1]])
        frames.append(dict(pts=pts, valid=None, K=K, cam2world=P, fu=g["fu"], fv=g["fv"], cu=g["cu"], cv=g["cv"],
                           w2c=np.linalg.inv(P)[:3].reshape(12).astype(F)))
        conf.append(c)
    return frames, conf


def order_example():
    """Three frames on the wall in which the two orders differ: (frames, conf, a, b) with a, b = (frame, row, col).
    Pixel a = (12, 16) of frame 0 is pulled to depth 1.5 along its ray and has confidence 5.  Frame 2 has confidence 9 at the pixel
    a lands on and 1 elsewhere, so a floats in front of a stronger measurement and is clipped.  The point on the same ray of frame 0
    at depth 1 is given to the pixel b of frame 1 it projects to, with confidence 3: b lands on a in frame 0, in front of it, and
    3 < 5.  Against the original confidences (parallel) b is clipped; in sequence order a already holds 0 when frame 1 is judged,
    and b is kept.  Nothing else is stronger than what it floats in front of."""
    eyes = WALL_EYES[:3]
    frames, conf = wall_frames(eyes)
    g = WALL
    a = (0, 12, 16)
    P0 = wall_pose(eyes[0])
    ray = np.array([(a[2] - g["cu"]) / g["fu"], (a[1] - g["cv"]) / g["fv"], 1.0])
    pa, pb = ((P0[:3, :3] @ (ray * depth) + P0[:3, 3]).astype(F) for depth in (1.5, 1.0))
    frames[0]["pts"][a[1], a[2]] = pa
    conf[0][a[1], a[2]] = 5.0
    r = lookup_scalar(pb, frames[1], 1e-3)
    b = (1, r[0], r[1])
    frames[1]["pts"][b[1], b[2]] = pb
    conf[1][b[1], b[2]] = 3.0
    r = lookup_scalar(pa, frames[2], 1e-3)
    conf[2][:] = 1.0
    conf[2][r[0], r[1]] = 9.0
    return frames, conf, a, b
