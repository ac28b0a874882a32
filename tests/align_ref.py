"""The rule of include/spann3r_hip.h "Global alignment" (sp3_align_loss_grad, sp3_align_moments), restated in numpy: the anchor the
kernels are checked against.  Three statements of the same loss live here:

  loss_grad_ref   vectorised numpy, every fp32 operation rounded on its own, in the header's order (the restatement);
  loss_grad_loop  the same rule as a loop over np.float32 scalars, pixel by pixel, with plain left-to-right Python-float sums;
  loss_f64        the reference's own formula (PointCloudOptimizer.forward with dist = "l1") in torch float64 with autograd, from the
                  parametrisation down: quaternion normalisation, signed_expm1, the scale factor, the adaptors, exp of log-depth.

Backend plugs the restatement into spann3r_amd.align.GlobalAligner in place of the device kernels, with the CPU oracles of the focal
and PnP steps (oracle/postprocess_oracle.py, oracle/pnp_oracle.py): the CPU path of the tests.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np
import torch

F32 = np.float32
U53 = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ tables
from spann3r_amd.align import make_items      # (the table layout is the library's; the rule below is restated)


def areas(imgs, edges):
    return [float(sum(imgs[ed["ij"][s]]["depth"].size for ed in edges)) for s in (0, 1)]


def sum_bound(count, abs_sum):
    """the bound of a reordered fp64 sum of `count` addends: count * 2^-53 * sum |addend|"""
    return count * U53 * abs_sum


# ------------------------------------------------------------------------------------------------ the restatement, vectorised
def _pixel(im):
    """the per-pixel quantities of one image, fp32 arrays [h, w]"""
    d = im["depth"].astype(F32)
    h, w = d.shape
    C = im["C"].astype(F32)
    f, cx, cy = F32(im["f"]), F32(im["cx"]), F32(im["cy"])
    u = np.broadcast_to(np.arange(w, dtype=F32)[None, :], (h, w))
    v = np.broadcast_to(np.arange(h, dtype=F32)[:, None], (h, w))
    with np.errstate(all="ignore"):
        ux, vy = u - cx, v - cy
        rx, ry = ux / f, vy / f
        xc, yc = (d * ux) / f, (d * vy) / f
        hx, hy, df = xc / f, yc / f, d / f
        X = [((C[4 * r] * xc + C[4 * r + 1] * yc) + C[4 * r + 2] * d) + C[4 * r + 3] for r in range(3)]
    return dict(d=d, C=C, rx=rx, ry=ry, xc=xc, yc=yc, hx=hx, hy=hy, df=df, X=X)


def _item(px, ed, s, Af, iA):
    """one item: the fp32 per-pixel term, g and depth-gradient addend, and the fp64 addends [15, h, w] of its image and its edge"""
    P, W = ed["P"][s].astype(F32), ed["W"][s].astype(F32)
    M, a, C = ed["M"].astype(F32), ed["a"].astype(F32), px["C"]
    with np.errstate(all="ignore"):
        q = [a[c] * P[..., c] for c in range(3)]
        Y = [((M[4 * r] * q[0] + M[4 * r + 1] * q[1]) + M[4 * r + 2] * q[2]) + M[4 * r + 3] for r in range(3)]
        r = [px["X"][c] - Y[c] for c in range(3)]
        rho = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
        term = W * rho
        k = W / rho
        g = [np.where(rho == 0, F32(0), k * r[c]) for c in range(3)]
        gc = [(g[0] * C[c] + g[1] * C[4 + c]) + g[2] * C[8 + c] for c in range(3)]
        gm = [(g[0] * M[c] + g[1] * M[4 + c]) + g[2] * M[8 + c] for c in range(3)]
        gd = ((gc[0] * px["rx"] + gc[1] * px["ry"]) + gc[2]) / F32(Af)
        gf, gpx, gpy = -(gc[0] * px["hx"] + gc[1] * px["hy"]), -(gc[0] * px["df"]), -(gc[1] * px["df"])
        one = np.ones_like(rho, dtype=np.float64)
        xh = [px["xc"].astype(np.float64), px["yc"].astype(np.float64), px["d"].astype(np.float64), one]
        qh = [q[0].astype(np.float64), q[1].astype(np.float64), q[2].astype(np.float64), one]
        G = [x.astype(np.float64) for x in g]
        img = [(G[r_] * xh[c]) * iA for r_ in range(3) for c in range(4)]
        img += [gf.astype(np.float64) * iA, gpx.astype(np.float64) * iA, gpy.astype(np.float64) * iA]
        edge = [-(G[r_] * qh[c]) * iA for r_ in range(3) for c in range(4)]
        edge += [-(gm[c].astype(np.float64) * P[..., c].astype(np.float64)) * iA for c in range(3)]
    return dict(term=term, g=g, gd=gd, img=np.stack(img), edge=np.stack(edge))


def loss_grad_ref(imgs, edges, items=None, keep_items=False):
    """imgs: list of dict(depth [h, w], C (12,), f, cx, cy); edges: list of dict(ij, P = (P_i, P_j), W = (W_i, W_j), M (12,), a (3,)).
    -> dict(gd: list of fp32 [h, w]; img [N, 15], edge [E, 15], S [2], L: fp64; img_abs / edge_abs / S_abs: the sums of |addend|;
    img_cnt / edge_cnt / S_cnt: the addend counts; with keep_items the per-item arrays too)."""
    N, E = len(imgs), len(edges)
    first, iedge, iside = items if items is not None else make_items(N, [ed["ij"] for ed in edges])
    A = areas(imgs, edges)
    out = dict(gd=[], img=np.zeros((N, 15)), edge=np.zeros((E, 15)), S=np.zeros(2), img_abs=np.zeros((N, 15)), edge_abs=np.zeros((E, 15)),
               S_abs=np.zeros(2), img_cnt=np.zeros(N), edge_cnt=np.zeros(E), S_cnt=np.zeros(2), items=[])
    with np.errstate(all="ignore"):
        for n in range(N):
            px = _pixel(imgs[n])
            gd = np.zeros_like(px["d"])
            for k in range(first[n], first[n + 1]):
                e, s = int(iedge[k]), int(iside[k])
                it = _item(px, edges[e], s, A[s], 1.0 / A[s])
                gd = gd + it["gd"]
                out["img"][n] += it["img"].sum((1, 2))
                out["img_abs"][n] += np.abs(it["img"]).sum((1, 2))
                out["edge"][e] += it["edge"].sum((1, 2))
                out["edge_abs"][e] += np.abs(it["edge"]).sum((1, 2))
                t64 = it["term"].astype(np.float64)
                out["S"][s] += t64.sum()
                out["S_abs"][s] += np.abs(t64).sum()
                out["img_cnt"][n] += t64.size
                out["edge_cnt"][e] += t64.size
                out["S_cnt"][s] += t64.size
                if keep_items:
                    out["items"].append(dict(n=n, e=e, s=s, **it))
            out["gd"].append(gd)
        out["L"] = out["S"][0] * (1.0 / A[0]) + out["S"][1] * (1.0 / A[1])
    out["A"] = A
    return out


# ------------------------------------------------------------------------------------------------ the same rule, scalar by scalar
def loss_grad_loop(imgs, edges, items=None):
    """the rule pixel by pixel on np.float32 scalars; the fp64 sums are plain left-to-right Python-float sums in (image, item, v, u)
    order -> dict(gd, term / g / gda per item (fp32 arrays), img, edge, S, L)"""
    N, E = len(imgs), len(edges)
    first, iedge, iside = items if items is not None else make_items(N, [ed["ij"] for ed in edges])
    A = areas(imgs, edges)
    img = [[0.0] * 15 for _ in range(N)]
    edge = [[0.0] * 15 for _ in range(E)]
    S = [0.0, 0.0]
    gds, its = [], []
    old = np.seterr(all="ignore")
    try:
        for n in range(N):
            im = imgs[n]
            h, w = im["depth"].shape
            C = [F32(x) for x in im["C"]]
            f, cx, cy = F32(im["f"]), F32(im["cx"]), F32(im["cy"])
            gd = np.zeros((h, w), F32)
            mine = []
            for k in range(first[n], first[n + 1]):
                mine.append(dict(n=n, e=int(iedge[k]), s=int(iside[k]), term=np.zeros((h, w), F32), g=np.zeros((3, h, w), F32),
                                 gd=np.zeros((h, w), F32)))
            for it in mine:      # item-major, so that every fp64 sum sees its addends in (item, v, u) order
                ed, s = edges[it["e"]], it["s"]
                M, a = [F32(x) for x in ed["M"]], [F32(x) for x in ed["a"]]
                Af, iA = F32(A[s]), 1.0 / A[s]
                for v in range(h):
                    for u in range(w):
                        d = F32(im["depth"][v, u])
                        ux, vy = F32(u) - cx, F32(v) - cy
                        rx, ry = ux / f, vy / f
                        xc, yc = (d * ux) / f, (d * vy) / f
                        hx, hy, df = xc / f, yc / f, d / f
                        X = [((C[4 * r] * xc + C[4 * r + 1] * yc) + C[4 * r + 2] * d) + C[4 * r + 3] for r in range(3)]
                        P = [F32(x) for x in ed["P"][s][v, u]]
                        W = F32(ed["W"][s][v, u])
                        q = [a[c] * P[c] for c in range(3)]
                        Y = [((M[4 * r] * q[0] + M[4 * r + 1] * q[1]) + M[4 * r + 2] * q[2]) + M[4 * r + 3] for r in range(3)]
                        r = [X[c] - Y[c] for c in range(3)]
                        rho = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
                        term = W * rho
                        kk = W / rho
                        g = [F32(0) if rho == 0 else kk * r[c] for c in range(3)]
                        gc = [(g[0] * C[c] + g[1] * C[4 + c]) + g[2] * C[8 + c] for c in range(3)]
                        gm = [(g[0] * M[c] + g[1] * M[4 + c]) + g[2] * M[8 + c] for c in range(3)]
                        t = ((gc[0] * rx + gc[1] * ry) + gc[2]) / Af
                        it["term"][v, u], it["gd"][v, u] = term, t
                        for c in range(3):
                            it["g"][c, v, u] = g[c]
                        xh, qh = [float(xc), float(yc), float(d), 1.0], [float(q[0]), float(q[1]), float(q[2]), 1.0]
                        for r_ in range(3):
                            for c in range(4):
                                img[n][4 * r_ + c] += (float(g[r_]) * xh[c]) * iA
                                edge[it["e"]][4 * r_ + c] += -(float(g[r_]) * qh[c]) * iA
                        img[n][12] += float(-(gc[0] * hx + gc[1] * hy)) * iA
                        img[n][13] += float(-(gc[0] * df)) * iA
                        img[n][14] += float(-(gc[1] * df)) * iA
                        for c in range(3):
                            edge[it["e"]][12 + c] += -(float(gm[c]) * float(P[c])) * iA
                        S[s] += float(term)
            for it in mine:      # the lane's own order: item after item
                gd = gd + it["gd"]
            gds.append(gd)
            its += mine
    finally:
        np.seterr(**old)
    return dict(gd=gds, items=its, img=np.array(img), edge=np.array(edge), S=np.array(S), L=S[0] * (1.0 / A[0]) + S[1] * (1.0 / A[1]))


# ------------------------------------------------------------------------------------------------ moments and the solve
def moments_ref(src, dst, w):
    """the 17 sums of sp3_align_moments in fp64 (numpy's summation order) and the sums of |addend| -> ([17], [17])"""
    p, q, w = (np.asarray(x, F32).astype(np.float64) for x in (src, dst, w))
    p, q, w = p.reshape(-1, 3), q.reshape(-1, 3), w.reshape(-1)
    wp = w[:, None] * p
    cols = [w] + [wp[:, c] for c in range(3)] + [w * q[:, c] for c in range(3)] + [wp[:, r] * q[:, c] for r in range(3) for c in range(3)]
    cols.append((wp[:, 0] * p[:, 0] + wp[:, 1] * p[:, 1]) + wp[:, 2] * p[:, 2])
    cols = np.stack(cols)
    return cols.sum(1), np.abs(cols).sum(1)


def umeyama_f64(src, dst, w):
    """the weighted similarity registration stated directly in fp64 (centred sums, not moments): dst ~ s R src + T -> (s, R, T)"""
    p, q, w = (np.asarray(x, np.float64) for x in (src, dst, w))
    p, q, w = p.reshape(-1, 3), q.reshape(-1, 3), w.reshape(-1)
    sw = w.sum()
    mp, mq = (w[:, None] * p).sum(0) / sw, (w[:, None] * q).sum(0) / sw
    pc, qc = p - mp, q - mq
    H = (w[:, None, None] * pc[:, :, None] * qc[:, None, :]).sum(0)      # sum w pc qc^T
    U, D, Vt = np.linalg.svd(H)
    sign = np.sign(np.linalg.det(Vt.T @ U.T))
    J = np.diag([1.0, 1.0, sign])
    R = Vt.T @ J @ U.T
    s = (D * np.diag(J)).sum() / (w * (pc * pc).sum(1)).sum()
    return s, R, mq - s * R @ mp


# ------------------------------------------------------------------------------------------------ the reference's formula, float64
def quat_to_R(q):
    """unit quaternion (x, y, z, w), normalised here -> rotation matrices [..., 3, 3] (torch, differentiable)"""
    q = q / q.norm(dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def signed_expm1(x):
    return torch.sign(x) * torch.expm1(torch.abs(x))


def loss_f64(params, problem, norm_pw_scale=True, base_scale=0.5, pw_break=20.0, focal_break=20.0):
    """params: dict(pw_poses [E, 8], pw_adaptors [E, 2], im_poses [N, 7], im_focals [N, 1], im_pp [N, 2], im_depthmaps: list of
    [h, w] log-depths), float64 torch tensors (requires_grad as the caller likes); problem: dict(ij, P_i, P_j, W_i, W_j: lists of
    numpy arrays, shapes: list of (h, w)).  -> L (float64 scalar tensor).  dust3r/cloud_opt/optimizer.py forward() with dist l1."""
    dt = torch.float64
    pw = params["pw_poses"]
    scale = pw[:, 7].exp()
    if norm_pw_scale:
        scale = scale * (math.log(base_scale) - pw[:, 7].mean()).exp()
    Rp, Tp = quat_to_R(pw[:, :4]), signed_expm1(pw[:, 4:7])
    ad = params["pw_adaptors"]
    ad = torch.cat((ad[:, 0:1], ad), -1)
    if norm_pw_scale:
        ad = ad - ad.mean(1, keepdim=True)
    ad = (ad / pw_break).exp()
    Ri, Ti = quat_to_R(params["im_poses"][:, :4]), signed_expm1(params["im_poses"][:, 4:7])
    focals = (params["im_focals"].reshape(-1) / focal_break).exp()
    world = []
    for n, (h, w) in enumerate(problem["shapes"]):
        pp = torch.tensor([w / 2, h / 2], dtype=dt) + 10 * params["im_pp"][n]
        d = params["im_depthmaps"][n].exp()
        u = torch.arange(w, dtype=dt)[None, :].expand(h, w)
        v = torch.arange(h, dtype=dt)[:, None].expand(h, w)
        cam = torch.stack((d * (u - pp[0]) / focals[n], d * (v - pp[1]) / focals[n], d), -1)
        world.append(cam @ Ri[n].T + Ti[n])
    ij = problem["ij"]
    A = [sum(problem["shapes"][p[s]][0] * problem["shapes"][p[s]][1] for p in ij) for s in (0, 1)]
    L = [0.0, 0.0]
    for e, pair in enumerate(ij):
        for s, (Pk, Wk) in enumerate((("P_i", "W_i"), ("P_j", "W_j"))):
            P = torch.as_tensor(np.asarray(problem[Pk][e], np.float64))
            W = torch.as_tensor(np.asarray(problem[Wk][e], np.float64))
            Y = scale[e] * ((ad[e] * P) @ Rp[e].T + Tp[e])
            L[s] = L[s] + ((world[pair[s]] - Y).norm(dim=-1) * W).sum()
    return L[0] / A[0] + L[1] / A[1]


# ------------------------------------------------------------------------------------------------ scenes
def _rot(rng, angle):
    ax = rng.standard_normal(3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def scene3(seed=0, shapes=((13, 21), (24, 32), (24, 32)), ij=None):
    """three images (13 x 21, 24 x 32, 24 x 32), six edges (complete, symmetrised), seeded; unrelated random geometry: every term is
    of order one.  About one weight in eight is exactly 0 (conf == 1 under "log").  -> (imgs, edges)"""
    rng = np.random.default_rng(seed)
    N = len(shapes)
    if ij is None:
        ij = [(i, j) for i in range(N) for j in range(N) if i != j]
    imgs = []
    for h, w in shapes:
        C = np.concatenate((_rot(rng, 0.4), rng.standard_normal((3, 1)) * 0.3), 1).reshape(12).astype(F32)
        imgs.append(dict(depth=rng.uniform(1, 3, (h, w)).astype(F32), C=C, f=F32(max(h, w) * rng.uniform(0.8, 1.4)),
                         cx=F32(w / 2 + rng.uniform(-1, 1)), cy=F32(h / 2 + rng.uniform(-1, 1))))
    edges = []
    for i, j in ij:
        P, W = [], []
        for n in (i, j):
            h, w = shapes[n]
            P.append((rng.standard_normal((h, w, 3)) * 0.5 + np.array([0, 0, 2.0])).astype(F32))
            conf = 1 + np.exp(rng.standard_normal((h, w)))
            conf[rng.random((h, w)) < 0.125] = 1.0
            W.append(np.log(conf.astype(F32)))
        s = math.exp(rng.standard_normal() * 0.2)
        M = (s * np.concatenate((_rot(rng, 0.3), rng.standard_normal((3, 1)) * 0.2), 1)).reshape(12).astype(F32)
        axy, az = math.exp(rng.standard_normal() * 0.05), math.exp(rng.standard_normal() * 0.05)
        edges.append(dict(ij=(i, j), P=P, W=W, M=M, a=np.array([axy, axy, az], F32)))
    return imgs, edges


def sheet_scene(seed=1, n_cams=4, h=24, w=32, ij=None):
    """A consistent scene: n_cams cameras on an arc look at the bumpy sheet z = 0.15 sin(3 x) cos(2 y); every depth map is the ray /
    sheet intersection (fixed-point iteration in float64).  The pair predictions are the true geometry in i's frame times a random
    per-edge scale; the confidences are smooth and above 3.  -> dict(c2w [n, 4, 4] float64, focal, pp, depth: list of [h, w] float64,
    pairs: the dict runner.pair_graph returns (pred1.pts3d, pred1.conf, pred2.pts3d_in_other_view, pred2.conf, view1.idx, view2.idx),
    scales [E])"""
    rng = np.random.default_rng(seed)
    focal, pp = 1.1 * w, (w / 2, h / 2)
    c2w, depth, cam_pts = [], [], []
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    rays = np.stack(((u - pp[0]) / focal, (v - pp[1]) / focal, np.ones_like(u)), -1)
    for n in range(n_cams):
        ang = (n - (n_cams - 1) / 2) * 0.22
        pos = np.array([2.5 * math.sin(ang), 0.1 * n, -2.5 * math.cos(ang)])
        z = -pos / np.linalg.norm(pos)
        x = np.cross([0, 1.0, 0], z)
        x /= np.linalg.norm(x)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = np.stack((x, np.cross(z, x), z), 1), pos
        dirs = rays @ T[:3, :3].T
        t = np.full((h, w), 2.5)
        for _ in range(80):      # z(pos + t dir) = sheet(x, y): a contraction, the sheet is gentle
            X = pos + t[..., None] * dirs
            t = (0.15 * np.sin(3 * X[..., 0]) * np.cos(2 * X[..., 1]) - pos[2]) / dirs[..., 2]
        c2w.append(T)
        depth.append(t)
        cam_pts.append(t[..., None] * rays)
    c2w = np.stack(c2w)
    if ij is None:
        ij = [(i, j) for i in range(n_cams) for j in range(n_cams) if i != j]
    p1, p2, c1, c2, scales = [], [], [], [], []
    for i, j in ij:
        s = math.exp(rng.uniform(-0.5, 0.5))
        rel = np.linalg.inv(c2w[i]) @ c2w[j]
        p1.append((s * cam_pts[i]).astype(F32))
        p2.append((s * (cam_pts[j] @ rel[:3, :3].T + rel[:3, 3])).astype(F32))
        base = 5 + np.sin(u / 5 + i) * np.cos(v / 4 + j)
        c1.append((base + 0.5 * rng.random((h, w))).astype(F32))
        c2.append((base + 0.5 * rng.random((h, w))).astype(F32))
        scales.append(s)
    pairs = dict(view1=dict(idx=[i for i, _ in ij]), view2=dict(idx=[j for _, j in ij]),
                 pred1=dict(pts3d=torch.from_numpy(np.stack(p1)), conf=torch.from_numpy(np.stack(c1))),
                 pred2=dict(pts3d_in_other_view=torch.from_numpy(np.stack(p2)), conf=torch.from_numpy(np.stack(c2))))
    return dict(c2w=c2w, focal=focal, pp=pp, depth=depth, pairs=pairs, scales=np.array(scales), ij=ij)


def similarity_between(poses_a, poses_b):
    """the similarity (s, R, T) that best maps the camera centres of poses_a onto those of poses_b, and the residuals after it:
    (largest centre distance, largest rotation difference |R R_a - R_b|)"""
    ca, cb = poses_a[:, :3, 3], poses_b[:, :3, 3]
    s, R, T = umeyama_f64(ca, cb, np.ones(len(ca)))
    dc = np.abs(s * ca @ R.T + T - cb).max()
    dr = max(np.abs(R @ a[:3, :3] - b[:3, :3]).max() for a, b in zip(poses_a, poses_b))
    return s, dc, dr


# ------------------------------------------------------------------------------------------------ the CPU backend of the tests
class Backend:
    """what spann3r_amd.align.GlobalAligner(backend=...) calls in place of the device kernels: the restatement, moments_ref and the
    CPU oracles of the focal and PnP steps."""

    def loss_grad(self, problem, depth_flat, C, f, pp, M, a):
        dn, Cn, fn, pn, Mn, an = (x.detach().cpu().numpy() for x in (depth_flat, C, f, pp, M, a))
        imgs, edges = [], []
        for n, (h, w) in enumerate(problem.shapes):
            o = problem.offsets[n]
            imgs.append(dict(depth=dn[o:o + h * w].reshape(h, w), C=Cn[n], f=fn[n], cx=pn[n, 0], cy=pn[n, 1]))
        for e, pair in enumerate(problem.ij):
            edges.append(dict(ij=pair, P=[problem.P[s][e].cpu().numpy() for s in (0, 1)], W=[problem.W[s][e].cpu().numpy() for s in (0, 1)],
                              M=Mn[e], a=an[e]))
        r = loss_grad_ref(imgs, edges, items=problem.items)
        loss3 = torch.tensor([r["S"][0], r["S"][1], r["L"]], dtype=torch.float64)
        gd = torch.from_numpy(np.concatenate([g.reshape(-1) for g in r["gd"]]).astype(F32))
        return loss3, gd, torch.from_numpy(r["img"]), torch.from_numpy(r["edge"])

    def moments(self, triples):
        return torch.from_numpy(np.stack([moments_ref(s.cpu().numpy(), d.cpu().numpy(), w.cpu().numpy())[0] for s, d, w in triples]))

    def focal(self, pts, pp):
        from oracle.postprocess_oracle import focal_weiszfeld
        return float(focal_weiszfeld(pts.cpu().numpy()[None].astype(np.float64), pp, min_focal=0.5, max_focal=3.5)[0])

    def pose(self, pts, focal, pp):
        from oracle.pnp_oracle import pose_c2w
        return pose_c2w(pts.cpu().numpy(), focal, pp)[0]
