"""A scipy-free float64 oracle for spann3r_amd.evaluate: chunked brute-force nearest neighbours, the metric formulas of
spann3r/tools/eval_recon.py:4-39, k-NN PCA normals and point-to-point ICP.  tests/golden/make_golden_eval.py runs the same
ICP / normals code with scipy's cKDTree as the neighbour search and stores the results in tests/golden/eval_metrics.npz.

The seeded clouds of the tests are built here too, so that the generator and the tests use the same ones."""
import numpy as np

EPS32 = 2.0 ** -24


def dist_bound(d64, max_coord):
    """|d_fp32 - d64| for direct differences in fp32: the three subtractions, squares and sums and the square root each
    round once (relative 2^-24); the coordinates themselves are exact fp32 inputs."""
    return 8 * EPS32 * max_coord + 4 * EPS32 * np.asarray(d64, np.float64)


def max_coord(*clouds):
    return max(float(np.abs(np.asarray(c, np.float64)).max()) for c in clouds)


def knn_brute(query, ref, k=1, dtype=np.float64, chunk=256):
    """k nearest neighbours by direct differences in `dtype` -> (dist [N, k], idx [N, k]) ascending; ties by lower index."""
    q, r = np.asarray(query, dtype), np.asarray(ref, dtype)
    k = min(k, len(r))
    dist, idx = np.empty((len(q), k), dtype), np.empty((len(q), k), np.int64)
    for s in range(0, len(q), chunk):
        d = q[s:s + chunk, None, :] - r[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        if k == 1:
            part = np.argmin(d2, axis=1)[:, None]
        else:
            part = np.argpartition(d2, k - 1, axis=1)[:, :k]
            sub = np.take_along_axis(d2, part, 1)
            part = np.take_along_axis(part, np.lexsort((part, sub), axis=1), 1)
        idx[s:s + chunk] = part
        dist[s:s + chunk] = np.sqrt(np.take_along_axis(d2, part, 1))
    return dist, idx


def nn_brute(query, ref, dtype=np.float64):
    d, i = knn_brute(query, ref, 1, dtype)
    return d[:, 0], i[:, 0]


# ------------------------------------------------------------------------------------------------ eval_recon.py:4-39
def completion_ratio(gt_points, rec_points, dist_th=0.05, nn=nn_brute):
    d, _ = nn(gt_points, rec_points)
    return np.mean((d < dist_th).astype(np.float32))


def accuracy(gt_points, rec_points, gt_normals=None, rec_normals=None, nn=nn_brute):
    d, idx = nn(rec_points, gt_points)
    if gt_normals is None or rec_normals is None:
        return np.mean(d), np.median(d)
    dots = np.abs(np.sum(gt_normals[idx] * rec_normals, axis=-1))
    return np.mean(d), np.median(d), np.mean(dots), np.median(dots)


def completion(gt_points, rec_points, gt_normals=None, rec_normals=None, nn=nn_brute):
    d, idx = nn(gt_points, rec_points)
    if gt_normals is None or rec_normals is None:
        return np.mean(d), np.median(d)
    dots = np.abs(np.sum(gt_normals * rec_normals[idx], axis=-1))
    return np.mean(d), np.median(d), np.mean(dots), np.median(dots)


# ------------------------------------------------------------------------------------------------ normals, ICP
def pca_normals(points, nbr, dtype=np.float64):
    """unit eigenvector of the smallest eigenvalue of the covariance of points[nbr[i]] about their mean; also the eigenvalues"""
    p = np.asarray(points, dtype)[nbr]
    c = p - p.mean(1, keepdims=True)
    w, v = np.linalg.eigh(np.einsum("nki,nkj->nij", c, c))
    return v[:, :, 0], w


def rigid(axis, angle_deg, t):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(angle_deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = t
    return T


def rot_angle(Ra, Rb):
    """angle of Ra Rb^T, from the skew part (accurate near zero)"""
    R = Ra @ Rb.T
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(np.linalg.norm(s), 0.5 * (np.trace(R) - 1.0)))


def kabsch(p, q):
    """R, t minimising sum |R p + t - q|^2 (SVD, reflection fixed) -> 4x4"""
    mp, mq = p.mean(0), q.mean(0)
    U, _, Vt = np.linalg.svd((q - mq).T @ (p - mp))
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    T = np.eye(4)
    T[:3, :3] = U @ S @ Vt
    T[:3, 3] = mq - T[:3, :3] @ mp
    return T


def icp(source, target, max_dist, nn=nn_brute, fp32_points=False, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """Point-to-point ICP from identity in float64 (the rule of spann3r_amd.evaluate.icp_point_to_point) -> T, fitness, rmse,
    iterations, and the per-evaluation NN distances of the last evaluation.  fp32_points: the transformed source is rounded to
    fp32 before it is matched and summed, as the device path does."""
    src, tgt = np.asarray(source, np.float64), np.asarray(target, np.float64)

    def evaluate(T):
        moved = src @ T[:3, :3].T + T[:3, 3]
        if fp32_points:
            moved = moved.astype(np.float32).astype(np.float64)
        d, idx = nn(moved, tgt)
        ok = d <= max_dist
        if not ok.any():
            return moved, idx, ok, 0.0, 0.0, d
        e = moved[ok] - tgt[idx[ok]]
        return moved, idx, ok, ok.sum() / len(src), float(np.sqrt((e * e).sum() / ok.sum())), d

    T = np.eye(4)
    moved, idx, ok, fitness, rmse, d = evaluate(T)
    it = 0
    while it < max_iteration and ok.any():
        it += 1
        T = kabsch(moved[ok], tgt[idx[ok]]) @ T
        moved, idx, ok, f2, r2, d = evaluate(T)
        stop = abs(f2 - fitness) < relative_fitness and abs(r2 - rmse) < relative_rmse
        fitness, rmse = f2, r2
        if stop:
            break
    return T, float(fitness), float(rmse), it, np.asarray(d, np.float64)


# ------------------------------------------------------------------------------------------------ the seeded clouds
def surface_cloud(n, seed):
    """n points of z = 0.3 sin(3u) cos(2v), (u, v) uniform over [-1, 1]^2"""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-1, 1, (2, n))
    return np.stack((u, v, 0.3 * np.sin(3 * u) * np.cos(2 * v)), 1).astype(np.float32)


def main_pair(seed=0, n_gt=6000, n_rec=5000, n_far=50):
    """gt on the surface; rec = its first n_rec points plus N(0, 0.01) noise, the first n_far of them moved by +5 on every axis"""
    gt = surface_cloud(n_gt, seed)
    rng = np.random.default_rng(seed + 1000)
    rec = gt[:n_rec].astype(np.float64) + rng.normal(0, 0.01, (n_rec, 3))
    rec[:n_far] += 5.0
    return gt, rec.astype(np.float32)


def planar_pair():
    rng = np.random.default_rng(3)
    ref = np.concatenate((rng.uniform(-2, 3, (4097, 2)), np.zeros((4097, 1))), 1).astype(np.float32)
    qry = np.concatenate((rng.uniform(-2.5, 3.5, (3001, 2)), rng.normal(0, 0.2, (3001, 1))), 1).astype(np.float32)
    return ref, qry


def cluster_pair():
    """two tight clusters of 2000 points 10^3 apart; queries around both and in between"""
    rng = np.random.default_rng(5)
    c = np.array([[0.0, 0.0, 0.0], [1000.0, 0.0, 0.0]])
    ref = np.concatenate([ci + rng.normal(0, 0.05, (2000, 3)) for ci in c]).astype(np.float32)
    qry = np.concatenate([ci + rng.normal(0, 0.1, (150, 3)) for ci in c] + [rng.uniform(0, 1000, (11, 1)) * np.array([[1.0, 0.0, 0.0]])])
    return ref, qry.astype(np.float32)


def uniform_pair(n=20000):
    rng = np.random.default_rng(6)
    return rng.random((n, 3)).astype(np.float32), rng.random((n, 3)).astype(np.float32)


ICP_MOTION = rigid((1.0, 2.0, 3.0), 5.0, (0.03, -0.02, 0.01))


def icp_sources(gt):
    """case A: 3000 points of gt under ICP_MOTION; case B: the same plus N(0, 0.005) noise, 10 % of them moved by +5"""
    rng = np.random.default_rng(7)
    sel = np.sort(rng.choice(len(gt), 3000, replace=False))
    a = gt[sel].astype(np.float64) @ ICP_MOTION[:3, :3].T + ICP_MOTION[:3, 3]
    b = a + rng.normal(0, 0.005, a.shape)
    b[:300] += 5.0
    return a.astype(np.float32), b.astype(np.float32)
