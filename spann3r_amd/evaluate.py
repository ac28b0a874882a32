"""Reconstruction metrics of eval.py on the device (reference: eval.py:189-231, spann3r/tools/eval_recon.py:4-39).

The reference scores a scene on the CPU: Open3D's point-to-point ICP of the predicted cloud onto the ground truth, Open3D's
`estimate_normals` of both, then accuracy / completion / normal consistency through scipy's cKDTree.  Everything here rests on one
primitive, exact nearest-neighbour search between two clouds (csrc/eval.hip: a cell grid over the reference cloud walked ring by
ring, an LDS-tiled brute-force kernel for the queries the rings do not settle); distances, covariances and sums are HIP, torch
provides memory, `torch.sort` (cell ids, medians) and `torch.searchsorted` (the cell-start table).

`accuracy`, `completion` and `completion_ratio` are pinned to the reference's own functions (tests/golden/eval_metrics.npz).
Open3D is not available to the tests: `icp_point_to_point` and `estimate_normals` implement the algorithms Open3D documents
(registration_icp with TransformationEstimationPointToPoint; k-NN PCA normals) and are pinned to a float64 restatement --
parity with Open3D itself is unpinned."""
import ctypes as C
import math

import numpy as np
import torch

from . import cell_grid
from . import lib as L
from .cell_grid import MAX_CELLS, choose_grid      # noqa: F401 -- re-exported: their public home was here

KNN_MAX = 32
RING_BUDGET = 3          # rings walked before a query is handed to the brute-force kernel
_read_counters = cell_grid.read_head      # tools/bench_eval_metrics.py reads the head through this name


def _cloud(x, name):
    """fp32 [N, 3] on the device: numpy arrays are moved there, CPU tensors are refused (as elsewhere in the package)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to("cuda")
    elif not isinstance(x, torch.Tensor):
        raise TypeError("%s: expected a CUDA tensor or a numpy array, got %s" % (name, type(x).__name__))
    elif not x.is_cuda:
        raise RuntimeError("%s: the metrics run on the GPU (HIP kernels); there is no CPU path -- pass a CUDA tensor or a numpy array" % name)
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError("%s: expected shape [N, 3], got %s" % (name, tuple(x.shape)))
    return x.contiguous().float()


class CellGrid(cell_grid.Grid):
    """The reference cloud binned for searching: records sorted by cell id, the cell-start table, the grid descriptor."""

    def __init__(self, ref, brute=False):
        lib = L.load()
        self.ref = ref
        self.m = m = ref.shape[0]
        dev = ref.device
        self.recs = torch.empty(m, 4, dtype=torch.float32, device=dev)
        if brute:                                    # one cell, records in caller order: what the brute-force kernels read
            self.g = cell_grid.one_cell()
            self.cell_start = torch.tensor([0, m], dtype=torch.int32, device=dev)
            L.check(lib.sp3_nn_pack_records(ref.data_ptr(), 0, m, self.recs.data_ptr(), L.stream_ptr()), "sp3_nn_pack_records")
            return
        box = cell_grid.finite_box(*torch.aminmax(ref, dim=0))
        h, dims = choose_grid(box[0], box[1], m)
        self.g = cell_grid.make_grid(box, h, dims)
        ids = torch.empty(m, dtype=torch.int32, device=dev)
        L.check(lib.sp3_nn_cell_ids(ref.data_ptr(), m, C.byref(self.g), ids.data_ptr(), L.stream_ptr()), "sp3_nn_cell_ids")
        order, self.cell_start = cell_grid.cell_table(ids, dims[0] * dims[1] * dims[2])
        L.check(lib.sp3_nn_pack_records(ref.data_ptr(), order.data_ptr(), m, self.recs.data_ptr(), L.stream_ptr()), "sp3_nn_pack_records")

    def nn(self, q, max_dist=math.inf, ring_budget=RING_BUDGET, ws=None):
        """1-NN of q [N, 3] -> dist fp32 [N], idx int32 [N], ws (its first 32 bytes hold the counters of this call)"""
        lib = L.load()
        n = q.shape[0]
        dist = torch.empty(n, dtype=torch.float32, device=q.device)
        idx = torch.empty(n, dtype=torch.int32, device=q.device)
        if ws is None:
            ws = torch.empty(lib.sp3_nn_query_ws_bytes(n), dtype=torch.uint8, device=q.device)
        order = self.query_order(q)
        L.check(lib.sp3_nn_query(q.data_ptr(), order.data_ptr(), n, self.recs.data_ptr(), self.cell_start.data_ptr(), self.m, C.byref(self.g),
                                 int(ring_budget), float(max_dist), ws.data_ptr(), dist.data_ptr(), idx.data_ptr(), L.stream_ptr()), "sp3_nn_query")
        return dist, idx, ws

    def nn_brute(self, q, max_dist=math.inf):
        lib = L.load()
        n = q.shape[0]
        dist = torch.empty(n, dtype=torch.float32, device=q.device)
        idx = torch.empty(n, dtype=torch.int32, device=q.device)
        ws = torch.empty(lib.sp3_nn_query_ws_bytes(n), dtype=torch.uint8, device=q.device)
        L.check(lib.sp3_nn_brute(q.data_ptr(), n, self.recs.data_ptr(), self.m, float(max_dist), ws.data_ptr(), dist.data_ptr(), idx.data_ptr(),
                                 L.stream_ptr()), "sp3_nn_brute")
        return dist, idx

    def knn(self, q, k, max_dist=math.inf, sort_queries=True):
        lib = L.load()
        n = q.shape[0]
        dist = torch.empty(n, k, dtype=torch.float32, device=q.device)
        idx = torch.empty(n, k, dtype=torch.int32, device=q.device)
        order = self.query_order(q) if sort_queries else None
        L.check(lib.sp3_knn_query(q.data_ptr(), L.ptr(order), n, self.recs.data_ptr(), self.cell_start.data_ptr(), self.m, C.byref(self.g), int(k),
                                  float(max_dist), dist.data_ptr(), idx.data_ptr(), L.stream_ptr()), "sp3_knn_query")
        return dist, idx


def nearest_neighbors(query, ref, k=1, max_dist=None, method="grid", return_stats=False, ring_budget=RING_BUDGET):
    """Exact nearest neighbours of every query point among ref -> (dist fp32, idx int32), [N] for k = 1, [N, k] ascending for
    k > 1 (k <= 32).  max_dist: neighbours farther than it are reported as index -1, distance +inf.
    method: "grid" (cell grid + brute-force second pass for what `ring_budget` rings leave open) or "brute" (the brute-force
    kernel for every query; for k > 1 the k-NN kernel over a grid of one cell) -- the in-tree cross-check.
    return_stats: also a dict with `fallback_queries` (served by the second pass), `cells_visited`, `points_visited`, `grid`, `h`."""
    if method not in ("grid", "brute"):
        raise ValueError("nearest_neighbors: method must be 'grid' or 'brute', got %r" % (method,))
    if not 1 <= int(k) <= KNN_MAX:
        raise ValueError("nearest_neighbors: k = %r, must be 1..%d" % (k, KNN_MAX))
    k = int(k)
    q, r = _cloud(query, "query"), _cloud(ref, "ref")
    if r.shape[0] == 0:
        raise ValueError("nearest_neighbors: ref is empty")
    md = math.inf if max_dist is None else float(max_dist)
    if md < 0:
        raise ValueError("nearest_neighbors: max_dist must be non-negative")
    n = q.shape[0]
    stats = {"fallback_queries": 0, "cells_visited": 0, "points_visited": 0, "grid": (1, 1, 1), "h": None}
    if n == 0:
        shape = (0,) if k == 1 else (0, k)
        out = torch.empty(shape, dtype=torch.float32, device=q.device), torch.empty(shape, dtype=torch.int32, device=q.device)
        return out + (stats,) if return_stats else out
    grid = CellGrid(r, brute=(method == "brute"))
    if k > 1:
        dist, idx = grid.knn(q, k, md, sort_queries=(method == "grid"))
        stats["fallback_queries"] = n if method == "brute" else 0
    elif method == "brute":
        dist, idx = grid.nn_brute(q, md)
        stats["fallback_queries"] = n
    else:
        dist, idx, ws = grid.nn(q, md, ring_budget)
        if return_stats:
            stats["fallback_queries"], stats["cells_visited"], stats["points_visited"] = _read_counters(ws)
    if method == "grid":
        stats["grid"], stats["h"] = (grid.g.nx, grid.g.ny, grid.g.nz), float(grid.g.h)
    return (dist, idx, stats) if return_stats else (dist, idx)


# ------------------------------------------------------------------------------------------------ eval_recon.py:4-39
def _sum_count(x, thresh):
    """device double [2] = (sum x, #(x < thresh)), fp64 partial slabs in a fixed order"""
    lib = L.load()
    n = x.numel()
    ws = torch.empty(lib.sp3_sum_count_ws_bytes(n), dtype=torch.uint8, device=x.device)
    out = torch.empty(2, dtype=torch.float64, device=x.device)
    L.check(lib.sp3_sum_count_f32(x.data_ptr(), n, float(thresh), ws.data_ptr(), out.data_ptr(), L.stream_ptr()), "sp3_sum_count_f32")
    return out


def _mean_median(x):
    """(mean, median) of a device fp32 vector as Python floats; numpy's median rule (mean of the two middle values for an even count)"""
    n = x.numel()
    s = torch.sort(x)[0]
    got = torch.cat((_sum_count(x, 0.0)[:1], s[(n - 1) // 2:n // 2 + 1].double())).cpu().numpy()
    return float(got[0] / n), float((got[1] + got[-1]) / 2.0)


def _nn_with_normals(tree_pts, query_pts, na, nb, gather_a, what):
    tree, q = _cloud(tree_pts, what + ": tree cloud"), _cloud(query_pts, what + ": query cloud")
    if tree.shape[0] == 0 or q.shape[0] == 0:
        raise ValueError(what + ": empty cloud")
    dist, idx, _ = CellGrid(tree).nn(q)
    out = _mean_median(dist)
    if na is not None and nb is not None:
        na, nb = _cloud(na, what + ": gt_normals"), _cloud(nb, what + ": rec_normals")
        n = q.shape[0]
        if (na.shape[0], nb.shape[0]) != ((tree.shape[0], n) if gather_a else (n, tree.shape[0])):
            raise ValueError(what + ": normals do not match their clouds")
        dots = torch.empty(n, dtype=torch.float32, device=q.device)
        L.check(L.load().sp3_normal_dot(na.data_ptr(), nb.data_ptr(), idx.data_ptr(), n, int(gather_a), dots.data_ptr(), L.stream_ptr()),
                "sp3_normal_dot")
        out = out + _mean_median(dots)
    return out


def accuracy(gt_points, rec_points, gt_normals=None, rec_normals=None):
    """eval_recon.py:11-24: distances from every reconstructed point to its nearest ground-truth point ->
    (mean, median) or, with normals, (mean, median, mean |n_gt[idx] . n_rec|, median of the same)."""
    return _nn_with_normals(gt_points, rec_points, gt_normals, rec_normals, True, "accuracy")


def completion(gt_points, rec_points, gt_normals=None, rec_normals=None):
    """eval_recon.py:27-39: distances from every ground-truth point to its nearest reconstructed point ->
    (mean, median) or, with normals, (mean, median, mean |n_gt . n_rec[idx]|, median of the same)."""
    return _nn_with_normals(rec_points, gt_points, gt_normals, rec_normals, False, "completion")


def completion_ratio(gt_points, rec_points, dist_th=0.05):
    """eval_recon.py:4-8: the share of ground-truth points whose nearest reconstructed point is closer than dist_th (a float32
    mean of 0 / 1 there, so the float32 quotient here)."""
    rec, gt = _cloud(rec_points, "completion_ratio: rec_points"), _cloud(gt_points, "completion_ratio: gt_points")
    if rec.shape[0] == 0 or gt.shape[0] == 0:
        raise ValueError("completion_ratio: empty cloud")
    dist, _, _ = CellGrid(rec).nn(gt)
    count = float(_sum_count(dist, dist_th)[1].item())
    return float(np.float32(count) / np.float32(gt.shape[0]))


# ------------------------------------------------------------------------------------------------ eval.py:203-212
def estimate_normals(points, knn=30):
    """Unit normals [N, 3] (device fp32) from the PCA of every point's knn nearest neighbours, itself included (what Open3D's
    `estimate_normals(KDTreeSearchParamKNN(knn))` documents; eval.py:211-212 uses its default, 30).  Sign is unconstrained;
    fewer than 3 points give (0, 0, 1).  Parity with Open3D itself is unpinned."""
    if not 1 <= int(knn) <= KNN_MAX:
        raise ValueError("estimate_normals: knn = %r, must be 1..%d" % (knn, KNN_MAX))
    pts = _cloud(points, "points")
    n = pts.shape[0]
    out = torch.empty(n, 3, dtype=torch.float32, device=pts.device)
    if n == 0:
        return out
    _, idx = CellGrid(pts).knn(pts, int(knn))
    L.check(L.load().sp3_knn_normals(pts.data_ptr(), idx.data_ptr(), n, int(knn), out.data_ptr(), L.stream_ptr()), "sp3_knn_normals")
    return out


def _transform(pts, T, out=None):
    out = torch.empty_like(pts) if out is None else out
    if pts.shape[0]:
        rt = (C.c_double * 12)(*T[:3, :3].reshape(-1).tolist(), *T[:3, 3].tolist())
        L.check(L.load().sp3_transform_points(pts.data_ptr(), pts.shape[0], rt, out.data_ptr(), L.stream_ptr()), "sp3_transform_points")
    return out


def kabsch_update(s):
    """The rigid motion that best maps the matched source points onto their targets, from the 17 sums of sp3_icp_accum
    (Umeyama without scale, reflection fixed) -> 4x4 float64."""
    n = s[0]
    mp, mq = s[1:4] / n, s[4:7] / n
    cov = (s[7:16].reshape(3, 3) / n - np.outer(mp, mq)).T          # sum (q - mq)(p - mp)^T / n
    U, _, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    T = np.eye(4)
    T[:3, :3] = U @ S @ Vt
    T[:3, 3] = mq - T[:3, :3] @ mp
    return T


def icp_point_to_point(source, target, max_dist, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """Point-to-point ICP as Open3D documents `registration_icp(source, target, max_dist, init,
    TransformationEstimationPointToPoint())` -> (T [4, 4] float64 numpy, fitness, inlier_rmse, iterations).
    Every evaluation matches each transformed source point to its nearest target point within max_dist (fitness = matches /
    source points, rmse = sqrt(sum d^2 / matches)); every iteration applies the Kabsch update of the current matches,
    T <- update . T, and re-evaluates; it stops when |d fitness| and |d rmse| are both below their criteria.  The loop reads
    back 17 doubles per evaluation; the 3x3 SVD runs on the host in float64.  Parity with Open3D itself is unpinned."""
    lib = L.load()
    src, tgt = _cloud(source, "source"), _cloud(target, "target")
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64).reshape(4, 4)
    n = src.shape[0]
    if n == 0 or tgt.shape[0] == 0:
        return T, 0.0, 0.0, 0
    grid = CellGrid(tgt)
    moved = torch.empty_like(src)
    ws_nn = torch.empty(lib.sp3_nn_query_ws_bytes(n), dtype=torch.uint8, device=src.device)
    ws_acc = torch.empty(lib.sp3_icp_accum_ws_bytes(n), dtype=torch.uint8, device=src.device)
    sums = torch.empty(17, dtype=torch.float64, device=src.device)

    def evaluate(T):
        _transform(src, T, moved)
        _, idx, _ = grid.nn(moved, max_dist, ws=ws_nn)
        L.check(lib.sp3_icp_accum(moved.data_ptr(), tgt.data_ptr(), idx.data_ptr(), n, ws_acc.data_ptr(), sums.data_ptr(), L.stream_ptr()),
                "sp3_icp_accum")
        s = sums.cpu().numpy()
        if s[0] == 0:
            return s, 0.0, 0.0
        return s, float(s[0] / n), float(math.sqrt(s[16] / s[0]))

    s, fitness, rmse = evaluate(T)
    if s[0] == 0:
        return T, 0.0, 0.0, 0
    it = 0
    while it < max_iteration:
        it += 1
        T = kabsch_update(s) @ T
        s, f2, r2 = evaluate(T)
        stop = (abs(f2 - fitness) < relative_fitness and abs(r2 - rmse) < relative_rmse) or s[0] == 0
        fitness, rmse = f2, r2
        if stop:
            break
    return T, fitness, rmse, it


def evaluate_reconstruction(pred_points, gt_points, threshold=0.1):
    """eval.py:203-218 on already-masked clouds: ICP of the prediction onto the ground truth from identity, the prediction
    transformed, normals of both clouds, accuracy and completion with normal consistency."""
    pred, gt = _cloud(pred_points, "pred_points"), _cloud(gt_points, "gt_points")
    T, _, _, _ = icp_point_to_point(pred, gt, threshold)
    pred = _transform(pred, T)
    pred_n, gt_n = estimate_normals(pred), estimate_normals(gt)
    acc, acc_med, nc1, nc1_med = accuracy(gt, pred, gt_n, pred_n)
    comp, comp_med, nc2, nc2_med = completion(gt, pred, gt_n, pred_n)
    return {"acc": acc, "comp": comp, "nc1": nc1, "nc2": nc2, "acc_med": acc_med, "comp_med": comp_med, "nc1_med": nc1_med,
            "nc2_med": nc2_med, "transformation": T}


def _exact_side(points, normals, target_mesh, face_normals, bvh=None):
    """points (with their normals) against the TRIANGLES of target_mesh -> (mean, median of the distances, mean, median of
    |n_point . n_face| with the unit normal of the face each closest point lies on)"""
    from . import mesh as M
    r = M.point_mesh_distance(points, target_mesh, bvh=bvh)
    n = points.shape[0]
    dots = torch.empty(n, dtype=torch.float32, device=points.device)
    L.check(L.load().sp3_normal_dot(face_normals.data_ptr(), normals.data_ptr(), r["face"].data_ptr(), n, 1, dots.data_ptr(), L.stream_ptr()),
            "sp3_normal_dot")
    return _mean_median(r["dist"]) + _mean_median(dots)


def evaluate_meshes(pred_mesh, gt_mesh, n_samples=200_000, seed=0, threshold=0.1, icp=True, exact=False, accel=None, cull_views=None):
    """The metrics of evaluate_reconstruction for two SURFACES instead of two clouds, as NICE-SLAM-style eval_recon scripts take
    them: n_samples points drawn by area from each mesh (mesh.sample_surface: the dicts of scene_mesh / extract_mesh / simplify,
    the same seed for both), point-to-point ICP of the prediction's samples onto the ground truth's from identity unless
    icp=False, the prediction's points moved by T and its normals rotated by T's rotation, then accuracy and completion with the
    SAMPLED normals -- the exact unit normals of the faces drawn; no k-NN PCA.  The numbers no longer depend on where a
    tessellation put its vertices.  -> the dict of evaluate_reconstruction plus pred_area, gt_area (the quantised areas) and
    samples.  A mesh without area raises ValueError.
    exact=True measures every sample against the other mesh's TRIANGLES instead of against its samples (mesh.point_mesh_distance;
    include/spann3r_hip.h "Mesh distance"): acc = the prediction's samples to the ground truth's faces, comp = the ground truth's
    samples to the prediction's faces, its vertices moved by T; nc1 / nc2 = |n_sample . n_face| with the unit normal of the face
    hit (mesh.face_frames; rotated by T's rotation for the prediction).  Sampling and ICP are unchanged.  The floor the sample
    spacing puts under acc / comp is gone: two tessellations of one plane score 0.  The dict gains exact=True.
    accel (with exact=True only): "grid" (the default: mesh.TriangleGrid, fastest when the prediction lies within a few cells of
    the ground truth) or "bvh" (mesh.TriangleBVH: the same numbers bit for bit, at a cost that does not depend on how far apart
    the two surfaces are -- the choice for a prediction that may be poor, and for meshes of wildly mixed face sizes).
    cull_views: a dict of the camera arguments of mesh.cull_to_views (intrinsics, cam2world, size and any of near, far, bias,
    pixel_offset, opengl, cull, mode, min_views): both meshes are first culled to what those cameras could see, each against its
    own surface (include/spann3r_hip.h "Mesh visibility") -- the cull_mesh step of NICE-SLAM-style protocols, without which rooms
    the sequence never entered ruin comp and hallucinated back sides ruin acc.  The dict gains pred_faces_kept and gt_faces_kept.
    With accel="bvh" the shadow rays walk a tree too.  None: nothing new runs."""
    from . import mesh as M
    if accel is not None and not exact:
        raise ValueError("evaluate_meshes: accel=%r chooses the structure of the exact distance: pass exact=True" % (accel,))
    if accel not in (None, "grid", "bvh"):
        raise ValueError("evaluate_meshes: accel must be 'grid' or 'bvh', got %r" % (accel,))
    bvh = True if accel == "bvh" else None
    n = int(n_samples)
    if n <= 0:
        raise ValueError("evaluate_meshes: n_samples = %r, must be positive" % (n_samples,))
    kept = {}
    if cull_views is not None:
        pred_mesh, gt_mesh = (M.cull_to_views(x, bvh=bvh, **cull_views) for x in (pred_mesh, gt_mesh))
        kept = dict(pred_faces_kept=pred_mesh["visibility"]["faces_kept"], gt_faces_kept=gt_mesh["visibility"]["faces_kept"])
    sp, sg = M.sample_surface(pred_mesh, n, seed=seed), M.sample_surface(gt_mesh, n, seed=seed)
    pred, pred_n, gt, gt_n = sp["points"], sp["normals"], sg["points"], sg["normals"]
    T = np.eye(4)
    R = np.eye(4)
    if icp:
        T, _, _, _ = icp_point_to_point(pred, gt, threshold)
        R[:3, :3] = T[:3, :3]
        pred, pred_n = _transform(pred, T), _transform(pred_n, R)
    if exact:
        pred_fn, gt_fn = M.face_frames(pred_mesh)["face_normals"], M.face_frames(gt_mesh)["face_normals"]
        moved = pred_mesh
        if icp:
            moved = dict(vertices=_transform(pred_mesh["vertices"].contiguous().float(), T), faces=pred_mesh["faces"])
            pred_fn = _transform(pred_fn, R)
        acc, acc_med, nc1, nc1_med = _exact_side(pred, pred_n, gt_mesh, gt_fn, bvh)
        comp, comp_med, nc2, nc2_med = _exact_side(gt, gt_n, moved, pred_fn, bvh)
    else:
        acc, acc_med, nc1, nc1_med = accuracy(gt, pred, gt_n, pred_n)
        comp, comp_med, nc2, nc2_med = completion(gt, pred, gt_n, pred_n)
    out = {"acc": acc, "comp": comp, "nc1": nc1, "nc2": nc2, "acc_med": acc_med, "comp_med": comp_med, "nc1_med": nc1_med,
           "nc2_med": nc2_med, "transformation": T, "pred_area": sp["area"], "gt_area": sg["area"], "samples": n}
    if exact:
        out["exact"] = True
    out.update(kept)
    return out


def evaluate_depth(m, views, near=0.0, far=math.inf, bvh=None):
    """A surface scored in image space against the depth of an RGB-D sequence, the usual companion of acc / comp: the mesh dict `m`
    rendered from every view's `camera_intrinsics` / `camera_pose` at its `depthmap` size (mesh.render_depth_maps: rays against the
    mesh on the device, all views in one launch; include/spann3r_hip.h "Mesh rays") and compared with `depthmap` on `valid_mask`.
    -> dict(abs_rel = mean |p - g| / g, rmse = sqrt(mean (p - g)^2), delta1 = the share of pixels with max(p / g, g / p) < 1.25 --
    all three over the valid_mask pixels the mesh hits -- coverage = the share of valid_mask pixels the mesh hits, its own number,
    pixels = how many were compared, views).  The views of views.build_views, batch size 1 each or stacked; landscape views only,
    as fusion.fuse_views.  Sums are fp64 reductions on the device; one host read.  No pixel to compare gives NaN errors.
    bvh: a mesh.TriangleBVH built on `m`, or True to build one: the rays walk it instead of a TriangleGrid, the same depth maps."""
    from . import mesh as M
    if len(views) == 0:
        raise ValueError("evaluate_depth: no views")
    dev = m["vertices"].device
    gt = torch.cat([v["depthmap"].to(dev) for v in views]).float()
    valid = torch.cat([v["valid_mask"].to(dev) for v in views]).bool()
    if gt.dim() != 3 or valid.shape != gt.shape:
        raise RuntimeError("evaluate_depth: mismatched shapes: depthmap %s, valid_mask %s" % (tuple(gt.shape), tuple(valid.shape)))
    K = torch.cat([v["camera_intrinsics"] for v in views]).double().cpu().numpy()
    poses = torch.cat([v["camera_pose"] for v in views]).double().cpu().numpy()
    pred = M.render_depth_maps(m, K, poses, gt.shape[1:], near=near, far=far, bvh=bvh)["depth"]
    hit = valid & (pred > 0)
    p, g = pred.double(), gt.double()
    g = torch.where(hit, g, torch.ones_like(g))
    p = torch.where(hit, p, torch.ones_like(p))
    diff = p - g
    ratio = torch.maximum(p / g, g / p)
    sums = torch.stack([valid.sum().double(), hit.sum().double(), (diff.abs() / g).sum(), (diff * diff).sum(),
                        (hit & (ratio < 1.25)).sum().double()]).cpu().tolist()
    nv, nh = sums[0], sums[1]
    nan = float("nan")
    return dict(abs_rel=sums[2] / nh if nh else nan, rmse=math.sqrt(sums[3] / nh) if nh else nan, delta1=sums[4] / nh if nh else nan,
                coverage=nh / nv if nv else nan, pixels=int(nh), views=int(gt.shape[0]))


def _align(views, preds, preds_all, clouds):
    from .loss import L21, Regr3D_t_ScaleShiftInv, _entries
    n = len(views)
    if len(preds) != n:
        raise ValueError("align_to_ground_truth: %d views but %d predictions" % (n, len(preds)))
    if views[0]["pts3d"].shape[0] != 1:
        raise ValueError("align_to_ground_truth: batch size 1 only (one sequence at a time, as the reference's eval.py), got %d"
                         % views[0]["pts3d"].shape[0])
    crit = Regr3D_t_ScaleShiftInv(L21, norm_mode=False, gt_scale=True)
    P, G, pose0, stats = crit.align_stats(views, preds_all)
    dev = P.device
    H, W = views[0]["pts3d"].shape[1:3]
    HW = H * W
    ent = _entries(n)
    # eval.py:146: the left prediction of every frame but the last, the right prediction of the last pair for the last frame
    pick = [next(e for e, (s, side) in enumerate(ent) if s == j and side == 0) for j in range(n - 1)] + [len(ent) - 1]
    Psel = P[pick].contiguous()
    pts, gt = torch.empty(n, H, W, 3, device=dev), torch.empty(n, H, W, 3, device=dev)
    masks = torch.cat([v["valid_mask"].to(dev) for v in views]).contiguous()
    conf = torch.cat([p["conf"].to(dev).float() for p in preds]).contiguous()
    img = torch.cat([v["img"].to(dev, torch.float32) for v in views]).contiguous()
    images = torch.empty(n, H, W, 3, device=dev)
    lib = L.load()
    ws = torch.empty(int(lib.sp3_eval_align_ws_bytes(n * HW)) // 4 + 1, dtype=torch.int32, device=dev)
    cp, cg, cc = (torch.empty(n * HW, 3, device=dev) for _ in range(3))
    src = torch.empty(n * HW, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(lib.sp3_eval_align(Psel.data_ptr(), n, G.data_ptr(), n, 1, HW, pose0.data_ptr(), stats.data_ptr(), 1, pts.data_ptr(),
                               gt.data_ptr(), masks.view(torch.uint8).data_ptr(), img.data_ptr(), ws.data_ptr(), images.data_ptr(),
                               cp.data_ptr(), cg.data_ptr(), cc.data_ptr(), src.data_ptr(), count.data_ptr(), L.stream_ptr()),
            "sp3_eval_align")
    out = dict(pts_all=pts, pts_gt_all=gt, masks_all=masks, images_all=images, conf_all=conf)
    if clouds:
        k = int(count.item())
        out.update(pred_cloud=cp[:k], gt_cloud=cg[:k], cloud_colors=cc[:k], cloud_index=src[:k])
    return out


def align_to_ground_truth(views, preds, preds_all):
    """eval.py:128-168 on the device for one sequence (batch size 1): the predictions, shift- and scale-aligned to the ground truth by
    `Regr3D_t_ScaleShiftInv(L21, norm_mode=False, gt_scale=True).get_all_pts3d_t`'s medians, and the ground truth, both with
    gt_shift_z added back and in the world of view 0's camera pose.  views: spann3r_amd.views.build_views (or the reference's
    batch); preds, preds_all: Spann3R.forward.  -> dict of pts_all, pts_gt_all [n, H, W, 3], masks_all [n, H, W] bool,
    images_all [n, H, W, 3] in [0, 1], conf_all [n, H, W], all on the device."""
    return _align(views, preds, preds_all, False)


def evaluate_sequence(views, preds, preds_all, threshold=0.1):
    """eval.py:128-218 for one sequence: align_to_ground_truth, the masked clouds (eval.py:189-191, in the reference's order: ICP and
    the k-NN normals are order-sensitive at ties) by a compaction on the device, then evaluate_reconstruction.  Returns that
    function's dict plus pred_cloud, gt_cloud, cloud_colors [N, 3] and cloud_index [N] (the pixel each point came from)."""
    a = _align(views, preds, preds_all, True)
    if a["pred_cloud"].shape[0] == 0:
        raise ValueError("evaluate_sequence: no valid pixel in any view (the masks are all false): nothing to evaluate")
    if not bool(torch.isfinite(a["pred_cloud"]).all()):
        raise ValueError("evaluate_sequence: non-finite predicted points under the valid masks")
    out = evaluate_reconstruction(a["pred_cloud"], a["gt_cloud"], threshold)
    out.update({k: a[k] for k in ("pred_cloud", "gt_cloud", "cloud_colors", "cloud_index")})
    return out
