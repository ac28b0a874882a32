"""spann3r_amd.evaluate: exact nearest neighbours, the metrics of spann3r/tools/eval_recon.py, k-NN PCA normals and point-to-point
ICP on the device, against tests/golden/eval_metrics.npz (tests/golden/make_golden_eval.py: the reference's own metric functions and
a float64 oracle) and tests/eval_ref.py (the scipy-free float64 oracle).

Tolerances.  Distances: the fp32 direct-difference bound of eval_ref.dist_bound, |d - d64| <= 8 * 2^-24 * max|coord| + 4 * 2^-24 * d64;
indices are checked through the float64 distance to the returned point, never by equality.  Normal consistency, normals and ICP: the
allowances the fixture stores (near-tie counts, deviation of an fp32 run of the oracle from its float64 run), as derived in
make_golden_eval.py.  Open3D is not available: ICP and estimate_normals are pinned to the oracle, not to Open3D."""
import os

import numpy as np
import pytest
import torch

import eval_ref as R
from conftest import REPO

gpu = pytest.mark.gpu
METHODS = ("grid", "brute")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "eval_metrics.npz")))


_cache = {}


def _case(name):
    """(query, ref, d64) of the NN cases whose oracle is computed here, once"""
    if name not in _cache:
        if name == "one_point":
            rng = np.random.default_rng(1)
            ref, qry = np.array([[0.25, -1.5, 3.0]], np.float32), rng.normal(0, 2, (5, 3)).astype(np.float32)
        elif name == "copies":
            rng = np.random.default_rng(2)
            ref, qry = np.tile(np.array([[1.0, 2.0, -0.5]], np.float32), (1000, 1)), rng.normal(0, 2, (7, 3)).astype(np.float32)
            qry[0] = ref[0]
        elif name == "planar":
            ref, qry = R.planar_pair()
        elif name == "clusters":
            ref, qry = R.cluster_pair()
        _cache[name] = (qry, ref, R.nn_brute(qry, ref)[0])
    return _cache[name]


def _check_nn(qry, ref, d64, dist, idx):
    dist, idx = dist.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    bound = R.dist_bound(d64, R.max_coord(qry, ref))
    assert dist.shape == d64.shape and idx.shape == d64.shape
    assert idx.min() >= 0 and idx.max() < len(ref)
    err = np.abs(dist - d64)
    print("worst |d - d64| / bound = %.3f" % float((err / bound).max()))
    assert np.all(err <= bound)
    to_idx = np.linalg.norm(qry.astype(np.float64) - ref.astype(np.float64)[idx], axis=-1)
    assert np.all(to_idx <= d64 + bound)


# ------------------------------------------------------------------------------------------------ CPU
def test_eval_ref_reproduces_the_reference_metrics(fx):
    """the scipy-free oracle equals what the reference's eval_recon.py (cKDTree) gave on the main pair"""
    gt, rec = R.main_pair()
    assert np.array_equal(gt, fx["gt"]) and np.array_equal(rec, fx["rec"])
    d_acc, _ = R.nn_brute(rec, gt)
    d_comp, _ = R.nn_brute(gt, rec)
    assert np.abs(d_acc - fx["d_acc"]).max() <= 1e-12 and np.abs(d_comp - fx["d_comp"]).max() <= 1e-12
    gt_n, rec_n = fx["gt_normals"].astype(np.float32).astype(np.float64), fx["rec_normals_f32"].astype(np.float64)
    for got, ref in ((R.accuracy(gt, rec, gt_n, rec_n), fx["ref_accuracy"]), (R.completion(gt, rec, gt_n, rec_n), fx["ref_completion"])):
        np.testing.assert_allclose(np.array(got), ref, rtol=4e-16, atol=0)
    assert R.accuracy(gt, rec) == R.accuracy(gt, rec, gt_n, rec_n)[:2]
    assert R.completion_ratio(gt, rec) == fx["ref_completion_ratio"]
    ur, uq = R.uniform_pair()
    assert np.array_equal(fx["uniform_checksum"], [ur.astype(np.float64).sum(), uq.astype(np.float64).sum()])


def test_choose_grid_handles_degenerate_boxes():
    from spann3r_amd.evaluate import choose_grid, MAX_CELLS
    assert choose_grid([1, 1, 1], [1, 1, 1], 1000)[1] == (1, 1, 1)                       # one point / copies
    h, dims = choose_grid([0, 0, 0], [1, 1, 0], 4096)                                    # planar: a 2-D grid of ~4 points per cell
    assert dims[2] == 1 and 24 <= dims[0] <= 40 and dims[0] == dims[1]
    h, dims = choose_grid([0, 0, 0], [5, 0, 0], 100)                                     # collinear
    assert dims[1:] == (1, 1) and 20 <= dims[0] <= 30
    h, dims = choose_grid([0, 0, 0], [1, 1, 1], 1 << 26)                                 # the cell cap binds
    assert dims[0] * dims[1] * dims[2] <= MAX_CELLS and h > (4.0 / (1 << 26)) ** (1 / 3)
    h, dims = choose_grid([0, 0, 0], [1e3, 1e3, 1e3], 4000)
    assert dims[0] * dims[1] * dims[2] <= 2 * 4000


def test_cell_table_keeps_the_order_inside_a_cell_and_spans_empty_cells():
    from spann3r_amd.cell_grid import cell_table, grow_to_cap
    ids = torch.tensor([4, 0, 1, 4, 0, 1, 0], dtype=torch.int32)        # 6 cells: 2 and 3 (in the middle) and 5 (at the end) are empty
    order, start = cell_table(ids, 6)
    assert order.tolist() == [1, 4, 6, 2, 5, 0, 3]                       # stable: the items of a cell keep their order
    assert start.dtype == torch.int32 and start.tolist() == [0, 3, 5, 5, 5, 7, 7]
    order, start = cell_table(torch.zeros(3, dtype=torch.int32), 1)      # the grid of one cell
    assert order.tolist() == [0, 1, 2] and start.tolist() == [0, 3]
    assert grow_to_cap([1.0, 1.0, 0.0], 0.25) == (0.25, (5, 5, 1))       # under the cap: h as given
    h, dims = grow_to_cap([1.0, 1.0, 1.0], 0.125, max_cells=100)         # 9^3 > 100: h grows by 1.25 until the cap holds
    assert dims[0] * dims[1] * dims[2] <= 100 and h == 0.125 * 1.25 ** 4 and dims == (4, 4, 4)


# ------------------------------------------------------------------------------------------------ GPU: NN exactness
@gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["one_point", "copies", "planar", "clusters"])
def test_nn_small_and_degenerate_clouds(name, method):
    from spann3r_amd.evaluate import nearest_neighbors
    qry, ref, d64 = _case(name)
    dist, idx = nearest_neighbors(qry, ref, method=method)
    _check_nn(qry, ref, d64, dist, idx)


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_nn_main_pair_with_far_outliers(fx, method):
    from spann3r_amd.evaluate import nearest_neighbors
    dist, idx, stats = nearest_neighbors(torch.from_numpy(fx["rec"]).cuda(), torch.from_numpy(fx["gt"]).cuda(), method=method, return_stats=True)
    _check_nn(fx["rec"], fx["gt"], fx["d_acc"], dist, idx)
    print(stats)
    if method == "grid":
        assert 0 < stats["fallback_queries"] <= 50 + 25        # the 50 points moved far outside the box go to the second pass


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_nn_uniform_20k(fx, method):
    from spann3r_amd.evaluate import nearest_neighbors
    ref, qry = R.uniform_pair()
    dist, idx, stats = nearest_neighbors(qry, ref, method=method, return_stats=True)
    _check_nn(qry, ref, fx["uniform_d"], dist, idx)
    print(stats)
    if method == "grid":
        assert stats["fallback_queries"] == 0
        assert stats["grid"][0] * stats["grid"][1] * stats["grid"][2] > 1000


@gpu
def test_nn_walk_without_a_ring_budget_on_a_flat_grid():
    """The ring walk alone, to its end: a flat grid (nz = 1, nx != ny), queries inside the box and outside it on every side and
    beyond every corner, out to 3 extents, and no ring budget, so that rings beyond the usual 3 and the exit taken when the walked
    block covers the whole grid (bound +inf) give the answer instead of the brute-force stage."""
    from spann3r_amd.evaluate import nearest_neighbors
    rng = np.random.default_rng(11)
    ext = np.array([4.0, 2.0, 0.0])
    ref = (rng.uniform(0, 1, (600, 3)) * ext).astype(np.float32)
    inside = rng.uniform(0, 1, (128, 3)) * ext
    outside = np.empty((0, 3))
    while len(outside) < 128:                        # uniform over the box pushed out by 3 extents (of x, for z), the box itself cut out
        c = rng.uniform(-3, 4, (512, 3)) * np.array([4.0, 2.0, 4.0])
        outside = np.concatenate([outside, c[((c[:, :2] < 0) | (c[:, :2] > ext[:2])).any(1)]])[:128]
    side = np.sign(outside[:, :2] - ext[:2] / 2) * ((outside[:, :2] < 0) | (outside[:, :2] > ext[:2]))
    assert len({tuple(s) for s in side.tolist()}) == 8                    # four sides, four corners
    qry = np.concatenate([inside, outside]).astype(np.float32)
    dist, idx, stats = nearest_neighbors(qry, ref, ring_budget=1 << 20, return_stats=True)
    print(stats)
    nx, ny, nz = stats["grid"]
    assert nz == 1 and nx != ny and min(nx, ny) > 2 * 3 + 1               # a block of 3 rings cannot cover the grid
    assert stats["fallback_queries"] == 0                                 # the walk alone answered
    _check_nn(qry, ref, R.nn_brute(qry, ref)[0], dist, idx)
    assert nearest_neighbors(qry, ref, return_stats=True)[2]["fallback_queries"] > 0      # and needed more than the usual 3 rings


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_nn_max_dist(fx, method):
    from spann3r_amd.evaluate import nearest_neighbors
    d64 = fx["d_acc"]
    assert not np.any(np.abs(d64 - 0.05) <= R.dist_bound(d64, R.max_coord(fx["rec"], fx["gt"])))     # no borderline query (generator)
    dist, idx = nearest_neighbors(fx["rec"], fx["gt"], max_dist=0.05, method=method)
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    far = d64 > 0.05
    assert far.sum() >= 50 and (~far).sum() > 1000
    assert np.array_equal(idx == -1, far) and np.all(np.isposinf(dist[far]))
    _check_nn(fx["rec"][~far], fx["gt"], d64[~far], torch.from_numpy(dist[~far]), torch.from_numpy(idx[~far]))


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_knn_30_on_the_cloud_itself(fx, method):
    from spann3r_amd.evaluate import nearest_neighbors
    gt = fx["gt"]
    if "knn" not in _cache:
        _cache["knn"] = R.knn_brute(gt, gt, 30)[0]
    d64 = _cache["knn"]
    dist, idx = nearest_neighbors(gt, gt, k=30, method=method)
    dist, idx = dist.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    assert dist.shape == (6000, 30) and idx.shape == (6000, 30)
    assert np.all(dist[:, 0] == 0) and np.array_equal(idx[:, 0], np.arange(6000))
    assert np.all(np.diff(dist, axis=1) >= 0)
    bound = R.dist_bound(d64, R.max_coord(gt))
    assert np.all(np.abs(dist - d64) <= bound)
    to_idx = np.linalg.norm(gt.astype(np.float64)[:, None] - gt.astype(np.float64)[idx], axis=-1)
    assert np.all(np.abs(to_idx - dist) <= bound)            # every returned index is the point its distance speaks of
    assert all(len(set(row)) == 30 for row in idx[::97])


# ------------------------------------------------------------------------------------------------ GPU: metrics
@gpu
def test_metrics_match_the_reference_dump(fx):
    from spann3r_amd.evaluate import accuracy, completion, completion_ratio
    gt, rec = torch.from_numpy(fx["gt"]).cuda(), torch.from_numpy(fx["rec"]).cuda()
    gt_n, rec_n = fx["gt_normals"].astype(np.float32), fx["rec_normals_f32"]
    mc = R.max_coord(fx["gt"], fx["rec"])
    m_acc, m_comp = (int(v) for v in fx["near_ties"])
    for fn, ref, m, n, window in ((accuracy, fx["ref_accuracy"], m_acc, 5000, fx["nc1_median_window"]),
                                  (completion, fx["ref_completion"], m_comp, 6000, fx["nc2_median_window"])):
        plain = fn(gt, rec)
        full = fn(gt, rec, gt_n, rec_n)
        print(fn.__name__, full, ref.tolist())
        assert len(plain) == 2 and len(full) == 4 and all(type(v) is float for v in full) and plain == full[:2]
        assert abs(full[0] - ref[0]) <= R.dist_bound(ref[0], mc) and abs(full[1] - ref[1]) <= R.dist_bound(ref[1], mc)
        assert abs(full[2] - ref[2]) <= m / n + 1e-6
        assert window[0] - 1e-6 <= full[3] <= window[1] + 1e-6
    ratio = completion_ratio(gt, rec)
    assert type(ratio) is float and ratio == float(fx["ref_completion_ratio"])


@gpu
def test_estimate_normals_against_the_float64_oracle(fx):
    from spann3r_amd.evaluate import estimate_normals
    n = estimate_normals(torch.from_numpy(fx["gt"]).cuda(), knn=30)
    assert n.shape == (6000, 3) and n.dtype == torch.float32
    n = n.cpu().numpy().astype(np.float64)
    dev = 1.0 - np.abs(np.sum(n * fx["gt_normals"], -1))
    print("worst 1 - |n . n_ref| = %.3e, allowed %.3e (4 x the fp32 run of the oracle)" % (dev.max(), 4 * float(fx["normals_fp32_dev"])))
    assert dev.max() <= 4 * float(fx["normals_fp32_dev"])
    few = estimate_normals(fx["gt"][:2])
    assert np.array_equal(few.cpu().numpy(), [[0, 0, 1], [0, 0, 1]])


# ------------------------------------------------------------------------------------------------ GPU: ICP
@gpu
@pytest.mark.parametrize("tag", ["a", "b"])
def test_icp_against_the_float64_oracle(fx, tag):
    from spann3r_amd.evaluate import icp_point_to_point
    src, n = fx["icp_src_" + tag], 3000
    T, fitness, rmse, it = icp_point_to_point(src, torch.from_numpy(fx["gt"]).cuda(), 0.1)
    T0 = fx["icp_%s_T" % tag]
    rot_tol, trans_tol = 4 * float(fx["icp_%s_rot_dev" % tag]), 4 * float(fx["icp_%s_trans_dev" % tag])
    rot, trans = R.rot_angle(T[:3, :3], T0[:3, :3]), float(np.linalg.norm(T[:3, 3] - T0[:3, 3]))
    print("case %s: rot %.3e (allowed %.3e), trans %.3e (allowed %.3e), fitness %r, rmse %r, iterations %d (oracle %d)"
          % (tag, rot, rot_tol, trans, trans_tol, fitness, rmse, it, int(fx["icp_%s_iterations" % tag])))
    assert T.shape == (4, 4) and T.dtype == np.float64 and np.array_equal(T[3], [0, 0, 0, 1])
    assert rot <= rot_tol and trans <= trans_tol
    assert abs(fitness - float(fx["icp_%s_fitness" % tag])) <= int(fx["icp_%s_borderline" % tag]) / n
    assert abs(it - int(fx["icp_%s_iterations" % tag])) <= 1
    if tag == "a":
        M = T @ fx["icp_motion"]                      # independent of the oracle: the recovered motion undoes the known one
        rot_i, trans_i = R.rot_angle(M[:3, :3], np.eye(3)), float(np.linalg.norm(M[:3, 3]))
        print("case a: T . motion vs identity: rot %.3e, trans %.3e" % (rot_i, trans_i))
        assert rot_i <= rot_tol and trans_i <= trans_tol
    else:
        assert fitness < 1.0


@gpu
def test_icp_without_matches_returns_init():
    from spann3r_amd.evaluate import icp_point_to_point
    init = R.rigid((0, 0, 1), 10.0, (0.5, 0, 0))
    src, tgt = R.surface_cloud(100, 11), R.surface_cloud(100, 12) + np.float32(50.0)
    T, fitness, rmse, it = icp_point_to_point(src, tgt, 0.1, init=init)
    assert np.array_equal(T, init) and fitness == 0.0 and it == 0


@gpu
def test_evaluate_reconstruction(fx):
    from spann3r_amd import evaluate as E
    pred, gt = torch.from_numpy(fx["icp_src_b"]).cuda(), torch.from_numpy(fx["gt"]).cuda()
    out = E.evaluate_reconstruction(pred, gt, threshold=0.1)
    assert set(out) == {"acc", "comp", "nc1", "nc2", "acc_med", "comp_med", "nc1_med", "nc2_med", "transformation"}
    T = out["transformation"]
    assert R.rot_angle(T[:3, :3], fx["icp_b_T"][:3, :3]) <= 4 * float(fx["icp_b_rot_dev"])
    moved = (fx["icp_src_b"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    acc, acc_med = E.accuracy(gt, moved)
    comp, comp_med = E.completion(gt, moved)
    mc = R.max_coord(moved, fx["gt"])
    for k, v in (("acc", acc), ("acc_med", acc_med), ("comp", comp), ("comp_med", comp_med)):
        assert abs(out[k] - v) <= R.dist_bound(v, mc), k
    assert all(0.0 <= out[k] <= 1.0 for k in ("nc1", "nc2", "nc1_med", "nc2_med")) and out["nc2"] > 0.9


# ------------------------------------------------------------------------------------------------ errors, determinism
@gpu
def test_error_cases(fx):
    from spann3r_amd.evaluate import nearest_neighbors, estimate_normals
    gt = torch.from_numpy(fx["gt"]).cuda()
    with pytest.raises(ValueError, match="empty"):
        nearest_neighbors(gt, gt[:0])
    with pytest.raises(RuntimeError, match="GPU"):
        nearest_neighbors(torch.from_numpy(fx["gt"]), gt)
    with pytest.raises(ValueError, match="1..32"):
        nearest_neighbors(gt, gt, k=33)
    with pytest.raises(ValueError, match="1..32"):
        estimate_normals(gt, knn=33)
    with pytest.raises(ValueError, match="shape"):
        nearest_neighbors(gt[:, :2], gt)


@gpu
def test_nn_is_deterministic(fx):
    from spann3r_amd.evaluate import nearest_neighbors
    a = nearest_neighbors(fx["rec"], fx["gt"])
    b = nearest_neighbors(fx["rec"], fx["gt"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a = nearest_neighbors(fx["gt"], fx["gt"], k=30)
    b = nearest_neighbors(fx["gt"], fx["gt"], k=30)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
