"""sp3_mesh_tri_cell_count / _fill, sp3_mesh_dist_query and sp3_mesh_dist_brute on the device (csrc/mesh_distance.hip;
include/spann3r_hip.h "Mesh distance") and what drives them: mesh.TriangleGrid / point_mesh_distance and
evaluate.evaluate_meshes(exact=True).

The anchor is tests/mesh_distance_ref.py (the numpy restatement, checked against exact rationals and a pair-by-pair loop in
tests/test_mesh_distance_cpu.py).  Every comparison with it is exact: dist and closest bit for bit, face and region equal.  The
result is a pure function of the inputs, so the grid walk, the brute-force kernels and the restatement must agree whatever the grid."""
import math
import sys

import numpy as np
import pytest
import torch

import bricks_ref as BR
import mesh_distance_ref as R
import raycast_ref as RC

pytestmark = pytest.mark.gpu

S = BR.SCENE


def _t(x):
    return torch.from_numpy(np.array(x)).cuda()


def _mesh(verts, faces):
    return dict(vertices=_t(np.asarray(verts, np.float32).reshape(-1, 3)), faces=_t(np.asarray(faces, np.int32).reshape(-1, 3)), bounds=None)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _assert_same(got, want, what=""):
    """a device result dict (or a second one) against the restatement's: bit for bit"""
    g = {k: (got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]) for k in ("dist", "closest", "face", "region")}
    w = {k: (want[k].cpu().numpy() if isinstance(want[k], torch.Tensor) else want[k]) for k in ("dist", "closest", "face", "region")}
    assert g["dist"].dtype == np.float32 and g["closest"].dtype == np.float32 and g["face"].dtype == np.int32 and g["region"].dtype == np.uint8
    assert g["closest"].shape == (len(g["dist"]), 3)
    bad = np.flatnonzero(g["face"] != w["face"])
    assert len(bad) == 0, "%s: %d faces differ, first at query %d: %d vs %d" % (what, len(bad), bad[0], g["face"][bad[0]], w["face"][bad[0]])
    assert np.array_equal(g["region"], w["region"]), what
    assert np.array_equal(_bits(g["dist"]), _bits(w["dist"])), what
    assert np.array_equal(_bits(g["closest"]), _bits(w["closest"])), what


def _check(m, verts, faces, queries, want=None, grid=None, what=""):
    """grid walk == brute force == restatement for these queries; -> (the grid result with stats, the restatement)"""
    from spann3r_amd import mesh as M
    want = R.query(queries, verts, faces) if want is None else want
    q = _t(np.asarray(queries, np.float32))
    got = M.point_mesh_distance(q, m, grid=grid, return_stats=True)
    _assert_same(got, want, what + " grid")
    _assert_same(M.point_mesh_distance(q, m, method="brute"), want, what + " brute")
    return got, want


# ------------------------------------------------------------------------------------------------ 1. one triangle, every region
TRI_V = np.array([(0, 0, 0), (2, 0, 0), (0, 2, 0)], np.float32)
TRI_F = np.array([[0, 1, 2]], np.int32)
TRI_Q = np.array([(-1, -1, 0.5), (3, -0.5, 0.25), (1, -1, 1), (-0.5, 3, -0.25), (-1, 1, -1), (2, 2, 0.5), (0.5, 0.5, 0.75),      # regions 0..6
                  (0.5, 0.5, 0), (0.25, 1.25, 0),                                                       # in the plane, inside
                  (1, 0, 0), (0, 0.5, 0), (1, 1, 0),                                                     # exactly on each edge
                  (0, 0, 0), (2, 0, 0), (0, 2, 0),                                                       # exactly at each vertex
                  (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)], np.float32)                           # no winner


def test_one_triangle_in_every_region():
    from spann3r_amd import mesh as M
    m = _mesh(TRI_V, TRI_F)
    got, want = _check(m, TRI_V, TRI_F, TRI_Q, what="triangle")
    assert want["region"][:7].tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert (want["dist"][7:15] == 0).all() and (want["face"][:15] == 0).all()
    assert want["face"][15:].tolist() == [-1] * 3 and want["region"][15:].tolist() == [255] * 3 and np.isinf(want["dist"][15:]).all()
    assert got["stats"]["grid"] != (1, 1, 1) and got["stats"]["pairs"] >= 1            # F = 1 through the cells ...
    one = M.TriangleGrid(m, h=100.0)                                                   # ... and through a grid of one cell
    assert one.dims == (1, 1, 1) and one.pairs == 0 and one.usable == 1
    got1, _ = _check(m, TRI_V, TRI_F, TRI_Q, want=want, grid=one, what="one cell")
    assert got1["stats"]["fallback_queries"] == len(TRI_Q)


# ------------------------------------------------------------------------------------------------ 2. the bumpy sheet
def _sheet(n=32):
    y, x = np.mgrid[:n, :n]
    verts = np.stack([x / (n - 1) + 0.003, y / (n - 1) - 0.5, 0.05 * np.sin(x * 0.9) * np.cos(y * 0.7)], -1).reshape(-1, 3).astype(np.float32)
    tl = (y[:-1, :-1] * n + x[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([tl, tl + 1, tl + n], 1), np.stack([tl + 1, tl + n + 1, tl + n], 1)]).astype(np.int32)
    return verts, faces


@pytest.fixture(scope="module")
def sheet():
    """(verts, faces, queries, the restatement's answer): 2048 queries within 0.005 of the surface, 1024 inside the box, 1024 outside it
    by up to 1000 extents"""
    verts, faces = _sheet()
    rng = np.random.default_rng(5)
    f = faces[rng.integers(0, len(faces), 2048)]
    w = rng.dirichlet((1, 1, 1), 2048)
    near = (verts[f] * w[:, :, None]).sum(1) + rng.uniform(-0.005, 0.005, (2048, 3))
    lo, hi = verts.min(0), verts.max(0)
    inside = rng.uniform(lo, hi, (1024, 3))
    direction = rng.normal(size=(1024, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    outside = (lo + hi) / 2 + direction * (10.0 ** rng.uniform(0, 3, (1024, 1)))
    q = np.concatenate([near, inside, outside]).astype(np.float32)
    return verts, faces, q, R.query(q, verts, faces)


def test_the_bumpy_sheet_grid_brute_and_restatement(sheet):
    from spann3r_amd import mesh as M
    verts, faces, q, want = sheet
    assert len(faces) == 2 * 31 * 31 and len(np.unique(want["region"])) == 7
    m = _mesh(verts, faces)
    grid = M.TriangleGrid(m)
    assert grid.usable == len(faces) and grid.pairs <= M.PAIRS_PER_FACE_CAP * len(faces) and np.prod(grid.dims) > 27
    got, _ = _check(m, verts, faces, q, want=want, grid=grid, what="sheet")
    print("sheet: grid %s h %.4f pairs %d (%d tries), %d fallbacks, %.1f faces evaluated per query" %
          (grid.dims, grid.h, grid.pairs, grid.tries, got["stats"]["fallback_queries"], got["stats"]["faces_evaluated"] / len(q)))
    # the near queries (within 0.005 sqrt 3 of the surface) settle inside the ring budget: after ring 2 every wall is 2 h away
    assert grid.h > 0.005
    near = M.point_mesh_distance(_t(q[:2048]), m, grid=grid, return_stats=True)
    assert near["stats"]["fallback_queries"] == 0 and near["stats"]["faces_evaluated"] > 0 and near["stats"]["cells_visited"] >= 2048
    _assert_same(near, {k: want[k][:2048] for k in want}, "near")
    # no ring budget: what the home cell does not settle goes to the brute-force kernels, and nothing changes
    r0 = M.point_mesh_distance(_t(q), m, grid=grid, return_stats=True, ring_budget=0)
    assert 0 < r0["stats"]["fallback_queries"] < len(q)
    _assert_same(r0, want, "ring budget 0")
    # the same bits a second time
    again = M.point_mesh_distance(_t(q), m, grid=grid)
    assert all(torch.equal(again[k], got[k]) for k in ("dist", "closest", "face", "region"))


def test_the_walk_without_a_ring_budget_answers_every_query():
    """No ring budget: rings beyond the usual 3 and the exit taken when the walked block covers the whole grid (bound +inf) give the
    answer, for queries near the surface, inside the box and outside it by up to 10 extents; nothing reaches the brute-force kernels."""
    from spann3r_amd import mesh as M
    verts, faces = _sheet(12)
    assert len(faces) == 242
    rng = np.random.default_rng(6)
    f = faces[rng.integers(0, len(faces), 64)]
    near = (verts[f] * rng.dirichlet((1, 1, 1), 64)[:, :, None]).sum(1) + rng.uniform(-0.005, 0.005, (64, 3))
    lo, hi = verts.min(0), verts.max(0)
    inside = rng.uniform(lo, hi, (64, 3))
    direction = rng.normal(size=(64, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    outside = (lo + hi) / 2 + direction * (hi - lo).max() * rng.uniform(1, 10, (64, 1))
    q = np.concatenate([near, inside, outside]).astype(np.float32)
    want = R.query(q, verts, faces)
    m = _mesh(verts, faces)
    grid = M.TriangleGrid(m)
    print("grid", grid.dims, "h", grid.h, "pairs", grid.pairs)
    assert max(grid.dims) > 2 * 3 + 1                                                  # a block of 3 rings cannot cover the grid
    got = M.point_mesh_distance(_t(q), m, grid=grid, ring_budget=1 << 20, return_stats=True)
    print(got["stats"])
    assert got["stats"]["fallback_queries"] == 0                                       # the walk alone answered
    _assert_same(got, want, "no ring budget")
    _assert_same(got, M.point_mesh_distance(_t(q), m, method="brute"), "no ring budget against brute")
    assert M.point_mesh_distance(_t(q), m, grid=grid, return_stats=True)["stats"]["fallback_queries"] > 0      # and needed more than 3 rings


# ------------------------------------------------------------------------------------------------ 3. faces that must never win
def test_unusable_faces_among_good_ones():
    from spann3r_amd import mesh as M
    rng = np.random.default_rng(21)
    nv = 300
    verts = rng.normal(size=(nv, 3)).astype(np.float32)
    verts[10], verts[11], verts[12] = (2, 4, 6), (1, 2, 3), (3, 6, 9)               # collinear, exactly: zero area
    verts[20, 1] = np.nan
    verts[21, 2] = np.inf
    good = rng.integers(30, nv, (900, 3)).astype(np.int32)
    good = good[(good[:, 0] != good[:, 1]) & (good[:, 1] != good[:, 2]) & (good[:, 0] != good[:, 2])]
    bad = np.array([[10, 11, 12], [12, 10, 11], [40, 40, 41], [42, 43, 42], [44, 44, 44], [-1, 50, 51], [50, nv, 51], [50, 51, 2 ** 31 - 1],
                    [-2 ** 31, 50, 51], [20, 60, 61], [60, 21, 61], [20, 21, 62]], np.int32)
    where = np.sort(rng.choice(len(good), len(bad), replace=False))
    faces = np.insert(good, where, bad, axis=0)
    is_bad = np.ones(len(faces), bool)
    is_bad[np.setdiff1d(np.arange(len(faces)), where + np.arange(len(bad)))] = False
    assert np.array_equal(R.usable(verts, faces), ~is_bad)
    q = np.concatenate([rng.normal(size=(500, 3)), verts[[10, 11, 12, 40, 42, 44, 50]], [[2.5, 5, 7.5]]]).astype(np.float32)
    m = _mesh(verts, faces)
    grid = M.TriangleGrid(m)
    assert grid.usable == len(good)
    got, want = _check(m, verts, faces, q, grid=grid, what="degenerates")
    assert not is_bad[want["face"]].any() and np.isfinite(want["dist"]).all()
    # the same mesh without them: the same distances and points, the faces renumbered
    clean = M.point_mesh_distance(_t(q), _mesh(verts, good))
    assert torch.equal(clean["dist"], got["dist"]) and torch.equal(clean["closest"], got["closest"]) and torch.equal(clean["region"], got["region"])
    assert np.array_equal(np.flatnonzero(~is_bad)[clean["face"].cpu().numpy()], want["face"])


# ------------------------------------------------------------------------------------------------ 4. ties and permutations
def test_ties_take_the_smallest_index_and_permuted_faces_leave_the_distance_alone(sheet):
    from spann3r_amd import mesh as M
    verts, faces, q, want = sheet
    twice = np.concatenate([faces[:40][::-1], faces[:40], faces[:40]])               # every face three times, the first copy reversed
    qq = q[:512]
    got, ref = _check(_mesh(verts, twice), verts, twice, qq, what="copies")
    f = ref["face"]
    assert (f < 80).all() and (f[(f >= 40)] < 80).all()
    # the winner is the FIRST position among its three copies
    pos = {tuple(r): i for i, r in reversed(list(enumerate(map(tuple, twice))))}
    assert all(pos[tuple(twice[i])] == i for i in f)
    perm = np.random.default_rng(3).permutation(len(faces))
    shuffled = np.ascontiguousarray(faces[perm])
    a = M.point_mesh_distance(_t(q), _mesh(verts, shuffled))
    assert np.array_equal(_bits(a["dist"].cpu().numpy()), _bits(want["dist"]))
    # the face may differ only where another face reaches the same d2 (a shared edge or vertex)
    moved = perm[a["face"].cpu().numpy()] != want["face"]
    assert (want["region"][moved] != 6).all()


# ------------------------------------------------------------------------------------------------ 5. face sizes that differ 64-fold
def _plane(mirror):
    """a plane of 2 x 1 units: a 64 x 64 grid of cells on one half, two triangles on the other (tests/test_mesh_sample_gpu.py)"""
    g = 64
    y, x = np.mgrid[:g + 1, :g + 1]
    v = np.stack([x / g, y / g, np.zeros_like(x, float)], -1).reshape(-1, 3)
    tl = (y[:-1, :-1] * (g + 1) + x[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([tl, tl + 1, tl + g + 2], 1), np.stack([tl, tl + g + 2, tl + g + 1], 1)])
    n, c10, c11 = len(v), g, g * (g + 1) + g
    v = np.concatenate([v, [[2, 0, 0], [2, 1, 0]]]).astype(np.float32)
    f = np.concatenate([f, [[c10, n, n + 1], [c10, n + 1, c11]]])
    if mirror:
        v[:, 0] = np.float32(2) - v[:, 0]
        f = f[:, ::-1]
    return v, np.ascontiguousarray(f).astype(np.int32)


def test_mixed_face_sizes_keep_the_pair_cap():
    from spann3r_amd import mesh as M
    verts, faces = _plane(False)
    m = _mesh(verts, faces)
    grid = M.TriangleGrid(m)
    print("mixed sizes: grid %s h %.4f pairs %d for %d faces after %d tries" % (grid.dims, grid.h, grid.pairs, len(faces), grid.tries))
    assert 0 < grid.pairs <= M.PAIRS_PER_FACE_CAP * len(faces) and grid.dims[2] == 1      # (also the flat mesh: one cell thick)
    fine = M.TriangleGrid(m, h=1 / 256)                                                # cells far below the two large faces: the cap grows h
    assert fine.tries > 1 and fine.pairs <= M.PAIRS_PER_FACE_CAP * len(faces) and fine.h > 1 / 256
    rng = np.random.default_rng(8)
    q = np.concatenate([rng.uniform((-0.2, -0.2, -0.3), (2.2, 1.2, 0.3), (384, 3)), rng.uniform((0, 0, 0), (2, 1, 0), (128, 3))]).astype(np.float32)
    got, want = _check(m, verts, faces, q, grid=grid, what="mixed")
    assert (want["face"] >= len(faces) - 2).sum() > 100 and (want["face"] < len(faces) - 2).sum() > 100
    _assert_same(M.point_mesh_distance(_t(q), m, grid=fine), want, "mixed, grown h")
    over = (q[:, 0] >= 0) & (q[:, 0] <= 2) & (q[:, 1] >= 0) & (q[:, 1] <= 1)
    off = over & (np.abs(q[:, 2]) > 1e-3)
    assert off.sum() > 100 and np.array_equal(want["dist"][off], np.abs(q[off, 2]))   # over the plane: |z|, to the bit
    assert (want["dist"][-128:] < 1e-12).all()                                        # in it: the fp64 rounding of the closest point


# ------------------------------------------------------------------------------------------------ 6. empty sizes and argument errors
def test_empty_sizes_and_argument_errors():
    from spann3r_amd import lib as L, mesh as M
    m = _mesh(TRI_V, TRI_F)
    for method in ("grid", "brute"):
        r = M.point_mesh_distance(torch.empty((0, 3), device="cuda"), m, method=method, return_stats=True)
        assert r["dist"].shape == (0,) and r["closest"].shape == (0, 3) and r["face"].shape == (0,) and r["region"].shape == (0,)
        assert (r["dist"].dtype, r["closest"].dtype, r["face"].dtype, r["region"].dtype) == (torch.float32, torch.float32, torch.int32, torch.uint8)
    flat = np.array([[0, 0, 1], [1, 1, 1], [0, 1, 9], [-1, 2, 3]], np.int32)           # all degenerate or invalid
    q = _t(TRI_Q[:4])
    for faces in (np.zeros((0, 3), np.int32), flat):
        bad = _mesh(TRI_V, faces)
        with pytest.raises(ValueError, match="no surface to measure"):
            M.TriangleGrid(bad)
        for method in ("grid", "brute"):
            with pytest.raises(ValueError, match="no surface to measure"):
                M.point_mesh_distance(q, bad, method=method)
    with pytest.raises(ValueError, match="cloud"):
        M.point_mesh_distance(q, dict(m, faces=None))
    with pytest.raises(ValueError, match="method"):
        M.point_mesh_distance(q, m, method="bvh")
    with pytest.raises(RuntimeError, match="CUDA"):
        M.point_mesh_distance(q.cpu(), m)
    # the C entry points.  An all-unusable mesh gives the "no usable face" outputs
    lib = L.load()
    v, f = m["vertices"], _t(flat)
    n = 4
    ws = torch.zeros(lib.sp3_mesh_dist_query_ws_bytes(n), dtype=torch.uint8, device="cuda")
    dist, closest = torch.zeros(n, device="cuda"), torch.zeros((n, 3), device="cuda")
    face, region = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    L.check(lib.sp3_mesh_dist_brute(q.data_ptr(), n, v.data_ptr(), 3, f.data_ptr(), len(flat), ws.data_ptr(), dist.data_ptr(), closest.data_ptr(),
                                    face.data_ptr(), region.data_ptr(), L.stream_ptr()), "sp3_mesh_dist_brute")
    assert torch.isinf(dist).all() and torch.equal(closest, q) and (face == -1).all() and (region == 255).all()
    g = L.NnGrid(0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 2, 2, 1)
    import ctypes as C
    gp = C.byref(g)
    top = 2 ** 31 - 1
    assert lib.sp3_mesh_dist_query_ws_bytes(-1) == 0 and lib.sp3_mesh_dist_query_ws_bytes(0) == 32 and lib.sp3_mesh_dist_query_ws_bytes(5) == 32 + 8 * 16
    assert lib.sp3_mesh_tri_cell_count(None, 3, None, 5, gp, None, None) != 0 and b"null" in lib.sp3_last_error()
    assert lib.sp3_mesh_tri_cell_count(None, 3, None, -1, gp, None, None) != 0 and b"out of range" in lib.sp3_last_error()
    assert lib.sp3_mesh_tri_cell_count(None, top, None, 5, gp, None, None) != 0 and b"out of range" in lib.sp3_last_error()
    assert lib.sp3_mesh_tri_cell_count(None, 3, None, 5, None, None, None) != 0 and b"null grid" in lib.sp3_last_error()
    assert lib.sp3_mesh_tri_cell_count(None, 3, None, 0, gp, None, None) == 0             # no faces: nothing is launched
    assert lib.sp3_mesh_tri_cell_fill(None, 3, None, 5, gp, None, 7, None, None, None) != 0 and b"null" in lib.sp3_last_error()
    assert lib.sp3_mesh_tri_cell_fill(None, 3, None, 5, gp, None, -1, None, None, None) != 0 and b"npairs" in lib.sp3_last_error()
    assert lib.sp3_mesh_tri_cell_fill(None, 3, None, 5, gp, None, 0, None, None, None) == 0
    args = (None, 3, None, 5, None, 0, None, gp, 3, None, None, None, None, None, None)
    assert lib.sp3_mesh_dist_query(None, None, 4, *args) != 0 and b"null pointer" in lib.sp3_last_error()
    assert lib.sp3_mesh_dist_query(None, None, -1, *args) != 0 and b"out of range" in lib.sp3_last_error()
    assert lib.sp3_mesh_dist_query(None, None, 0, *args) == 0                               # nq = 0 launches nothing
    assert lib.sp3_mesh_dist_query(None, None, 4, None, 3, None, 0, None, 0, None, gp, 3, None, None, None, None, None, None) != 0
    assert b"1 face at least" in lib.sp3_last_error()
    assert lib.sp3_mesh_dist_query(None, None, 4, None, 3, None, 5, None, 0, None, gp, -1, None, None, None, None, None, None) != 0
    assert b"max_ring" in lib.sp3_last_error()
    bad_grid = L.NnGrid(0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0, 2, 1)
    assert lib.sp3_mesh_dist_query(None, None, 4, None, 3, None, 5, None, 0, None, C.byref(bad_grid), 3, None, None, None, None, None, None) != 0
    assert b"grid dims" in lib.sp3_last_error()
    assert lib.sp3_mesh_dist_brute(None, 4, None, 3, None, 5, None, None, None, None, None, None) != 0 and b"null pointer" in lib.sp3_last_error()
    assert lib.sp3_mesh_dist_brute(None, -2, None, 3, None, 5, None, None, None, None, None, None) != 0 and b"out of range" in lib.sp3_last_error()
    assert lib.sp3_mesh_dist_brute(None, 0, None, 3, None, 5, None, None, None, None, None, None) == 0


# ------------------------------------------------------------------------------------------------ 7. the analytic sphere
def _icosphere(levels):
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(levels):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, np.float32), np.array(f, np.int32)


def test_the_unit_sphere_from_radius_two():
    """An icosphere inscribed in the unit sphere, queries on the sphere of radius 2.  The mesh lies inside the ball of its largest
    vertex norm r_max, so dist >= |q| - r_max.  The ray from the origin to q crosses a face; every point of a face is at least
    sqrt(r_min^2 - R^2) from the origin, R its circumradius <= e_max / sqrt 3 (acute faces), so dist <= |q| - sqrt(r_min^2 -
    e_max^2 / 3): the [1, 1 + s] of s = 1 - sqrt(1 - e_max^2 / 3) with the fp32 rounding of the vertices (r_min, r_max) and of the
    queries (|q|) written in.  One fp32 ulp at 2 (2.4e-7) covers the rounding of dist itself."""
    from spann3r_amd import mesh as M
    verts, faces = _icosphere(3)
    assert len(faces) == 1280
    rng = np.random.default_rng(4)
    q = rng.normal(size=(2048, 3))
    q = (2 * q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    v64 = verts.astype(np.float64)
    edges = np.concatenate([v64[faces[:, i]] - v64[faces[:, (i + 1) % 3]] for i in range(3)])
    e_max = np.linalg.norm(edges, axis=1).max()
    rv = np.linalg.norm(v64, axis=1)
    rq = np.linalg.norm(q.astype(np.float64), axis=1)
    s = 1 - math.sqrt(1 - e_max ** 2 / 3)
    m = _mesh(verts, faces)
    r = M.point_mesh_distance(_t(q), m, return_stats=True)
    d = r["dist"].cpu().numpy().astype(np.float64)
    print("sphere: e_max %.4f s %.3e, dist in [%.7f, %.7f], %d fallbacks" % (e_max, s, d.min(), d.max(), r["stats"]["fallback_queries"]))
    tol = 2.4e-7
    assert (d >= rq - rv.max() - tol).all() and (d <= rq - np.sqrt(rv.min() ** 2 - e_max ** 2 / 3) + tol).all()
    assert d.min() >= 1 - 1e-6 and d.max() <= 1 + s + 1e-6 and s < 0.005
    b = M.point_mesh_distance(_t(q), m, method="brute")
    assert all(torch.equal(b[k], r[k]) for k in ("dist", "closest", "face", "region"))
    c = r["closest"].cpu().numpy().astype(np.float64)
    assert np.abs(np.linalg.norm(q - c, axis=1) - d).max() < 1e-6                     # the closest point is where the distance says


# ------------------------------------------------------------------------------------------------ 8. evaluate_meshes(exact=True)
def test_evaluate_meshes_exact_scores_one_plane_tessellated_twice_as_zero():
    """acc and comp below 1e-12: the fp64 rounding of a closest point at coordinates of at most 2 is a few 1e-16.  The sampled call on
    the same meshes keeps the floor of its sample spacing (0.0028 at 65536 samples)."""
    from spann3r_amd import evaluate as E
    (va, fa), (vb, fb) = _plane(False), _plane(True)
    a, b = _mesh(va, fa), _mesh(vb, fb)
    r = E.evaluate_meshes(a, b, n_samples=65536, icp=False, exact=True)
    print("exact: acc %.3e comp %.3e nc1 %.5f nc2 %.5f" % (r["acc"], r["comp"], r["nc1"], r["nc2"]))
    assert r["acc"] < 1e-12 and r["comp"] < 1e-12 and r["acc_med"] < 1e-12 and r["comp_med"] < 1e-12
    assert r["nc1"] == 1.0 and r["nc2"] == 1.0 and r["nc1_med"] == 1.0 and r["nc2_med"] == 1.0
    assert r["exact"] is True and r["samples"] == 65536 and r["pred_area"] == r["gt_area"] == 2.0 and np.array_equal(r["transformation"], np.eye(4))
    rs = E.evaluate_meshes(a, b, n_samples=65536, icp=False)
    assert rs["acc"] > 1e-3 and rs["comp"] > 1e-3
    keys = ["acc", "comp", "nc1", "nc2", "acc_med", "comp_med", "nc1_med", "nc2_med", "transformation", "pred_area", "gt_area", "samples"]
    assert sorted(rs) == sorted(keys) and sorted(r) == sorted(keys + ["exact"])
    # with ICP the prediction's vertices move with its samples: still one plane
    ri = E.evaluate_meshes(a, b, n_samples=65536, icp=True, exact=True)
    print("exact with ICP: acc %.3e comp %.3e, T - I at most %.2e" % (ri["acc"], ri["comp"], np.abs(ri["transformation"] - np.eye(4)).max()))
    assert ri["acc"] < 0.01 and ri["comp"] < 0.01 and ri["nc1"] > 0.99 and ri["nc2"] > 0.99      # (the bars of the sampled call with ICP)


# ------------------------------------------------------------------------------------------------ 9. the brick scene
@pytest.fixture(scope="module")
def brick():
    from spann3r_amd import fusion as F_
    frs = RC.scene_frames()
    vol = F_.BrickTSDFVolume(S["origin"], S["voxel"], S["dims"], trunc=S["trunc"], band=S["band"])
    vol.integrate(intrinsics=[f["K"] for f in frs], cam2world=[f["cam2world"] for f in frs], valid=[_t(f["valid"]) for f in frs],
                  pts=[_t(f["pts"]) for f in frs], images=[_t(f["images"]) for f in frs])
    return vol


@pytest.mark.parametrize("direct", [True, False])
def test_the_fused_surface_against_its_simplification(brick, direct):
    """prediction = the fused mesh, ground truth = the mesh simplified at 2 voxels.  The samples of a surface are a subset of it, so
    the distance to the surface cannot exceed the distance to the nearest sample: at most one fp32 ulp above it, query by query."""
    from spann3r_amd import evaluate as E, mesh as M
    pred = brick.extract_mesh(direct=direct)
    gt = brick.extract_mesh(direct=direct, simplify_cell=2 * S["voxel"])
    n = 20000
    sp, sg = M.sample_surface(pred, n, seed=0), M.sample_surface(gt, n, seed=0)
    for name, pts, mesh, samples in (("acc", sp["points"], gt, sg["points"]), ("comp", sg["points"], pred, sp["points"])):
        grid = M.TriangleGrid(mesh)
        assert grid.tries == 1 or mesh is gt                                          # marching tetrahedra's near-uniform faces: the first h holds
        ex = M.point_mesh_distance(pts, mesh, grid=grid, return_stats=True)
        sampled = E.CellGrid(samples).nn(pts)[0]
        up = torch.nextafter(sampled, torch.full_like(sampled, math.inf))
        assert bool((ex["dist"] <= up).all()), name
        print("brick scene %s (%s): %d faces, grid %s, %d pairs, %d tries; exact mean %.6f, sampled mean %.6f; %d fallbacks, %.1f faces per query" %
              (name, "direct" if direct else "dense", mesh["faces"].shape[0], grid.dims, grid.pairs, grid.tries, float(ex["dist"].mean()), float(sampled.mean()),
               ex["stats"]["fallback_queries"], ex["stats"]["faces_evaluated"] / n))
        br = M.point_mesh_distance(pts[:4096], mesh, method="brute")
        assert all(torch.equal(br[k], ex[k][:4096]) for k in ("dist", "closest", "face", "region")), name
        want = R.query(pts[:64].cpu().numpy(), mesh["vertices"].cpu().numpy(), mesh["faces"].cpu().numpy())
        _assert_same({k: ex[k][:64] for k in ("dist", "closest", "face", "region")}, want, name)
    r = E.evaluate_meshes(pred, gt, n_samples=n, icp=False, exact=True)
    rs = E.evaluate_meshes(pred, gt, n_samples=n, icp=False)
    assert r["exact"] is True and sorted(set(r) - {"exact"}) == sorted(rs)
    assert r["acc"] <= rs["acc"] and r["comp"] <= rs["comp"] and r["pred_area"] == rs["pred_area"] and r["gt_area"] == rs["gt_area"]
    print("brick scene evaluate_meshes: exact acc %.6f comp %.6f nc1 %.4f nc2 %.4f; sampled acc %.6f comp %.6f nc1 %.4f nc2 %.4f" %
          (r["acc"], r["comp"], r["nc1"], r["nc2"], rs["acc"], rs["comp"], rs["nc1"], rs["nc2"]))


# ------------------------------------------------------------------------------------------------ 10. the demo's argument
def test_demo_loop_rejects_eval_exact_without_eval_samples(monkeypatch, capsys):
    import demo_loop
    monkeypatch.setattr(sys, "argv", ["demo_loop.py", "--tiny", "--eval_exact"])
    with pytest.raises(SystemExit) as e:
        demo_loop.main()
    assert e.value.code == 2 and "needs --eval_samples" in capsys.readouterr().err
