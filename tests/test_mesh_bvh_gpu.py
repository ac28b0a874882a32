"""mesh.TriangleBVH and the bvh= keyword on the device (csrc/mesh_bvh.hip; include/spann3r_hip.h "Mesh BVH"): sp3_mesh_bvh_keys /
_build / _dist_query / _ray_query / _ray_views, and evaluate.evaluate_meshes(exact=True, accel="bvh").

Rules 3 of "Mesh distance" and 4 of "Mesh rays" make every result a pure function of the inputs, so the tree is held to the
brute-force kernels, to the grid and to the numpy restatements (tests/mesh_distance_ref.py, tests/mesh_ray_ref.py) BIT FOR BIT:
the bits of every float output, equality of face / region / side.  The structure is held to torch's amin / amax over its groups and
to tests/mesh_bvh_ref.py, and the walk's counters to the restatement's own walk.  The cap on the work is the form of
tests/test_mesh_ray_gpu.py: faces_evaluated <= n F / 8 in total -- a condition, which tests/test_mesh_bvh_cpu.py shows the
restatement to meet on the same inputs."""
import ctypes as C
import math
import sys

import numpy as np
import pytest
import torch

import bricks_ref as BR
import mesh_bvh_ref as B
import mesh_distance_ref as DR
import mesh_ray_ref as RR
import raycast_ref as RC
from test_mesh_ray_gpu import _grid_rays, sheet      # noqa: F401 -- the fixture and the grid rays of the set the rays are held to

pytestmark = pytest.mark.gpu

S = BR.SCENE
DKEYS = ("dist", "closest", "face", "region")
RKEYS = ("t", "face", "bary", "point", "side")


def _t(x):
    return torch.from_numpy(np.array(x)).cuda()


def _mesh(verts, faces):
    return dict(vertices=_t(np.asarray(verts, np.float32).reshape(-1, 3)), faces=_t(np.asarray(faces, np.int32).reshape(-1, 3)), bounds=None)


def _same(got, want, keys, what=""):
    """two result dicts (device or numpy), byte for byte (NaN origins come back as they are)"""
    for k in keys:
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        w = want[k].cpu().numpy() if isinstance(want[k], torch.Tensor) else want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero((np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)).reshape(len(g), -1).any(1))
        assert len(bad) == 0, "%s: %s differs at %d of %d, first at %d: %r vs %r" % (what, k, len(bad), len(g), bad[0], g[bad[0]], w[bad[0]])


def _dist(m, verts, faces, q, bvh=None, want=None, what=""):
    """bvh == brute == restatement for these queries -> (the tree's result with stats, the restatement)"""
    from spann3r_amd import mesh as M
    want = DR.query(q, verts, faces) if want is None else want
    qd = _t(np.asarray(q, np.float32))
    got = M.point_mesh_distance(qd, m, bvh=True if bvh is None else bvh, return_stats=True)
    _same(got, want, DKEYS, what + " bvh")
    _same(M.point_mesh_distance(qd, m, method="brute"), want, DKEYS, what + " brute")
    assert got["stats"]["fallback_queries"] == 0
    return got, want


def _rays(m, verts, faces, o, d, bvh=None, want=None, what="", **kw):
    from spann3r_amd import mesh as M
    want = RR.intersect(o, d, verts, faces, **kw) if want is None else want
    od, dd = _t(np.asarray(o, np.float32)), _t(np.asarray(d, np.float32))
    got = M.ray_mesh_intersect(od, dd, m, bvh=True if bvh is None else bvh, return_stats=True, **kw)
    _same(got, want, RKEYS, what + " bvh")
    _same(M.ray_mesh_intersect(od, dd, m, method="brute", **kw), want, RKEYS, what + " brute")
    return got, want


# ------------------------------------------------------------------------------------------------ 1. the structure
def _bad_faces_mixed_in(verts, faces, rng):
    """the mesh with a NaN and an infinite vertex appended and zero-area, repeated-index, out-of-range, NaN and infinite faces inserted"""
    nv = len(verts)
    v = np.concatenate([verts, [[np.nan, 0, 0], [0, np.inf, 0], [0.5, 0.0, 0.0], [0.25, 0.0, 0.0], [0.75, 0.0, 0.0]]]).astype(np.float32)
    bad = np.array([[nv + 2, nv + 3, nv + 4], [5, 5, 6], [7, 8, 7], [9, 9, 9], [-1, 3, 4], [3, nv + 5, 4], [3, 4, 2 ** 31 - 1], [-2 ** 31, 3, 4],
                    [nv, 10, 11], [10, nv + 1, 11], [nv, nv + 1, 12]], np.int32)
    where = np.sort(rng.choice(len(faces), len(bad), replace=False))
    f = np.insert(faces, where, bad, axis=0)
    is_bad = np.zeros(len(f), bool)
    is_bad[where + np.arange(len(bad))] = True
    assert np.array_equal(DR.usable(v, f), ~is_bad)
    return v, f, is_bad


def _check_structure(bvh, verts, faces, usable_idx):
    from spann3r_amd import cell_grid as G
    order = bvh.order.cpu().numpy()
    assert bvh.order.dtype == torch.int32 and bvh.usable == len(usable_idx) and np.array_equal(np.sort(order), usable_idx)
    sizes, offsets = B.level_table(bvh.usable)
    assert bvh.level_sizes == sizes and bvh.level_offsets == offsets and bvh.levels == len(sizes) == bvh.b.levels
    assert list(bvh.b.level_off[:len(offsets)]) == offsets and bvh.b.leaves == sizes[0] and bvh.b.usable == bvh.usable
    assert bvh.node_lo.shape == bvh.node_hi.shape == (offsets[-1], 3) and bvh.node_lo.dtype == torch.float32
    box = B.finite_box(verts)
    assert bvh.slack == B.slack_of(box) == float(np.float32(G.bvh_slack(box)))
    # every level against torch's amin / amax over its groups, from the device's own order
    tri = _t(verts)[_t(faces.astype(np.int64))[bvh.order.long()]]                      # [usable, 3, 3]
    inf = torch.tensor(math.inf, device="cuda")
    for l, n in enumerate(sizes):
        span = B.LEAF * B.ARITY ** l                                                   # faces below a node of this level; the last one may hold fewer
        pad = n * span - bvh.usable
        assert 0 <= pad < span
        lo = torch.cat([tri, inf.expand(pad, 3, 3)]).reshape(n, span * 3, 3).amin(1)
        hi = torch.cat([tri, (-inf).expand(pad, 3, 3)]).reshape(n, span * 3, 3).amax(1)
        assert torch.equal(bvh.node_lo[offsets[l]:offsets[l + 1]], lo) and torch.equal(bvh.node_hi[offsets[l]:offsets[l + 1]], hi), l
    # all of them against the restatement built on the same order; the order itself against the restatement's keys
    ref = B.build(verts, faces, order=order)
    assert np.array_equal(bvh.node_lo.cpu().numpy(), ref["node_lo"]) and np.array_equal(bvh.node_hi.cpu().numpy(), ref["node_hi"])
    assert np.array_equal(order, B.build(verts, faces)["order"])
    return ref


def test_the_structure_on_the_sheet_with_bad_faces_mixed_in():
    from spann3r_amd import mesh as M
    verts, faces = RR.bumpy_sheet()
    v, f, is_bad = _bad_faces_mixed_in(verts, faces, np.random.default_rng(21))
    bvh = M.TriangleBVH(_mesh(v, f))
    assert bvh.usable == 1922 and bvh.levels == 6
    _check_structure(bvh, v, f, np.flatnonzero(~is_bad))
    again = M.TriangleBVH(_mesh(v, f))                                                 # the same bits every run
    assert torch.equal(again.order, bvh.order) and torch.equal(again.node_lo, bvh.node_lo) and torch.equal(again.node_hi, bvh.node_hi)
    # queries through it never see a bad face
    q = np.concatenate([np.random.default_rng(22).uniform(-0.5, 1.5, (256, 3)), v[f[~is_bad][:64, 0]]]).astype(np.float32)
    got, want = _dist(_mesh(v, f), v, f, q, bvh=bvh, what="bad faces")
    assert not is_bad[want["face"]].any()


@pytest.mark.parametrize("usable", B.COUNTS[:-1])
def test_the_structure_at_the_counts_where_the_table_changes(usable):
    from spann3r_amd import mesh as M
    verts, faces = RR.bumpy_sheet()
    faces = np.ascontiguousarray(faces[np.random.default_rng(usable).permutation(len(faces))[:usable]])
    m = _mesh(verts, faces)
    bvh = M.TriangleBVH(m)
    _check_structure(bvh, verts, faces, np.arange(usable))
    rng = np.random.default_rng(usable + 1)
    q = rng.uniform(-0.5, 1.5, (64, 3)).astype(np.float32)
    _dist(m, verts, faces, q, bvh=bvh, what="%d faces" % usable)
    o = rng.uniform(-0.2, 1.2, (64, 3)) + (0, 0, 1)
    d = np.concatenate([rng.uniform(0, 1, (64, 1)), rng.uniform(-0.5, 0.5, (64, 1)), np.zeros((64, 1))], 1) - o
    _rays(m, verts, faces, o, d, bvh=bvh, what="%d faces" % usable)


# ------------------------------------------------------------------------------------------------ 2. distance
TRI_V = np.array([(0, 0, 0), (2, 0, 0), (0, 2, 0)], np.float32)
TRI_F = np.array([[0, 1, 2]], np.int32)
TRI_Q = np.array([(-1, -1, 0.5), (3, -0.5, 0.25), (1, -1, 1), (-0.5, 3, -0.25), (-1, 1, -1), (2, 2, 0.5), (0.5, 0.5, 0.75),      # regions 0..6
                  (0.5, 0.5, 0), (0.25, 1.25, 0),                                                       # in the plane, inside
                  (1, 0, 0), (0, 0.5, 0), (1, 1, 0),                                                     # exactly on each edge
                  (0, 0, 0), (2, 0, 0), (0, 2, 0),                                                       # exactly at each vertex
                  (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)], np.float32)                           # no winner


def test_distance_one_triangle_in_every_region():
    from spann3r_amd import mesh as M
    m = _mesh(TRI_V, TRI_F)
    bvh = M.TriangleBVH(m)
    assert bvh.usable == 1 and bvh.levels == 1 and bvh.level_sizes == [1]                # F = 1: the root is the leaf
    got, want = _dist(m, TRI_V, TRI_F, TRI_Q, bvh=bvh, what="triangle")
    assert want["region"][:7].tolist() == [0, 1, 2, 3, 4, 5, 6] and want["face"][15:].tolist() == [-1] * 3
    assert got["stats"]["faces_evaluated"] == 15 and got["stats"]["nodes_visited"] == 15      # a non-finite query never enters the tree
    assert sorted(got["stats"]) == ["cells_visited", "faces_evaluated", "fallback_queries", "grid", "h", "levels", "nodes", "nodes_visited", "pairs"]
    assert got["stats"]["cells_visited"] == 0 and got["stats"]["pairs"] == 0 and got["stats"]["levels"] == 1 and got["stats"]["nodes"] == 1


@pytest.fixture(scope="module")
def dsheet():
    """the fixture of tests/test_mesh_distance_gpu.py, rebuilt: (verts, faces, queries, the restatement's answer): 2048 queries within
    0.005 of the surface, 1024 inside the box, 1024 outside it by up to 1000 extents"""
    verts, faces = RR.bumpy_sheet()
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
    return verts, faces, q, DR.query(q, verts, faces)


def test_distance_on_the_sheet_and_the_far_queries_alone(dsheet):
    from spann3r_amd import mesh as M
    verts, faces, q, want = dsheet
    F = len(faces)
    m = _mesh(verts, faces)
    bvh = M.TriangleBVH(m)
    got, _ = _dist(m, verts, faces, q, bvh=bvh, want=want, what="sheet")
    print("sheet: %d levels, %d nodes; %.1f nodes visited and %.1f faces evaluated per query (brute force: %d)" %
          (bvh.levels, bvh.level_offsets[-1], got["stats"]["nodes_visited"] / len(q), got["stats"]["faces_evaluated"] / len(q), F))
    assert 0 < got["stats"]["faces_evaluated"] <= len(q) * F // 8
    # the far 1024 alone: under the cap, where the grid hands every one of them to the brute-force kernels
    far = {k: want[k][3072:] for k in want}
    fb, _ = _dist(m, verts, faces, q[3072:], bvh=bvh, want=far, what="far")
    print("far: %.1f nodes visited and %.1f faces evaluated per query" % (fb["stats"]["nodes_visited"] / 1024, fb["stats"]["faces_evaluated"] / 1024))
    assert 0 < fb["stats"]["faces_evaluated"] <= 1024 * F // 8
    fg = M.point_mesh_distance(_t(q[3072:]), m, return_stats=True)
    assert fg["stats"]["fallback_queries"] == 1024
    _same(fg, fb, DKEYS, "far, grid against bvh")
    # the walk's counters are the restatement's own, query set by query set (the same order of the faces, the same walk)
    ref = B.build(verts, faces, order=bvh.order.cpu().numpy())
    pick = np.concatenate([np.arange(0, 96), np.arange(2048, 2112), np.arange(3072, 3168)])
    rw = B.dist_query(q[pick], ref)
    gw = M.point_mesh_distance(_t(q[pick]), m, bvh=bvh, return_stats=True)
    _same(gw, rw, DKEYS, "walk")
    assert gw["stats"]["nodes_visited"] == int(rw["nodes"].sum()) and gw["stats"]["faces_evaluated"] == int(rw["evals"].sum())
    # the same bits a second time, and with bvh=True
    again = M.point_mesh_distance(_t(q), m, bvh=True)
    assert all(torch.equal(again[k], got[k]) for k in DKEYS)


@pytest.mark.parametrize("reverse", [False, True])
def test_distance_ties_take_the_smaller_index_across_the_tree(reverse):
    """two copies of one triangle at z = +1 and z = -1, the sheet's faces between them in index order, queries on z = 0 over the
    triangle: both copies give d2 = 1 exactly, in leaves far apart, and the smaller index wins"""
    from spann3r_amd import mesh as M
    sv, sf = RR.bumpy_sheet(12)
    sv = sv + np.float32((5, 0, 0))                                                    # the sheet out of the way: it never wins
    tri = np.array([(0, 0, 1), (1, 0, 1), (0, 1, 1), (0, 0, -1), (1, 0, -1), (0, 1, -1)], np.float32)
    verts = np.concatenate([tri, sv])
    faces = np.concatenate([[(0, 1, 2)], sf + 6, [(3, 4, 5)]]).astype(np.int32)
    if reverse:
        faces = np.ascontiguousarray(faces[::-1])
    rng = np.random.default_rng(9)
    w = rng.dirichlet((1, 1, 1), 256)
    q = np.stack([w[:, 1], w[:, 2], np.zeros(256)], 1).astype(np.float32)
    got, want = _dist(_mesh(verts, faces), verts, faces, q, what="tie")
    assert (want["face"] == 0).all() and (want["dist"] == 1).all() and (want["region"] == 6).all()
    assert (want["closest"][:, 2] == (-1 if reverse else 1)).all()


def test_distance_permuted_faces_and_mixed_face_sizes(dsheet):
    from spann3r_amd import mesh as M
    verts, faces, q, want = dsheet
    perm = np.random.default_rng(3).permutation(len(faces))
    a = M.point_mesh_distance(_t(q), _mesh(verts, np.ascontiguousarray(faces[perm])), bvh=True)
    _same(a, want, ("dist",), "permuted")
    moved = perm[a["face"].cpu().numpy()] != want["face"]
    assert (want["region"][moved] != 6).all()                                          # another face only where two reach the same d2
    # the 64-fold mixed-size plane of tests/test_mesh_distance_gpu.py: the grid needs several tries of h, the tree none
    g = 64
    y, x = np.mgrid[:g + 1, :g + 1]
    v = np.stack([x / g, y / g, np.zeros_like(x, float)], -1).reshape(-1, 3)
    tl = (y[:-1, :-1] * (g + 1) + x[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([tl, tl + 1, tl + g + 2], 1), np.stack([tl, tl + g + 2, tl + g + 1], 1)])
    n, c10, c11 = len(v), g, g * (g + 1) + g
    v = np.concatenate([v, [[2, 0, 0], [2, 1, 0]]]).astype(np.float32)
    f = np.concatenate([f, [[c10, n, n + 1], [c10, n + 1, c11]]]).astype(np.int32)
    m = _mesh(v, f)
    fine = M.TriangleGrid(m, h=1 / 256)
    assert fine.tries > 1
    rng = np.random.default_rng(8)
    qq = np.concatenate([rng.uniform((-0.2, -0.2, -0.3), (2.2, 1.2, 0.3), (384, 3)), rng.uniform((0, 0, 0), (2, 1, 0), (128, 3))]).astype(np.float32)
    got, w2 = _dist(m, v, f, qq, what="mixed")
    assert (w2["face"] >= len(f) - 2).sum() > 100 and (w2["face"] < len(f) - 2).sum() > 100
    _same(M.point_mesh_distance(_t(qq), m, grid=fine), got, DKEYS, "mixed, grid against bvh")
    assert got["stats"]["faces_evaluated"] <= len(qq) * len(f) // 8


# ------------------------------------------------------------------------------------------------ 3. rays
EYE = np.array((0.25, 0.5, 4), np.float32)
TRI_RAYS = [((0.5, 0.5, 1), (0, 0, -1)), ((0.5, 0.5, -1), (0, 0, 2)), ((0.25, 0.25, 2), (0.5, 0.25, -2)),
            (EYE, (1, 0, 0) - EYE), (EYE, (0, 1, 0) - EYE), (EYE, (1, 1, 0) - EYE),      # onto each edge
            (EYE, (0, 0, 0) - EYE), (EYE, (2, 0, 0) - EYE), (EYE, (0, 2, 0) - EYE),      # onto each vertex
            ((-1, 0.5, 0), (1, 0, 0)), ((0.5, 0.5, 0), (1, 1, 0)),                       # in its plane
            ((-1, 0.5, 0.5), (1, 0, 0)),                                                 # parallel above it
            ((0.5, 0.5, 1), (0, 0, 1)), ((0.5, 0.5, -1), (0, 0, -1)),                    # it lies behind the start
            ((3, 3, 1), (0, 0, -1)),                                                     # past it
            ((0.5, 0.5, 0), (0, 0, 1))]                                                  # starting on it: t = +0
TRI_O = np.array([r[0] for r in TRI_RAYS], np.float32)
TRI_D = np.array([r[1] for r in TRI_RAYS], np.float32)


def test_rays_one_triangle_and_a_shared_edge():
    from spann3r_amd import mesh as M
    m = _mesh(TRI_V, TRI_F)
    bvh = M.TriangleBVH(m)
    got, want = _rays(m, TRI_V, TRI_F, TRI_O, TRI_D, bvh=bvh, what="triangle")
    assert want["face"].tolist() == [0] * 9 + [-1] * 6 + [0] and want["side"].tolist() == [0, 1, 0] + [0] * 6 + [255] * 6 + [1]
    assert sorted(got["stats"]) == ["cells_visited", "faces_evaluated", "grid", "h", "levels", "nodes", "nodes_visited", "pairs"]
    back, _ = _rays(m, TRI_V, TRI_F, TRI_O, TRI_D, bvh=bvh, what="cull back", cull="back")
    front, _ = _rays(m, TRI_V, TRI_F, TRI_O, TRI_D, bvh=bvh, what="cull front", cull="front")
    assert back["face"].cpu().tolist() == [0, -1] + [0] * 7 + [-1] * 7 and front["face"].cpu().tolist() == [-1, 0] + [-1] * 13 + [0]
    # the range cuts the hit off on either end and holds exactly at it (ray 0 hits at t = 1, ray 1 at 0.5)
    for t_min, t_max, hit0 in ((0.0, 0.5, False), (1.5, math.inf, False), (1.0, 1.0, True), (0.0, 1.0, True), (1.0, 2.0, True), (0.75, 0.875, False)):
        r, _ = _rays(m, TRI_V, TRI_F, TRI_O[:2], TRI_D[:2], bvh=bvh, what="range %g %g" % (t_min, t_max), t_min=t_min, t_max=t_max)
        assert (int(r["face"][0]) == 0) == hit0 and (int(r["face"][1]) == 0) == (t_min <= 0.5 <= t_max)
    # a shared edge: dyadic coordinates, U = 0 on the diagonal for both faces, the smaller index takes it
    verts = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], np.float32)
    faces = np.array([(0, 1, 2), (0, 2, 3)], np.int32)
    k = np.arange(1, 8) / 8.0
    tgt = np.stack([k, k, np.zeros_like(k)], 1)
    off = np.array([(0, 0, 1), (0.25, -0.5, 1), (-0.75, 0.125, 1), (0.5, 0.5, 1)])
    o = (tgt[:, None] + off[None]).reshape(-1, 3).astype(np.float32)
    d = (np.repeat(tgt, len(off), 0) - o).astype(np.float32)
    _, w = _rays(_mesh(verts, faces), verts, faces, o, d, what="shared edge")
    assert (w["face"] == 0).all() and (w["t"] == 1).all()
    _, w2 = _rays(_mesh(verts, faces[::-1].copy()), verts, faces[::-1].copy(), o, d, what="shared edge, swapped")
    assert (w2["face"] == 0).all()
    rng = np.random.default_rng(2)
    s = rng.uniform(0.01, 0.99, 512)
    o2 = rng.uniform(-1, 2, (512, 3)) + (0, 0, 3)
    _, w3 = _rays(_mesh(verts, faces), verts, faces, o2, np.stack([s, s, np.zeros_like(s)], 1) - o2, what="diagonal")
    assert (w3["face"] >= 0).all()                                                     # no ray passes between the two faces


@pytest.fixture(scope="module")
def rsheet(sheet):
    """the 4096-ray set of tests/test_mesh_ray_gpu.py itself: its `sheet` fixture (256 rays that miss the box, two 32 x 32 cameras,
    rays from outside and from inside, zero components, non-finite and zero rays), its rays on the walls and through the corners
    of the cells of TriangleGrid(m), and its random rays up to 4096
    -> (verts, faces, o, d, the restatement's answer, the number of leading rays that miss the box, where the bad rays start)"""
    from spann3r_amd import mesh as M
    verts, faces, o, d, n_miss = sheet
    go, gd = _grid_rays(M.TriangleGrid(_mesh(verts, faces)), verts)
    n_pad = 4096 - len(o) - len(go)
    assert n_pad >= 0
    rng = np.random.default_rng(8)
    po = rng.uniform(-1, 2, (n_pad, 3)).astype(np.float32)
    pd = rng.normal(size=(n_pad, 3)).astype(np.float32)
    o, d = np.concatenate([o, go, po]), np.concatenate([d, gd, pd])
    assert len(o) == 4096
    return verts, faces, o, d, RR.intersect(o, d, verts, faces), n_miss, 256 + 2048 + 512 + 512 + 384


def test_rays_on_the_sheet(rsheet):
    from spann3r_amd import mesh as M
    verts, faces, o, d, want, n_miss, bad0 = rsheet
    F = len(faces)
    m = _mesh(verts, faces)
    bvh = M.TriangleBVH(m)
    got, _ = _rays(m, verts, faces, o, d, bvh=bvh, want=want, what="sheet")
    hits = int((want["face"] >= 0).sum())
    print("sheet: %d of 4096 rays hit; %.1f nodes visited and %.1f faces evaluated per ray (brute force: %d)" %
          (hits, got["stats"]["nodes_visited"] / 4096, got["stats"]["faces_evaluated"] / 4096, F))
    assert 1024 < hits < 4096 and 0 < got["stats"]["faces_evaluated"] <= 4096 * F // 8
    _same(M.ray_mesh_intersect(_t(o), _t(d), m), got, RKEYS, "grid against bvh")
    # the rays that miss the root's box evaluate nothing and visit nothing
    miss = M.ray_mesh_intersect(_t(o[:n_miss]), _t(d[:n_miss]), m, bvh=bvh, return_stats=True)
    assert miss["stats"]["faces_evaluated"] == 0 and miss["stats"]["nodes_visited"] == 0 and bool((miss["face"] == -1).all())
    assert (want["face"][bad0:bad0 + 48] == -1).all() and (want["face"][bad0 + 48:bad0 + 64] >= 0).all()
    _rays(m, verts, faces, o[256:1280], d[256:1280], bvh=bvh, what="sheet, range and cull", t_min=0.25, t_max=0.95, cull="back")
    # the walk's counters are the restatement's own
    ref = B.build(verts, faces, order=bvh.order.cpu().numpy())
    pick = np.concatenate([np.arange(224, 320), np.arange(2304, 2400), np.arange(3328, 3392), np.arange(bad0, bad0 + 128)])      # (the last 64: rays on cell walls and through cell corners)
    rw = B.ray_query(o[pick], d[pick], ref)
    gw = M.ray_mesh_intersect(_t(o[pick]), _t(d[pick]), m, bvh=bvh, return_stats=True)
    _same(gw, rw, RKEYS, "walk")
    assert gw["stats"]["nodes_visited"] == int(rw["nodes"].sum()) and gw["stats"]["faces_evaluated"] == int(rw["evals"].sum())
    again = M.ray_mesh_intersect(_t(o), _t(d), m, bvh=True)
    _same(again, got, RKEYS, "a second time")


def test_rays_on_a_flat_plane_and_from_inside_the_icosphere():
    from spann3r_amd import mesh as M
    # zero-thickness boxes: every node of the plane z = 2 has lo.z == hi.z
    verts, faces = RR.plane(9, 2.0)
    m = _mesh(verts, faces)
    bvh = M.TriangleBVH(m)
    assert torch.equal(bvh.node_lo[:, 2], bvh.node_hi[:, 2]) and bool((bvh.node_lo[:, 2] == 2).all())
    rng = np.random.default_rng(13)
    xy = np.concatenate([rng.uniform(-1.5, 1.5, (448, 2)), verts[::3, :2], [(-1.5, -1.5), (1.5, 1.5), (0, 0)]])
    o = np.concatenate([xy, np.zeros((len(xy), 1))], 1).astype(np.float32)
    d = np.tile(np.array([(0, 0, 1)], np.float32), (len(o), 1))
    got, want = _rays(m, verts, faces, o, d, bvh=bvh, what="plane")
    assert (want["face"] >= 0).all() and (want["t"] == 2.0).all()
    o2 = rng.uniform(-1, 1, (256, 3)).astype(np.float32)                               # oblique ones
    d2 = (np.concatenate([rng.uniform(-1.4, 1.4, (256, 2)), np.full((256, 1), 2.0)], 1) - o2).astype(np.float32)
    _, w2 = _rays(m, verts, faces, o2, d2, bvh=bvh, what="plane, oblique")
    assert (w2["face"] >= 0).all()
    # watertight: no ray from inside the level-3 icosphere gets out
    verts, faces = RR.icosphere(3)
    m = _mesh(verts, faces)
    bvh = M.TriangleBVH(m)
    for origin in RR.SPHERE_ORIGINS:
        o, d = RR.sphere_rays(verts, faces, origin)
        got, want = _rays(m, verts, faces, o, d, bvh=bvh, what="icosphere")
        assert bool((got["face"] >= 0).all()) and bool((got["side"] == 1).all())
        assert got["stats"]["faces_evaluated"] <= len(o) * len(faces) // 8


def test_render_depth_maps_through_the_tree_equal_the_grids(rsheet):
    from spann3r_amd import mesh as M
    verts, faces = rsheet[:2]
    m = _mesh(verts, faces)
    bvh = M.TriangleBVH(m)
    K = np.array([[[16.0, 0, 10.25], [0, 15.0, 6.5], [0, 0, 1]], [[11.0, 0, 9.0], [0, 12.5, 5.75], [0, 0, 1]], [[9.0, 0, 10.0], [0, 9.0, 6.0], [0, 0, 1]]])
    P = np.stack([np.diag([1.0, -1.0, -1.0, 1.0]), np.eye(4), np.diag([1.0, -1.0, -1.0, 1.0])])
    a = 2.4
    P[1, :3, :3] = np.array([[math.cos(0.3), 0, math.sin(0.3)], [0, 1, 0], [-math.sin(0.3), 0, math.cos(0.3)]]) @ \
        np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    P[0, :3, 3], P[1, :3, 3], P[2, :3, 3] = (0.5, 0.0, 0.8), (0.3, 0.4, 0.7), (1.4, 0.2, 2.5)      # the third sees the sheet's edge and past it
    h, w = 13, 21                                                     # neither a multiple of the 8 x 8 tile
    keys = ("depth", "face", "bary")
    for kw in (dict(), dict(pixel_offset=0.5), dict(near=0.75, far=0.8125)):
        ref = M.render_depth_maps(m, K, P, (h, w), return_faces=True, **kw)
        got = M.render_depth_maps(m, K, P, (h, w), bvh=bvh, return_faces=True, return_stats=True, **kw)
        _same(got, ref, keys, "maps %s" % kw)
        assert 0 < int((got["face"] >= 0).sum()) < 3 * h * w and 0 < got["stats"]["faces_evaluated"] <= 3 * h * w * len(faces) // 8
        assert sorted(got["stats"]) == ["cells_visited", "faces_evaluated", "grid", "h", "levels", "nodes", "nodes_visited", "pairs"]
    ref = M.render_depth_maps(m, K, P, (h, w), return_faces=True)
    gl = P * np.array([1.0, -1.0, -1.0, 1.0])
    _same(M.render_depth_maps(m, K, gl, (h, w), bvh=True, opengl=True, return_faces=True), ref, keys, "opengl")
    # and the rule itself: camera 2 against the restatement on its rays
    o, d = RR.camera_rays(K[2], P[2], (h, w))
    want = RR.intersect(o, d, verts, faces)
    one = M.render_depth_maps(m, K[2], P[2], (h, w), bvh=bvh, return_faces=True)
    assert sorted(M.render_depth_maps(m, K[2], P[2], (h, w), bvh=bvh)) == ["depth"]
    assert np.array_equal(one["face"].cpu().numpy().reshape(-1), want["face"])
    _same(dict(depth=one["depth"].reshape(-1)), dict(depth=np.where(want["face"] >= 0, want["t"], np.float32(0))), ("depth",), "camera 2")
    none = M.render_depth_maps(m, K[0], np.zeros((0, 4, 4)), (h, w), bvh=bvh, return_faces=True)
    assert none["depth"].shape == (0, h, w) and none["face"].shape == (0, h, w)


# ------------------------------------------------------------------------------------------------ 4. evaluate
def _plane(mirror):
    """a plane of 2 x 1 units: a 64 x 64 grid of cells on one half, two triangles on the other (tests/test_mesh_distance_gpu.py)"""
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


def _same_dict(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], (k, a[k], b[k])


def test_evaluate_meshes_accel_bvh_returns_the_grids_dict_on_the_plane():
    from spann3r_amd import evaluate as E
    (va, fa), (vb, fb) = _plane(False), _plane(True)
    a, b = _mesh(va, fa), _mesh(vb, fb)
    for icp in (False, True):
        rg = E.evaluate_meshes(a, b, n_samples=16384, icp=icp, exact=True, accel="grid")
        rb = E.evaluate_meshes(a, b, n_samples=16384, icp=icp, exact=True, accel="bvh")
        _same_dict(rb, rg)
        _same_dict(E.evaluate_meshes(a, b, n_samples=16384, icp=icp, exact=True), rg)  # the default is the grid
    assert rb["exact"] is True and rb["acc"] < 0.01
    with pytest.raises(ValueError, match="exact=True"):
        E.evaluate_meshes(a, b, n_samples=64, accel="bvh")
    with pytest.raises(ValueError, match="exact=True"):
        E.evaluate_meshes(a, b, n_samples=64, accel="grid")
    with pytest.raises(ValueError, match="accel"):
        E.evaluate_meshes(a, b, n_samples=64, exact=True, accel="kd")


@pytest.fixture(scope="module")
def brick():
    from spann3r_amd import fusion as F_
    frs = RC.scene_frames()
    vol = F_.BrickTSDFVolume(S["origin"], S["voxel"], S["dims"], trunc=S["trunc"], band=S["band"])
    vol.integrate(intrinsics=[f["K"] for f in frs], cam2world=[f["cam2world"] for f in frs], valid=[_t(f["valid"]) for f in frs],
                  pts=[_t(f["pts"]) for f in frs], images=[_t(f["images"]) for f in frs])
    return vol, frs


@pytest.mark.parametrize("direct", [True, False])
def test_the_brick_scene_through_the_tree(brick, direct):
    from spann3r_amd import evaluate as E, mesh as M
    vol, frs = brick
    pred = vol.extract_mesh(direct=direct)
    gt = vol.extract_mesh(direct=direct, simplify_cell=2 * S["voxel"])
    n = 20000
    _same_dict(E.evaluate_meshes(pred, gt, n_samples=n, icp=False, exact=True, accel="bvh"), E.evaluate_meshes(pred, gt, n_samples=n, icp=False, exact=True))
    # the samples of one surface against the other, and the same displaced by a scene extent: the grid's fallback, the tree's walk
    pts = M.sample_surface(pred, 4096, seed=1)["points"]
    bvh = M.TriangleBVH(gt)
    nf = gt["faces"].shape[0]
    ext = float((gt["vertices"].amax(0) - gt["vertices"].amin(0)).max())
    for name, q in (("near", pts), ("displaced", (pts + torch.tensor([0.0, 0.0, 2 * ext], device="cuda")).contiguous())):
        g = M.point_mesh_distance(q, gt, return_stats=True)
        b = M.point_mesh_distance(q, gt, bvh=bvh, return_stats=True)
        _same(b, g, DKEYS, name)
        print("brick scene %s (%s): %d faces, %d levels; grid %d fallbacks, %.1f faces per query; tree %.1f nodes, %.1f faces per query" %
              (name, "direct" if direct else "dense", nf, bvh.levels, g["stats"]["fallback_queries"], g["stats"]["faces_evaluated"] / 4096,
               b["stats"]["nodes_visited"] / 4096, b["stats"]["faces_evaluated"] / 4096))
        assert b["stats"]["faces_evaluated"] <= 4096 * nf // 8
    assert g["stats"]["fallback_queries"] == 4096
    # a camera of the scene: the maps of the tree are the grid's, and evaluate_depth scores them alike
    K = np.asarray(frs[2]["K"], np.float64).copy()
    K[:2] *= 0.5
    P = np.asarray(frs[2]["cam2world"], np.float64)
    mg = M.render_depth_maps(pred, K, P, (24, 32), return_faces=True)
    mb = M.render_depth_maps(pred, K, P, (24, 32), bvh=True, return_faces=True, return_stats=True)
    _same(mb, mg, ("depth", "face", "bary"), "brick camera")
    assert int((mb["face"] >= 0).sum()) > 0 and mb["stats"]["faces_evaluated"] < 768 * pred["faces"].shape[0] // 8
    view = dict(depthmap=mg["depth"] * 1.1, valid_mask=mg["depth"] > 0, camera_intrinsics=torch.from_numpy(K[None].astype(np.float32)),
                camera_pose=torch.from_numpy(P[None].astype(np.float32)))
    assert E.evaluate_depth(pred, [view], bvh=True) == E.evaluate_depth(pred, [view])


# ------------------------------------------------------------------------------------------------ 5. empty sizes and argument errors
def test_empty_sizes_and_argument_errors():
    from spann3r_amd import cell_grid as G, lib as L, mesh as M
    m = _mesh(TRI_V, TRI_F)
    bvh = M.TriangleBVH(m)
    r = M.point_mesh_distance(torch.empty((0, 3), device="cuda"), m, bvh=bvh, return_stats=True)
    assert r["dist"].shape == (0,) and r["closest"].shape == (0, 3) and r["face"].dtype == torch.int32 and r["region"].dtype == torch.uint8
    assert r["stats"]["nodes_visited"] == 0 and r["stats"]["faces_evaluated"] == 0
    e = torch.empty((0, 3), device="cuda")
    r = M.ray_mesh_intersect(e, e, m, bvh=bvh, return_stats=True)
    assert r["t"].shape == (0,) and r["bary"].shape == (0, 3) and r["side"].dtype == torch.uint8 and r["stats"]["nodes_visited"] == 0
    q = _t(TRI_Q[:4])
    grid = M.TriangleGrid(m)
    for call in (lambda **kw: M.point_mesh_distance(q, m, **kw), lambda **kw: M.ray_mesh_intersect(q, q, m, **kw)):
        with pytest.raises(ValueError, match="bvh= replaces the grid"):
            call(bvh=bvh, grid=grid)
        with pytest.raises(ValueError, match="bvh= replaces the grid"):
            call(bvh=True, method="brute")
        with pytest.raises(ValueError, match="method must be"):
            call(bvh=bvh, method="bvh")
        with pytest.raises(ValueError, match="method must be"):
            call(method="bvh")
        with pytest.raises(ValueError, match="TriangleBVH"):
            call(bvh=grid)
    with pytest.raises(ValueError, match="bvh= replaces the grid"):
        M.render_depth_maps(m, np.array([[10.0, 0, 2], [0, 10.0, 2], [0, 0, 1]]), np.eye(4), (4, 4), bvh=bvh, grid=grid)
    flat = np.array([[0, 0, 1], [1, 1, 1], [0, 1, 9], [-1, 2, 3]], np.int32)           # all degenerate or invalid
    for faces in (np.zeros((0, 3), np.int32), flat):
        bad = _mesh(TRI_V, faces)
        with pytest.raises(ValueError, match="no surface to measure"):
            M.TriangleBVH(bad)
        with pytest.raises(ValueError, match="none valid"):
            M.point_mesh_distance(q, bad, bvh=True)
        with pytest.raises(ValueError, match="none valid"):
            M.ray_mesh_intersect(q, q, bad, bvh=True)
        with pytest.raises(ValueError, match="none valid"):
            M.render_depth_maps(bad, np.array([[10.0, 0, 2], [0, 10.0, 2], [0, 0, 1]]), np.eye(4), (4, 4), bvh=True)
    with pytest.raises(ValueError, match="cloud"):
        M.TriangleBVH(dict(m, faces=None))
    with pytest.raises(ValueError, match="one at least"):
        G.bvh_levels(0)
    # the C entry points validate the level table before anything is launched or dereferenced
    lib = L.load()

    def table(usable, sizes, slack=0.0, leaves=None, levels=None):
        b = L.MeshBvh(usable=usable, leaves=sizes[0] if leaves is None else leaves, levels=len(sizes) if levels is None else levels, slack=slack)
        b.level_off[:len(sizes) + 1] = [0] + np.cumsum(sizes).tolist()
        return C.byref(b)

    dq = lambda b, nq=4, nf=100: lib.sp3_mesh_bvh_dist_query(None, None, nq, None, 3, None, nf, None, None, None, b, None, None, None, None, None, None)
    assert dq(table(100, [25, 7, 2, 1]), nq=0) == 0                                    # nq = 0 launches nothing
    assert dq(table(100, [25, 7, 2, 1])) != 0 and b"null pointer" in lib.sp3_last_error()
    assert dq(None) != 0 and b"null tree" in lib.sp3_last_error()
    assert dq(table(100, [25, 7, 2, 1]), nq=-1) != 0 and b"out of range" in lib.sp3_last_error()
    assert dq(table(101, [25, 7, 2, 1])) != 0 and b"usable" in lib.sp3_last_error()     # more usable faces than faces
    assert dq(table(100, [26, 7, 2, 1])) != 0 and b"leaves" in lib.sp3_last_error()
    assert dq(table(100, [25, 6, 2, 1])) != 0 and b"level 1 holds 7" in lib.sp3_last_error()     # not the ceiling quotient
    assert dq(table(100, [25, 7, 2])) != 0 and b"last level" in lib.sp3_last_error()
    assert dq(table(100, [25, 7, 2, 1, 1])) != 0 and b"already the root" in lib.sp3_last_error()
    assert dq(table(100, [25, 7, 2, 1], levels=17)) != 0 and b"levels" in lib.sp3_last_error()
    # the tallest tree there is: 2^31 - 2 faces, 16 levels, the root alone on the last -- accepted (what fails next is the null pointers)
    top = 2 ** 31 - 2
    tall, _ = G.bvh_levels(top)
    assert len(tall) == 16 == L.MeshBvh.MAX_LEVELS and tall[0] == 2 ** 29 and tall[-2:] == [2, 1]
    assert dq(table(top, tall), nf=top) != 0 and b"null pointer" in lib.sp3_last_error()
    assert G.make_bvh(np.zeros((2, 3)), top)[0].levels == 16
    assert dq(table(100, [25, 7, 2, 1], levels=0)) != 0 and b"levels" in lib.sp3_last_error()
    assert dq(table(100, [25, 7, 2, 1], slack=-1.0)) != 0 and b"slack" in lib.sp3_last_error()
    assert dq(table(100, [25, 7, 2, 1], slack=math.nan)) != 0 and b"slack" in lib.sp3_last_error()
    assert dq(table(100, [25, 7, 2, 1]), nf=0) != 0 and b"1 face at least" in lib.sp3_last_error()
    bad_off = L.MeshBvh(usable=4, leaves=1, levels=1, slack=0.0)
    bad_off.level_off[0], bad_off.level_off[1] = 1, 2
    assert dq(C.byref(bad_off)) != 0 and b"start at 0" in lib.sp3_last_error()
    good = table(100, [25, 7, 2, 1])
    rq = lambda **kw: lib.sp3_mesh_bvh_ray_query(None, None, None, kw.get("nq", 4), None, 3, None, 100, None, None, None, kw.get("b", good),
                                                 kw.get("t_min", 0.0), kw.get("t_max", 1.0), kw.get("cull", 0), None, None, None, None, None, None, None)
    assert rq(nq=0) == 0
    assert rq() != 0 and b"null pointer" in lib.sp3_last_error()
    assert rq(t_min=2.0) != 0 and b"t_min" in lib.sp3_last_error()
    assert rq(cull=3) != 0 and b"cull" in lib.sp3_last_error()
    assert rq(b=table(100, [25, 6, 2, 1])) != 0 and b"level 1" in lib.sp3_last_error()
    rv = lambda T, b=good: lib.sp3_mesh_bvh_ray_views(None, None, T, 0.0, None, 3, None, 100, None, None, None, b, None, None)
    assert rv(0) == 0 and rv(2) != 0 and b"null pointer" in lib.sp3_last_error()
    assert rv(-1) != 0 and b"T -1" in lib.sp3_last_error()
    assert lib.sp3_mesh_bvh_build(None, 3, None, 100, None, good, None, None, None) != 0 and b"null pointer" in lib.sp3_last_error()
    assert lib.sp3_mesh_bvh_build(None, 3, None, 100, None, table(100, [25, 7, 1]), None, None, None) != 0 and b"level 2" in lib.sp3_last_error()
    box = (C.c_float * 6)(0, 0, 0, 1, 1, 1)
    assert lib.sp3_mesh_bvh_keys(None, 3, None, 0, box, None, None) != 0 and b"point form" in lib.sp3_last_error()
    assert lib.sp3_mesh_bvh_keys(None, 0, None, 0, box, None, None) == 0                # nothing to key
    assert lib.sp3_mesh_bvh_keys(None, 3, None, 3, box, None, None) != 0 and b"null" in lib.sp3_last_error()
    assert lib.sp3_mesh_bvh_keys(None, 3, None, 3, (C.c_float * 6)(0, 0, 0, 1, math.nan, 1), None, None) != 0 and b"box" in lib.sp3_last_error()
    assert lib.sp3_mesh_bvh_keys(None, 3, None, 3, None, None, None) != 0 and b"null box" in lib.sp3_last_error()
    # the keys on the device are the restatement's
    verts, faces = RR.bumpy_sheet()
    bv = M.TriangleBVH(_mesh(verts, faces))
    pts = np.concatenate([np.random.default_rng(1).uniform(-1, 2, (500, 3)), [(np.nan, 0, 0), (0, 0, np.inf)]]).astype(np.float32)
    keys = bv._keys(lib, _t(pts), None, len(pts)).cpu().numpy()
    assert np.array_equal(keys, B.point_keys(pts, B.finite_box(verts))) and (keys[-2:] == B.KEY_NONE).all()
    assert np.array_equal(bv.query_order(_t(pts)).cpu().numpy(), np.argsort(keys, kind="stable"))


def test_demo_loop_rejects_eval_bvh_without_an_evaluation_that_queries_faces(monkeypatch, capsys):
    import demo_loop
    monkeypatch.setattr(sys, "argv", ["demo_loop.py", "--tiny", "--eval_bvh"])
    with pytest.raises(SystemExit) as e:
        demo_loop.main()
    assert e.value.code == 2 and "--eval_bvh needs --eval_exact or --eval_depth" in capsys.readouterr().err
