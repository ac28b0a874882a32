"""sp3_mesh_ray_query, sp3_mesh_ray_brute and sp3_mesh_ray_views on the device (csrc/mesh_ray.hip; include/spann3r_hip.h "Mesh
rays") and what drives them: mesh.ray_mesh_intersect / render_depth_maps and evaluate.evaluate_depth.

The anchor is tests/mesh_ray_ref.py (the numpy restatement, checked against exact rationals and a pair-by-pair loop in
tests/test_mesh_ray_cpu.py).  Every comparison with it is exact: t, bary and point bit for bit, face and side equal.  The result is a
pure function of the inputs, so the grid walk, the brute-force kernels and the restatement must agree whatever the grid."""
import ctypes as C
import math
import sys

import numpy as np
import pytest
import torch

import bricks_ref as BR
import mesh_ray_ref as R
import raycast_ref as RC

pytestmark = pytest.mark.gpu

S = BR.SCENE
KEYS = ("t", "face", "bary", "point", "side")


def _t(x):
    return torch.from_numpy(np.array(x)).cuda()


def _mesh(verts, faces):
    return dict(vertices=_t(np.asarray(verts, np.float32).reshape(-1, 3)), faces=_t(np.asarray(faces, np.int32).reshape(-1, 3)), bounds=None)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _assert_same(got, want, what=""):
    """a device result dict (or a second one) against the restatement's: bit for bit"""
    g = {k: (got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]) for k in KEYS}
    w = {k: (want[k].cpu().numpy() if isinstance(want[k], torch.Tensor) else want[k]) for k in KEYS}
    assert g["t"].dtype == np.float32 and g["bary"].dtype == np.float32 and g["point"].dtype == np.float32
    assert g["face"].dtype == np.int32 and g["side"].dtype == np.uint8 and g["bary"].shape == g["point"].shape == (len(g["t"]), 3)
    bad = np.flatnonzero(g["face"] != w["face"])
    assert len(bad) == 0, "%s: %d faces differ, first at ray %d: %d vs %d" % (what, len(bad), bad[0], g["face"][bad[0]], w["face"][bad[0]])
    assert np.array_equal(g["side"], w["side"]), what
    for k in ("t", "bary", "point"):
        assert np.array_equal(_bits(g[k]), _bits(w[k])), "%s: %s" % (what, k)


def _check(m, verts, faces, o, d, want=None, grid=None, what="", **kw):
    """grid walk == brute force == restatement for these rays; -> (the grid result with stats, the restatement)"""
    from spann3r_amd import mesh as M
    want = R.intersect(o, d, verts, faces, **kw) if want is None else want
    o, d = _t(np.asarray(o, np.float32)), _t(np.asarray(d, np.float32))
    got = M.ray_mesh_intersect(o, d, m, grid=grid, return_stats=True, **kw)
    _assert_same(got, want, what + " grid")
    _assert_same(M.ray_mesh_intersect(o, d, m, method="brute", **kw), want, what + " brute")
    return got, want


# ------------------------------------------------------------------------------------------------ 1. one triangle
TRI_V = np.array([(0, 0, 0), (2, 0, 0), (0, 2, 0)], np.float32)                 # counter-clockwise seen from z > 0
TRI_F = np.array([[0, 1, 2]], np.int32)
EYE = np.array((0.25, 0.5, 4), np.float32)                # d_z = -4: every operation of the rule on rays 3..8 is exact
TRI_RAYS = [((0.5, 0.5, 1), (0, 0, -1)), ((0.5, 0.5, -1), (0, 0, 2)),            # 0, 1: the interior, from the front and from the back
            ((0.25, 0.25, 2), (0.5, 0.25, -2)),                                  # 2: oblique
            (EYE, (1, 0, 0) - EYE), (EYE, (0, 1, 0) - EYE), (EYE, (1, 1, 0) - EYE),      # 3..5: onto each edge
            (EYE, (0, 0, 0) - EYE), (EYE, (2, 0, 0) - EYE), (EYE, (0, 2, 0) - EYE),      # 6..8: onto each vertex
            ((-1, 0.5, 0), (1, 0, 0)), ((0.5, 0.5, 0), (1, 1, 0)),               # 9, 10: in its plane
            ((-1, 0.5, 0.5), (1, 0, 0)),                                         # 11: parallel above it
            ((0.5, 0.5, 1), (0, 0, 1)), ((0.5, 0.5, -1), (0, 0, -1)),            # 12, 13: it lies behind the start
            ((3, 3, 1), (0, 0, -1)),                                             # 14: past it
            ((0.5, 0.5, 0), (0, 0, 1))]                                          # 15: starting on it: t = +0
TRI_O = np.array([r[0] for r in TRI_RAYS], np.float32)
TRI_D = np.array([r[1] for r in TRI_RAYS], np.float32)


def test_one_triangle_from_every_direction():
    from spann3r_amd import mesh as M
    m = _mesh(TRI_V, TRI_F)
    grid = M.TriangleGrid(m)
    one = M.TriangleGrid(m, h=100.0)
    assert grid.dims != (1, 1, 1) and grid.pairs >= 1 and one.dims == (1, 1, 1) and one.pairs == 0
    got, want = _check(m, TRI_V, TRI_F, TRI_O, TRI_D, grid=grid, what="triangle")
    _check(m, TRI_V, TRI_F, TRI_O, TRI_D, want=want, grid=one, what="one cell")
    assert want["face"].tolist() == [0] * 9 + [-1] * 6 + [0]
    # the side: det > 0 = front = the origin sees A, B, C counter-clockwise
    assert want["side"].tolist() == [0, 1, 0] + [0] * 6 + [255] * 6 + [1]
    assert want["t"][:2].tolist() == [1.0, 0.5] and want["t"][15] == 0 and not np.signbit(want["t"][15]) and np.isinf(want["t"][9:15]).all()
    assert want["point"][0].tolist() == [0.5, 0.5, 0.0] and want["bary"][0].tolist() == [0.5, 0.25, 0.25]
    assert (want["point"][9:15] == TRI_O[9:15]).all() and (want["bary"][9:15] == 0).all()
    for g in (grid, one):
        back, _ = _check(m, TRI_V, TRI_F, TRI_O, TRI_D, grid=g, what="cull back", cull="back")
        front, _ = _check(m, TRI_V, TRI_F, TRI_O, TRI_D, grid=g, what="cull front", cull="front")
        assert back["face"].cpu().tolist() == [0, -1] + [0] * 7 + [-1] * 7
        assert front["face"].cpu().tolist() == [-1, 0] + [-1] * 13 + [0]
        # the range cuts the hit off on either end and holds exactly at it (ray 0 hits at t = 1, ray 1 at 0.5)
        for t_min, t_max, hit0 in ((0.0, 0.5, False), (1.5, math.inf, False), (1.0, 1.0, True), (0.0, 1.0, True), (1.0, 2.0, True), (0.75, 0.875, False)):
            r, _ = _check(m, TRI_V, TRI_F, TRI_O[:2], TRI_D[:2], grid=g, what="range %g %g" % (t_min, t_max), t_min=t_min, t_max=t_max)
            assert (int(r["face"][0]) == 0) == hit0 and (int(r["face"][1]) == 0) == (t_min <= 0.5 <= t_max)


# ------------------------------------------------------------------------------------------------ 2. shared edges, copies, permutations
def test_a_shared_edge_copies_and_permuted_faces():
    from spann3r_amd import mesh as M
    verts = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], np.float32)
    faces = np.array([(0, 1, 2), (0, 2, 3)], np.int32)                           # the diagonal (0, 0) - (1, 1) is shared
    # dyadic coordinates and d_z = -1: every operation of the rule is exact, so U = 0 on the diagonal for both faces
    k = np.arange(1, 8) / 8.0
    tgt = np.stack([k, k, np.zeros_like(k)], 1)
    off = np.array([(0, 0, 1), (0.25, -0.5, 1), (-0.75, 0.125, 1), (0.5, 0.5, 1)])
    o = (tgt[:, None] + off[None]).reshape(-1, 3).astype(np.float32)
    d = (np.repeat(tgt, len(off), 0) - o).astype(np.float32)
    m = _mesh(verts, faces)
    got, want = _check(m, verts, faces, o, d, what="shared edge")
    assert (want["face"] == 0).all() and (want["t"] == 1).all() and (want["bary"][:, 1] == 0).all()
    swapped = faces[::-1].copy()
    _, w2 = _check(_mesh(verts, swapped), verts, swapped, o, d, what="shared edge, swapped")
    assert (w2["face"] == 0).all() and np.array_equal(_bits(w2["t"]), _bits(want["t"]))
    # rays aimed at inexact points of the diagonal from inexact origins: one of the two faces always takes them
    rng = np.random.default_rng(2)
    s = rng.uniform(0.01, 0.99, 512)
    o2 = rng.uniform(-1, 2, (512, 3)) + (0, 0, 3)
    d2 = np.stack([s, s, np.zeros_like(s)], 1) - o2
    _, w3 = _check(m, verts, faces, o2, d2, what="diagonal")
    assert (w3["face"] >= 0).all()
    # exact copies of a face: the smallest index wins
    copies = np.array([(0, 1, 2)] * 3 + [(0, 2, 3)] * 2, np.int32)
    oc = np.array([(0.75, 0.25, 1), (0.25, 0.75, 1)], np.float32)
    dc = np.array([(0, 0, -1), (0, 0, -1)], np.float32)
    _, wc = _check(_mesh(verts, copies), verts, copies, oc, dc, what="copies")
    assert wc["face"].tolist() == [0, 3]
    # permuted faces: t unchanged bit for bit
    sv, sf = R.bumpy_sheet()
    perm = np.random.default_rng(3).permutation(len(sf))
    o3 = rng.uniform((0, -0.5, 0.5), (1, 0.5, 1.0), (256, 3)).astype(np.float32)
    d3 = (rng.uniform((0, -0.5, -0.05), (1, 0.5, 0.05), (256, 3)) - o3).astype(np.float32)
    a = M.ray_mesh_intersect(_t(o3), _t(d3), _mesh(sv, sf))
    b = M.ray_mesh_intersect(_t(o3), _t(d3), _mesh(sv, sf[perm]))
    assert torch.equal(a["t"].view(torch.int32), b["t"].view(torch.int32)) and int((a["face"] >= 0).sum()) > 192


# ------------------------------------------------------------------------------------------------ 3. the bumpy sheet
def _box_missing_rays(lo, hi, rng, n):
    """rays that cannot touch the box [lo, hi] pushed out by 1 %: they start beyond one face of it and do not point back"""
    ext = hi - lo
    o = rng.uniform(lo - ext, hi + ext, (n, 3))
    d = rng.normal(size=(n, 3))
    ax = rng.integers(0, 3, n)
    sg = rng.choice([-1.0, 1.0], n)
    rows = np.arange(n)
    o[rows, ax] = np.where(sg > 0, hi[ax] + ext[ax] * rng.uniform(0.05, 2, n), lo[ax] - ext[ax] * rng.uniform(0.05, 2, n))
    d[rows, ax] = sg * np.abs(d[rows, ax])
    d[::4, :] = 0
    d[::4][np.arange(len(d[::4])), (ax[::4] + 1) % 3] = 1.0          # every fourth: parallel to the face it lies beyond
    return o.astype(np.float32), d.astype(np.float32)


@pytest.fixture(scope="module")
def sheet():
    """(verts, faces, grid-independent rays o, d, the number of leading rays that miss the box)"""
    verts, faces = R.bumpy_sheet()
    rng = np.random.default_rng(7)
    lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
    mo, md = _box_missing_rays(lo, hi, rng, 256)
    rays = [(mo, md)]
    for K, P in ((np.array([[30.0, 0, 15.5], [0, 30.0, 15.5], [0, 0, 1]]), np.diag([1.0, -1.0, -1.0, 1.0])),        # looking down -z
                 (np.array([[22.0, 0, 12.0], [0, 26.0, 19.0], [0, 0, 1]]), None)):
        if P is None:
            P = np.eye(4)
            a = 2.8
            P[:3, :3] = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
        P = P.copy()
        P[:3, 3] = (0.5, 0.1, 0.9)
        rays.append(R.camera_rays(K, P, (32, 32)))
    ext = hi - lo
    centre = (lo + hi) / 2
    dirs = rng.normal(size=(512, 3))
    out_o = centre + 3 * dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    rays.append((out_o, rng.uniform(lo, hi, (512, 3)) - out_o))                      # from outside the box, towards it
    in_o = rng.uniform(lo, hi, (512, 3))
    rays.append((in_o, rng.normal(size=(512, 3))))                                   # from inside, pointing out
    zo = rng.uniform(lo - 0.2 * ext, hi + 0.2 * ext, (384, 3)) + (0, 0, 0.3)
    zd = rng.normal(size=(384, 3))
    zd[:192, 0] = 0                                                                  # one zero component ...
    zd[192:, :2] = 0                                                                 # ... and two: straight down or up
    rays.append((zo, zd))
    bad = np.zeros((64, 3), np.float32) + (0.5, 0.0, 0.5)
    bd = np.tile(np.array([(0, 0, -1)], np.float32), (64, 1))
    bad[0:8, 0] = np.nan
    bad[8:16, 2] = np.inf
    bd[16:24, 1] = np.nan
    bd[24:32, 2] = -np.inf
    bd[32:48] = 0                                                                    # d = 0
    rays.append((bad, bd))                                                           # (48..63 stay plain hits)
    o = np.concatenate([np.asarray(r[0], np.float64) for r in rays]).astype(np.float32)
    d = np.concatenate([np.asarray(r[1], np.float64) for r in rays]).astype(np.float32)
    return verts, faces, o, d, 256


def _grid_rays(grid, verts):
    """rays that depend on the grid: axis-parallel ones lying exactly on cell walls, and ones through cell corners along the diagonal"""
    g = grid.g
    wall = lambda o, i: np.float32(np.float64(np.float32(o)) + np.float64(i) * np.float64(np.float32(g.h)))      # origin + i h, the product exact
    org, n = (g.ox, g.oy, g.oz), (g.nx, g.ny, g.nz)
    o, d = [], []
    for i in range(1, n[0], max(n[0] // 6, 1)):
        for j in range(1, n[1], max(n[1] // 6, 1)):
            x, y = wall(org[0], i), wall(org[1], j)
            o += [(x, y, 1.0), (x, -2.0, 0.01), (-2.0, y, 0.01)]
            d += [(0, 0, -1), (0, 1, 0), (1, 0, 0)]                                  # on the walls x = wall(i) and / or y = wall(j)
            c = np.array([x, y, wall(org[2], min(1, n[2] - 1))], np.float64)
            o += [tuple(c - 3 * g.h), tuple(c + 2 * g.h)]
            d += [(g.h, g.h, g.h), (-g.h, -g.h, -g.h)]                               # through the corner along the grid diagonal
    return np.array(o, np.float32), np.array(d, np.float32)


def test_the_bumpy_sheet_grid_brute_and_restatement(sheet):
    from spann3r_amd import mesh as M
    verts, faces, o, d, n_miss = sheet
    m = _mesh(verts, faces)
    grid = M.TriangleGrid(m)
    assert len(faces) == 2 * 31 * 31 and grid.usable == len(faces) and np.prod(grid.dims) > 27
    go, gd = _grid_rays(grid, verts)
    n_pad = 4096 - len(o) - len(go)
    assert n_pad >= 0
    rng = np.random.default_rng(8)
    po = rng.uniform(-1, 2, (n_pad, 3)).astype(np.float32)
    pd = rng.normal(size=(n_pad, 3)).astype(np.float32)
    o, d = np.concatenate([o, go, po]), np.concatenate([d, gd, pd])
    assert len(o) == 4096
    got, want = _check(m, verts, faces, o, d, grid=grid, what="sheet")
    hits = int((want["face"] >= 0).sum())
    print("sheet: grid %s h %.4f pairs %d; %d of 4096 rays hit; %.1f cells visited and %.1f faces evaluated per ray (brute force: %d)" %
          (grid.dims, grid.h, grid.pairs, hits, got["stats"]["cells_visited"] / 4096, got["stats"]["faces_evaluated"] / 4096, len(faces)))
    assert 1024 < hits < 4096 and (want["face"][:n_miss] == -1).all()
    assert 0 < got["stats"]["faces_evaluated"] < 4096 * len(faces) // 4 and got["stats"]["cells_visited"] <= 4096 * sum(grid.dims)
    # the rays that miss the box evaluate nothing and visit nothing
    miss = M.ray_mesh_intersect(_t(o[:n_miss]), _t(d[:n_miss]), m, grid=grid, return_stats=True)
    assert miss["stats"]["faces_evaluated"] == 0 and miss["stats"]["cells_visited"] == 0 and bool((miss["face"] == -1).all())
    # non-finite and zero rays hit nothing; the plain rays next to them do
    bad0 = 256 + 2048 + 512 + 512 + 384
    assert (want["face"][bad0:bad0 + 48] == -1).all() and (want["face"][bad0 + 48:bad0 + 64] >= 0).all()
    # another grid, a range and culling: still the restatement
    coarse = M.TriangleGrid(m, h=4 * grid.h)
    assert coarse.dims != grid.dims and coarse.pairs > 0
    _check(m, verts, faces, o, d, want=want, grid=coarse, what="sheet, coarse grid")
    _check(m, verts, faces, o[256:1280], d[256:1280], grid=grid, what="sheet, range and cull", t_min=0.25, t_max=0.95, cull="back")
    # the same bits a second time
    again = M.ray_mesh_intersect(_t(o), _t(d), m, grid=grid)
    assert all(np.array_equal(again[k].cpu().numpy().view(np.uint8), got[k].cpu().numpy().view(np.uint8)) for k in KEYS)      # (NaN origins come back as they are)


def test_consistency_with_point_mesh_distance(sheet):
    """The fp64 point of a hit lies on its face to fp64 rounding; `point` is that rounded to fp32 per axis, at most half an fp32 ulp
    of the largest |coordinate| per axis, sqrt(3) / 2 < 1 ulp in length."""
    from spann3r_amd import mesh as M
    verts, faces, o, d, n_miss = sheet
    m = _mesh(verts, faces)
    grid = M.TriangleGrid(m)
    r = M.ray_mesh_intersect(_t(o), _t(d), m, grid=grid)
    hit = r["face"] >= 0
    pm = M.point_mesh_distance(r["point"][hit].contiguous(), m, grid=grid)
    ulp = float(np.spacing(np.float32(np.abs(verts).max())))
    print("sibling: %d hits, largest distance of a hit point to the surface %.3e (one fp32 ulp of the scene: %.3e)" %
          (int(hit.sum()), float(pm["dist"].max()), ulp))
    assert float(pm["dist"].max()) <= ulp
    inside = pm["region"] == 6
    assert int(inside.sum()) > 0 and torch.equal(pm["face"][inside], r["face"][hit][inside])


# ------------------------------------------------------------------------------------------------ 4. bad faces
def test_bad_faces_among_good_ones():
    from spann3r_amd import mesh as M
    verts = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0.5, 0.5, 0), (np.nan, 0, 0), (0, np.inf, 0), (2, 2, 0)], np.float32)
    faces = np.array([(0, 1, 4), (0, 0, 1), (0, 4, 2), (0, 1, 9), (-1, 1, 2), (1, 3, 4), (0, 4, 3), (0, 1, 5), (2, 6, 3), (3, 2, 4), (1, 1, 1)], np.int32)
    assert R.usable(verts, faces).tolist() == [True, False, True, False, False, True, False, False, False, True, False]
    rng = np.random.default_rng(4)
    o = rng.uniform(-0.2, 1.2, (512, 3)) + (0, 0, 1)
    d = np.concatenate([rng.uniform(-0.2, 1.2, (512, 2)), np.zeros((512, 1))], 1) - o
    m = _mesh(verts, faces)
    got, want = _check(m, verts, faces, o, d, what="bad faces")
    assert set(np.unique(want["face"]).tolist()) == {-1, 0, 2, 5, 9}
    bad = faces[[1, 3, 4, 6, 7, 8, 10]]
    for method in ("grid", "brute"):
        with pytest.raises(ValueError, match="none valid"):
            M.ray_mesh_intersect(_t(o.astype(np.float32)), _t(d.astype(np.float32)), _mesh(verts, bad), method=method)
    with pytest.raises(ValueError, match="none valid"):
        M.render_depth_maps(_mesh(verts, bad), np.array([[10.0, 0, 2], [0, 10.0, 2], [0, 0, 1]]), np.eye(4), (4, 4))


# ------------------------------------------------------------------------------------------------ 5. the icosphere
def test_the_icosphere_is_watertight_on_the_device():
    from spann3r_amd import mesh as M
    verts, faces = R.icosphere(3)
    lo, hi = R.sphere_radial_bounds(verts, faces)
    m = _mesh(verts, faces)
    grid = M.TriangleGrid(m)
    assert grid.pairs > 0
    for origin in R.SPHERE_ORIGINS:
        o, d = R.sphere_rays(verts, faces, origin)
        got, want = _check(m, verts, faces, o, d, grid=grid, what="icosphere")
        brute = M.ray_mesh_intersect(_t(o), _t(d), m, method="brute")
        assert bool((got["face"] >= 0).all()) and bool((brute["face"] >= 0).all()) and bool((got["side"] == 1).all())
        rad = got["point"].double().norm(dim=1)
        assert float(rad.min()) >= lo - 2.4e-7 and float(rad.max()) <= hi + 2.4e-7
    # from outside towards the centre: the front, and the first of the two crossings
    o = (3 * verts[::3]).astype(np.float32)
    got, want = _check(m, verts, faces, o, -o, grid=grid, what="icosphere from outside")
    assert (want["side"] == 0).all() and (want["t"] < 0.7).all() and (want["t"] > 0.66).all()


# ------------------------------------------------------------------------------------------------ 6. render_depth_maps
def _sheet_cameras():
    K = np.array([[[16.0, 0, 10.25], [0, 15.0, 6.5], [0, 0, 1]], [[11.0, 0, 9.0], [0, 12.5, 5.75], [0, 0, 1]]])
    P = np.stack([np.diag([1.0, -1.0, -1.0, 1.0]), np.eye(4)])
    a = 2.4
    P[1, :3, :3] = np.array([[math.cos(0.3), 0, math.sin(0.3)], [0, 1, 0], [-math.sin(0.3), 0, math.cos(0.3)]]) @ \
        np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    P[0, :3, 3] = (0.5, 0.0, 0.8)
    P[1, :3, 3] = (0.3, 0.4, 0.7)
    return K, P


def test_render_depth_maps_equals_ray_mesh_intersect_on_the_same_rays(sheet):
    from spann3r_amd import mesh as M
    verts, faces = sheet[:2]
    m = _mesh(verts, faces)
    grid = M.TriangleGrid(m)
    K, P = _sheet_cameras()
    h, w = 13, 21                                                     # neither a multiple of the 8 x 8 tile
    for off in (0.0, 0.5):
        maps = M.render_depth_maps(m, K, P, (h, w), grid=grid, pixel_offset=off, return_faces=True, return_stats=True)
        assert maps["depth"].shape == (2, h, w) and maps["face"].shape == (2, h, w) and maps["bary"].shape == (2, h, w, 3)
        nhit = 0
        for i in range(2):
            o, d = R.camera_rays(K[i], P[i], (h, w), off)
            want = R.intersect(o, d, verts, faces)
            r = M.ray_mesh_intersect(_t(o), _t(d), m, grid=grid)
            _assert_same(r, want, "camera %d" % i)
            depth, face, bary = (maps[k][i].cpu().numpy() for k in ("depth", "face", "bary"))
            hit = want["face"] >= 0
            nhit += int(hit.sum())
            assert np.array_equal(face.reshape(-1), want["face"]) and np.array_equal(_bits(bary.reshape(-1, 3)), _bits(want["bary"]))
            assert np.array_equal(_bits(depth.reshape(-1)), _bits(np.where(hit, want["t"], np.float32(0))))
            assert ((depth == 0) == (face == -1)).all()
        assert h * w // 2 < nhit < 2 * h * w and maps["stats"]["faces_evaluated"] > 0
    ref = M.render_depth_maps(m, K, P, (h, w), grid=grid, return_faces=True)
    # the poses as pyrender takes them: columns 1 and 2 negated
    gl = P * np.array([1.0, -1.0, -1.0, 1.0])
    flipped = M.render_depth_maps(m, K, gl, (h, w), grid=grid, opengl=True, return_faces=True)
    assert all(torch.equal(flipped[k].view(torch.int32), ref[k].view(torch.int32)) for k in ("depth", "face", "bary"))
    # near / far cut as t_min / t_max do
    near, far = 0.75, 0.8125
    cut = M.render_depth_maps(m, K, P, (h, w), near=near, far=far, return_faces=True)          # (builds its own grid)
    for i in range(2):
        o, d = R.camera_rays(K[i], P[i], (h, w))
        want = R.intersect(o, d, verts, faces, t_min=near, t_max=far)
        assert np.array_equal(cut["face"][i].cpu().numpy().reshape(-1), want["face"])
        assert np.array_equal(_bits(cut["depth"][i].cpu().numpy().reshape(-1)), _bits(np.where(want["face"] >= 0, want["t"], np.float32(0))))
    assert 0 < int((cut["face"] >= 0).sum()) < int((ref["face"] >= 0).sum())
    # T = 1, one [4, 4] pose, one [3, 3] K
    for pose in (P[:1], P[0], _t(P[0])):
        one = M.render_depth_maps(m, K[0], pose, (h, w), grid=grid)
        assert sorted(one) == ["depth"] and torch.equal(one["depth"].view(torch.int32), ref["depth"][:1].view(torch.int32))
    none = M.render_depth_maps(m, K[0], np.zeros((0, 4, 4)), (h, w), grid=grid, return_faces=True)
    assert none["depth"].shape == (0, h, w) and none["face"].shape == (0, h, w)


def _plane_views(depth_value, poses, K, size, holes=True):
    h, w = size
    views = []
    for P in poses:
        valid = torch.ones((1, h, w), dtype=torch.bool, device="cuda")
        if holes:
            valid[0, 2:5, 3:9] = False
            valid[0, ::4, ::3] = False
        views.append(dict(depthmap=torch.full((1, h, w), depth_value, dtype=torch.float32, device="cuda"), valid_mask=valid,
                          camera_intrinsics=torch.from_numpy(K[None].astype(np.float32)), camera_pose=torch.from_numpy(P[None].astype(np.float32))))
    return views


def test_the_plane_renders_at_its_depth_and_scores_as_derived():
    from spann3r_amd import evaluate as E, mesh as M
    verts, faces = R.plane(9, 2.0)
    m = _mesh(verts, faces)
    K = np.array([[14.0, 0, 9.5], [0, 14.0, 7.0], [0, 0, 1]])
    size = (15, 20)
    P0, P1 = np.eye(4), np.eye(4)
    P1[:3, 3] = (0.125, -0.125, 0.0)
    maps = M.render_depth_maps(m, K, np.stack([P0, P1]), size, return_faces=True)
    assert bool((maps["face"] >= 0).all()) and bool((maps["depth"] == 2.0).all())
    # a one-cell grid: every face per ray, the same maps
    one = M.TriangleGrid(m, h=100.0)
    assert one.pairs == 0
    maps1 = M.render_depth_maps(m, K, np.stack([P0, P1]), size, grid=one, return_faces=True)
    assert all(torch.equal(maps1[k].view(torch.int32), maps[k].view(torch.int32)) for k in ("depth", "face", "bary"))
    # the prediction at 2.0 against a ground truth of 2.2 on a mask with holes
    r = E.evaluate_depth(m, _plane_views(2.2, (P0, P1), K, size))
    print("evaluate_depth:", r)
    assert abs(r["abs_rel"] - 1 / 11) < 1e-6 and abs(r["rmse"] - 0.2) < 1e-6 and r["delta1"] == 1.0 and r["coverage"] == 1.0 and r["views"] == 2
    assert sorted(r) == ["abs_rel", "coverage", "delta1", "pixels", "rmse", "views"] and 0 < r["pixels"] < 2 * 15 * 20
    # delta1: 2.0 against 1.5 is a ratio of 1.333
    assert E.evaluate_depth(m, _plane_views(1.5, (P0,), K, size))["delta1"] == 0.0
    # a camera above the plane's edge x = 1.5: the ray of pixel u reaches x = 1.5 + 2 (u - 9.5) / 14, on the plane for u <= 9: half
    P2 = np.eye(4)
    P2[:3, 3] = (1.5, 0.0, 0.0)
    r2 = E.evaluate_depth(m, _plane_views(2.2, (P2,), K, size, holes=False))
    assert r2["coverage"] == 0.5 and r2["pixels"] == 15 * 10 and abs(r2["abs_rel"] - 1 / 11) < 1e-6
    # far in front of the plane: nothing to compare
    r3 = E.evaluate_depth(m, _plane_views(2.2, (P0,), K, size), far=1.0)
    assert r3["coverage"] == 0.0 and r3["pixels"] == 0 and math.isnan(r3["abs_rel"])


# ------------------------------------------------------------------------------------------------ 7. the brick scene
@pytest.fixture(scope="module")
def brick():
    from spann3r_amd import fusion as F_
    frs = RC.scene_frames()
    vol = F_.BrickTSDFVolume(S["origin"], S["voxel"], S["dims"], trunc=S["trunc"], band=S["band"])
    vol.integrate(intrinsics=[f["K"] for f in frs], cam2world=[f["cam2world"] for f in frs], valid=[_t(f["valid"]) for f in frs],
                  pts=[_t(f["pts"]) for f in frs], images=[_t(f["images"]) for f in frs])
    return vol, frs


@pytest.mark.parametrize("direct", [True, False])
def test_the_fused_surface_seen_from_a_camera(brick, direct):
    from spann3r_amd import mesh as M
    vol, frs = brick
    mesh = vol.extract_mesh(direct=direct)
    grid = M.TriangleGrid(mesh)
    K = np.asarray(frs[2]["K"], np.float64).copy()
    K[:2] *= 0.5                                                      # the frame's 48 x 64 camera at 24 x 32
    P = np.asarray(frs[2]["cam2world"], np.float64)
    o, d = R.camera_rays(K, P, (24, 32))
    g = M.ray_mesh_intersect(_t(o), _t(d), mesh, grid=grid, return_stats=True)
    b = M.ray_mesh_intersect(_t(o), _t(d), mesh, method="brute")
    assert all(torch.equal(g[k], b[k]) for k in ("face", "side")) and all(torch.equal(g[k].view(torch.int32), b[k].view(torch.int32)) for k in ("t", "bary", "point"))
    maps = M.render_depth_maps(mesh, K, P, (24, 32), grid=grid, return_faces=True)
    assert torch.equal(maps["face"].reshape(-1), g["face"])
    assert torch.equal(maps["depth"].reshape(-1).view(torch.int32), torch.where(g["face"] >= 0, g["t"], torch.zeros_like(g["t"])).view(torch.int32))
    nf = mesh["faces"].shape[0]
    hits = int((g["face"] >= 0).sum())
    print("brick scene (%s): %d faces, grid %s, %d pairs; %d of 768 rays hit; %.1f cells and %.1f faces per ray" %
          ("direct" if direct else "dense", nf, grid.dims, grid.pairs, hits, g["stats"]["cells_visited"] / 768, g["stats"]["faces_evaluated"] / 768))
    assert hits > 0 and g["stats"]["faces_evaluated"] < 768 * nf // 8
    want = R.intersect(o[:48], d[:48], mesh["vertices"].cpu().numpy(), mesh["faces"].cpu().numpy())
    _assert_same({k: g[k][:48] for k in KEYS}, want, "brick scene")


# ------------------------------------------------------------------------------------------------ 8. empty sizes and argument errors
def test_empty_sizes_and_argument_errors():
    from spann3r_amd import lib as L, mesh as M
    m = _mesh(TRI_V, TRI_F)
    e = torch.empty((0, 3), dtype=torch.float32, device="cuda")
    for method in ("grid", "brute"):
        r = M.ray_mesh_intersect(e, e, m, method=method, return_stats=True)
        assert r["t"].shape == (0,) and r["bary"].shape == (0, 3) and r["point"].shape == (0, 3) and r["face"].dtype == torch.int32
        assert r["side"].dtype == torch.uint8 and r["stats"]["faces_evaluated"] == 0
    o, d = _t(TRI_O), _t(TRI_D)
    with pytest.raises(ValueError, match="method"):
        M.ray_mesh_intersect(o, d, m, method="bvh")
    with pytest.raises(ValueError, match="cull"):
        M.ray_mesh_intersect(o, d, m, cull="both")
    for t_min, t_max in ((-1.0, 1.0), (2.0, 1.0), (math.nan, 1.0), (0.0, math.nan)):
        with pytest.raises(ValueError, match="t_min"):
            M.ray_mesh_intersect(o, d, m, t_min=t_min, t_max=t_max)
    with pytest.raises(RuntimeError, match=r"fp32 \[N, 3\]"):
        M.ray_mesh_intersect(o.double(), d, m)
    with pytest.raises(RuntimeError, match=r"fp32 \[N, 3\]"):
        M.ray_mesh_intersect(o, d[:, :2], m)
    with pytest.raises(RuntimeError, match="origins and"):
        M.ray_mesh_intersect(o, d[:3], m)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        M.ray_mesh_intersect(o.cpu(), d, m)
    with pytest.raises(TypeError):
        M.ray_mesh_intersect(TRI_O, d, m)
    with pytest.raises(ValueError, match="no faces"):
        M.ray_mesh_intersect(o, d, dict(vertices=m["vertices"], faces=None))
    # the C entry points
    lib = L.load()
    g = M.TriangleGrid(m).g
    gp = C.byref(g)
    assert lib.sp3_mesh_ray_ws_bytes(-1) == 0 and lib.sp3_mesh_ray_ws_bytes(0) == 32 and lib.sp3_mesh_ray_ws_bytes(5) == 32 + 8 * 12
    q = (None, None, None)
    tail = (None,) * 7
    assert lib.sp3_mesh_ray_query(*q, 0, None, 3, None, 1, None, 1, None, gp, 0.0, 1.0, 0, *tail) == 0                    # nq = 0 launches nothing
    assert lib.sp3_mesh_ray_query(*q, 4, None, 3, None, 1, None, 1, None, gp, 0.0, 1.0, 0, *tail) != 0 and b"null pointer" in lib.sp3_last_error()
    assert lib.sp3_mesh_ray_query(*q, -1, None, 3, None, 1, None, 1, None, gp, 0.0, 1.0, 0, *tail) != 0 and b"out of range" in lib.sp3_last_error()
    assert lib.sp3_mesh_ray_query(*q, 4, None, 3, None, 0, None, 1, None, gp, 0.0, 1.0, 0, *tail) != 0 and b"1 face at least" in lib.sp3_last_error()
    assert lib.sp3_mesh_ray_query(*q, 4, None, 3, None, 1, None, 0, None, gp, 0.0, 1.0, 0, *tail) != 0 and b"npairs" in lib.sp3_last_error()
    assert lib.sp3_mesh_ray_query(*q, 4, None, 3, None, 1, None, 1, None, gp, 2.0, 1.0, 0, *tail) != 0 and b"t_min" in lib.sp3_last_error()
    assert lib.sp3_mesh_ray_query(*q, 4, None, 3, None, 1, None, 1, None, gp, -1.0, 1.0, 0, *tail) != 0 and b"t_min" in lib.sp3_last_error()
    assert lib.sp3_mesh_ray_query(*q, 4, None, 3, None, 1, None, 1, None, gp, 0.0, 1.0, 3, *tail) != 0 and b"cull" in lib.sp3_last_error()
    bad_grid = L.NnGrid(0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0, 1, 1)
    assert lib.sp3_mesh_ray_query(*q, 4, None, 3, None, 1, None, 1, None, C.byref(bad_grid), 0.0, 1.0, 0, *tail) != 0 and b"grid dims" in lib.sp3_last_error()
    assert lib.sp3_mesh_ray_brute(None, None, 0, None, 3, None, 1, 0.0, 1.0, 0, *tail) == 0
    assert lib.sp3_mesh_ray_brute(None, None, 4, None, 3, None, 1, 0.0, 1.0, 0, *tail) != 0 and b"null pointer" in lib.sp3_last_error()
    assert lib.sp3_mesh_ray_brute(None, None, 4, None, 3, None, 1, 0.0, math.nan, 0, *tail) != 0 and b"t_min" in lib.sp3_last_error()
    assert lib.sp3_mesh_ray_views(None, None, 0, 0.0, None, 3, None, 1, None, 0, None, gp, None, None) == 0                 # T = 0 launches nothing
    assert lib.sp3_mesh_ray_views(None, None, 2, 0.0, None, 3, None, 1, None, 0, None, gp, None, None) != 0 and b"null pointer" in lib.sp3_last_error()
    assert lib.sp3_mesh_ray_views(None, None, 70000, 0.0, None, 3, None, 1, None, 0, None, gp, None, None) != 0 and b"65535" in lib.sp3_last_error()
    # a view the host table refuses: nothing is launched
    table = (L.MeshRayView * 1)()
    table[0].w, table[0].h, table[0].row_stride, table[0].fu, table[0].fv, table[0].far = 4, 4, 2, 1.0, 1.0, 1.0
    ws = torch.zeros(32, dtype=torch.uint8, device="cuda")
    args = (m["vertices"].data_ptr(), 3, m["faces"].data_ptr(), 1, None, 0, None, gp, ws.data_ptr(), None)
    assert lib.sp3_mesh_ray_views(table, ws.data_ptr(), 1, 0.0, *args) != 0 and b"bad geometry" in lib.sp3_last_error()
    table[0].row_stride = 4
    assert lib.sp3_mesh_ray_views(table, ws.data_ptr(), 1, 0.0, *args) != 0 and b"null depth" in lib.sp3_last_error()


def test_demo_loop_rejects_eval_depth_without_a_fused_evaluation(monkeypatch, capsys):
    import demo_loop
    for extra in ([], ["--fused"], ["--fused", "--eval"]):
        monkeypatch.setattr(sys, "argv", ["demo_loop.py", "--tiny", "--eval_depth"] + extra)
        with pytest.raises(SystemExit) as e:
            demo_loop.main()
        assert e.value.code == 2 and "--eval_depth needs --fused --rgbd --eval" in capsys.readouterr().err
