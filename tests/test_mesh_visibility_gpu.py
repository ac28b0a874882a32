"""sp3_mesh_ray_occluded, sp3_mesh_point_views (and their _bvh_ forms) and sp3_mesh_vis_face_class on the device (csrc/ray_kernels.h,
csrc/mesh_ray.hip, csrc/mesh_bvh.hip, csrc/mesh_visibility.hip; include/spann3r_hip.h "Mesh visibility") and what drives them:
mesh.ray_mesh_occluded / point_visibility / vertex_visibility / cull_to_views and evaluate.evaluate_meshes(cull_views=...).

The anchors are tests/mesh_visibility_ref.py (the numpy restatement, checked on hand-built scenes in tests/test_mesh_visibility_cpu.py)
and the closest-hit kernels of "Mesh rays".  Every comparison is exact equality."""
import ctypes as C
import math
import sys

import numpy as np
import pytest
import torch

import mesh_ray_ref as R
import mesh_visibility_ref as V
from test_mesh_distance_gpu import _plane
from test_mesh_ray_gpu import TRI_D, TRI_F, TRI_O, TRI_V, _grid_rays, _mesh, _t, brick, sheet      # noqa: F401 (sheet, brick: fixtures)

pytestmark = pytest.mark.gpu


def _np(x):
    return x.cpu().numpy()


def _occluded_everywhere(m, verts, faces, o, d, grid=None, bvh=None, what="", **kw):
    """ray_mesh_occluded through the grid, the tree and brute force == face >= 0 of ray_mesh_intersect on each == the restatement
    -> the restatement's mask"""
    from spann3r_amd import mesh as M
    want = V.occluded(o, d, verts, faces, kw.get("t_min", 0.0), kw.get("t_max", math.inf), kw.get("cull"))      # (= R.intersect(...)["face"] >= 0)
    o, d = _t(np.asarray(o, np.float32)), _t(np.asarray(d, np.float32))
    bvh = M.TriangleBVH(m) if bvh is None else bvh
    for name, route in (("grid", dict(grid=grid)), ("bvh", dict(bvh=bvh)), ("brute", dict(method="brute"))):
        got = M.ray_mesh_occluded(o, d, m, **route, **kw)
        assert got.dtype == torch.bool and got.shape == (len(want),)
        assert torch.equal(got, M.ray_mesh_intersect(o, d, m, **route, **kw)["face"] >= 0), "%s %s: closest hit" % (what, name)
        bad = np.flatnonzero(_np(got) != want)
        assert len(bad) == 0, "%s %s: %d rays differ from the restatement, first %d" % (what, name, len(bad), bad[0])
    return want


# ------------------------------------------------------------------------------------------------ 1. ray_mesh_occluded
def test_occlusion_of_one_triangle_from_every_direction():
    from spann3r_amd import mesh as M
    m = _mesh(TRI_V, TRI_F)
    grid, one = M.TriangleGrid(m), M.TriangleGrid(m, h=100.0)
    assert grid.pairs >= 1 and one.pairs == 0
    for g in (grid, one):                                                           # (F = 1; the second a grid of one cell)
        want = _occluded_everywhere(m, TRI_V, TRI_F, TRI_O, TRI_D, grid=g, what="triangle")
        assert want.tolist() == [True] * 9 + [False] * 6 + [True]                  # every region; in its plane and behind it: not occluded
        assert _occluded_everywhere(m, TRI_V, TRI_F, TRI_O, TRI_D, grid=g, what="cull back", cull="back").tolist() == [True, False] + [True] * 7 + [False] * 7
        assert _occluded_everywhere(m, TRI_V, TRI_F, TRI_O, TRI_D, grid=g, what="cull front", cull="front").tolist() == [False, True] + [False] * 13 + [True]
        # ranges that cut at and around the hit (ray 0 hits at t = 1, ray 1 at 0.5)
        for t_min, t_max, hit0 in ((0.0, 0.5, False), (1.5, math.inf, False), (1.0, 1.0, True), (0.0, 1.0, True), (1.0, 2.0, True), (0.75, 0.875, False)):
            w = _occluded_everywhere(m, TRI_V, TRI_F, TRI_O[:2], TRI_D[:2], grid=g, what="range", t_min=t_min, t_max=t_max)
            assert w.tolist() == [hit0, t_min <= 0.5 <= t_max]


def test_occlusion_on_the_bumpy_sheet_and_its_counters(sheet):
    """The 4 096 rays of tests/test_mesh_ray_gpu.py.  The counters are a condition: a ray that hits nothing walks exactly the path
    of the closest-hit walk, so over the misses cells / nodes visited and faces evaluated are EQUAL; over the whole set they are no
    larger and the faces strictly fewer (a hit stops the walk)."""
    from spann3r_amd import mesh as M
    verts, faces, o, d, n_miss = sheet
    m = _mesh(verts, faces)
    grid, bvh = M.TriangleGrid(m), M.TriangleBVH(m)
    go, gd = _grid_rays(grid, verts)
    rng = np.random.default_rng(8)
    n_pad = 4096 - len(o) - len(go)
    o = np.concatenate([o, go, rng.uniform(-1, 2, (n_pad, 3)).astype(np.float32)])
    d = np.concatenate([d, gd, rng.normal(size=(n_pad, 3)).astype(np.float32)])
    assert len(o) == 4096
    want = _occluded_everywhere(m, verts, faces, o, d, grid=grid, bvh=bvh, what="sheet")
    assert 1024 < want.sum() < 4096 and not want[:n_miss].any()
    bad0 = 256 + 2048 + 512 + 512 + 384
    assert not want[bad0:bad0 + 48].any() and want[bad0 + 48:bad0 + 64].all()      # NaN, inf and zero rays are not occluded
    _occluded_everywhere(m, verts, faces, o[256:1280], d[256:1280], grid=grid, bvh=bvh, what="sheet, range and cull", t_min=0.25, t_max=0.95, cull="back")
    _occluded_everywhere(m, verts, faces, o, d, grid=M.TriangleGrid(m, h=4 * grid.h), bvh=bvh, what="sheet, coarse grid")
    to, td = _t(o), _t(d)
    mo, md = _t(o[~want]), _t(d[~want])
    for name, route, steps in (("grid", dict(grid=grid), "cells_visited"), ("bvh", dict(bvh=bvh), "nodes_visited")):
        occ, s_any = M.ray_mesh_occluded(to, td, m, return_stats=True, **route)
        s_hit = M.ray_mesh_intersect(to, td, m, return_stats=True, **route)["stats"]
        none, m_any = M.ray_mesh_occluded(mo, md, m, return_stats=True, **route)
        m_hit = M.ray_mesh_intersect(mo, md, m, return_stats=True, **route)["stats"]
        print("sheet, %s: %s per ray %.2f (closest hit %.2f), faces evaluated per ray %.2f (%.2f); over the %d misses %.2f and %.2f for both" %
              (name, steps, s_any[steps] / 4096, s_hit[steps] / 4096, s_any["faces_evaluated"] / 4096, s_hit["faces_evaluated"] / 4096,
               len(mo), m_any[steps] / len(mo), m_any["faces_evaluated"] / len(mo)))
        assert not bool(none.any()) and m_any[steps] == m_hit[steps] > 0 and m_any["faces_evaluated"] == m_hit["faces_evaluated"] > 0
        assert s_any[steps] <= s_hit[steps] and s_any["faces_evaluated"] < s_hit["faces_evaluated"]
        assert sorted(s_any) == sorted(s_hit)


def test_occlusion_with_bad_faces_mixed_in():
    verts = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0.5, 0.5, 0), (np.nan, 0, 0), (0, np.inf, 0), (2, 2, 0)], np.float32)
    faces = np.array([(0, 1, 4), (0, 0, 1), (0, 4, 2), (0, 1, 9), (-1, 1, 2), (1, 3, 4), (0, 4, 3), (0, 1, 5), (2, 6, 3), (3, 2, 4), (1, 1, 1)], np.int32)
    rng = np.random.default_rng(4)
    o = rng.uniform(-0.2, 1.2, (512, 3)) + (0, 0, 1)
    d = np.concatenate([rng.uniform(-0.2, 1.2, (512, 2)), np.zeros((512, 1))], 1) - o
    want = _occluded_everywhere(_mesh(verts, faces), verts, faces, o.astype(np.float32), d.astype(np.float32), what="bad faces")
    assert 0 < want.sum() < 512


def test_occlusion_empty_sizes_and_argument_errors():
    from spann3r_amd import lib as L, mesh as M
    m = _mesh(TRI_V, TRI_F)
    e = torch.empty((0, 3), dtype=torch.float32, device="cuda")
    for route in (dict(), dict(method="brute"), dict(bvh=True)):
        r, stats = M.ray_mesh_occluded(e, e, m, return_stats=True, **route)
        assert r.shape == (0,) and r.dtype == torch.bool and stats["faces_evaluated"] == 0
    o, d = _t(TRI_O), _t(TRI_D)
    with pytest.raises(ValueError, match="method"):
        M.ray_mesh_occluded(o, d, m, method="bvh")
    with pytest.raises(ValueError, match="cull"):
        M.ray_mesh_occluded(o, d, m, cull="both")
    for t_min, t_max in ((-1.0, 1.0), (2.0, 1.0), (math.nan, 1.0)):
        with pytest.raises(ValueError, match="t_min"):
            M.ray_mesh_occluded(o, d, m, t_min=t_min, t_max=t_max)
    with pytest.raises(RuntimeError, match=r"fp32 \[N, 3\]"):
        M.ray_mesh_occluded(o.double(), d, m)
    with pytest.raises(RuntimeError, match="origins and"):
        M.ray_mesh_occluded(o, d[:3], m)
    with pytest.raises(ValueError, match="bvh= replaces the grid"):
        M.ray_mesh_occluded(o, d, m, bvh=True, method="brute")
    with pytest.raises(ValueError, match="no faces"):
        M.ray_mesh_occluded(o, d, dict(vertices=m["vertices"], faces=None))
    # the C entry points: the shared host checks
    lib = L.load()
    gp = C.byref(M.TriangleGrid(m).g)
    q, tail = (None, None, None), (None, None, None)
    assert lib.sp3_mesh_ray_occluded(*q, 0, None, 3, None, 1, None, 1, None, gp, 0.0, 1.0, 0, *tail) == 0                  # nq = 0 launches nothing
    assert lib.sp3_mesh_ray_occluded(*q, 4, None, 3, None, 1, None, 1, None, gp, 0.0, 1.0, 0, *tail) != 0 and b"null pointer" in lib.sp3_last_error()
    assert lib.sp3_mesh_ray_occluded(*q, 4, None, 3, None, 1, None, 0, None, gp, 0.0, 1.0, 0, *tail) != 0 and b"npairs" in lib.sp3_last_error()
    assert lib.sp3_mesh_ray_occluded(*q, 4, None, 3, None, 1, None, 1, None, gp, 2.0, 1.0, 0, *tail) != 0 and b"t_min" in lib.sp3_last_error()
    assert lib.sp3_mesh_ray_occluded(*q, 4, None, 3, None, 1, None, 1, None, gp, 0.0, 1.0, 3, *tail) != 0 and b"cull" in lib.sp3_last_error()
    b = M.TriangleBVH(m)
    tree = (None, None, None, C.byref(b.b))
    assert lib.sp3_mesh_bvh_ray_occluded(*q, 0, None, 3, None, 1, *tree, 0.0, 1.0, 0, *tail) == 0
    assert lib.sp3_mesh_bvh_ray_occluded(*q, 4, None, 3, None, 1, *tree, 0.0, 1.0, 0, *tail) != 0 and b"null pointer" in lib.sp3_last_error()
    assert lib.sp3_mesh_bvh_ray_occluded(*q, 4, None, 3, None, 1, *tree, 0.0, math.nan, 0, *tail) != 0 and b"t_min" in lib.sp3_last_error()


# ------------------------------------------------------------------------------------------------ 2. point_visibility
@pytest.fixture(scope="module")
def cases():
    """every CPU case with the restatement's answer, computed once"""
    return [(c, V.run_case(c)) for c in V.cases()]


def _visibility(c, route, **more):
    from spann3r_amd import mesh as M
    m = _mesh(c["vertices"], c["faces"])
    if route == "grid":
        acc = dict(grid=M.TriangleGrid(m))
    elif route == "one cell":
        acc = dict(grid=M.TriangleGrid(m, h=1e6))
        assert acc["grid"].pairs == 0
    else:
        acc = dict(bvh=M.TriangleBVH(m))
    return M.point_visibility(_t(c["points"]), m, c["K"], c["poses"], c["size"], return_mask=True, **acc, **c["kw"], **more)


@pytest.mark.parametrize("route", ["grid", "bvh", "one cell"])
def test_point_visibility_equals_the_restatement(cases, route):
    for c, want in cases:
        got = _visibility(c, route, return_stats=True)
        assert got["count"].dtype == torch.int32 and got["mask"].dtype == torch.bool and got["mask"].shape == want["mask"].shape
        bad = np.argwhere(_np(got["mask"]) != want["mask"])
        assert len(bad) == 0, "%s through %s: %d pairs differ, first (view, point) %s" % (c["name"], route, len(bad), bad[0])
        assert np.array_equal(_np(got["count"]), want["count"]) and got["views"] == len(c["poses"])
        assert got["stats"]["faces_evaluated"] >= 0 and sorted(got) == ["count", "mask", "stats", "views"]


def test_point_visibility_equals_the_composition_a_user_had_before(cases):
    """frustum tests in torch fp64, then ray_mesh_intersect on the materialised shadow rays with the same t_min / t_max, then face < 0.
    ray_mesh_intersect takes one range for all rays: t_min = near / z is one number where near = 0, and for the cameras with
    near > 0 below the rays are grouped by their z (a handful of distinct values)."""
    from spann3r_amd import mesh as M
    sv, sf = R.icosphere(3)
    m = _mesh(sv, sf)
    rng = np.random.default_rng(11)
    pts = np.concatenate([sv, rng.uniform(-1.5, 1.5, (512, 3)).astype(np.float32)])
    zs = np.array([1.5, 2.0, 2.75, 3.5], np.float32)                                 # exact camera z for the axis camera below
    layers = np.stack([rng.uniform(-0.9, 0.9, 256), rng.uniform(-0.9, 0.9, 256), 3.0 - rng.choice(zs, 256)], 1).astype(np.float32)
    poses = np.stack([V.look_at(V.SPHERE_EYE), V.look_at((0, 0, 3)), V.look_at((-2.5, 0.4, 0.3))])
    # near = 2.25 cuts into the sphere (its top lies at camera z = 2): a point inside it whose shadow ray starts inside too is seen
    for T, near, far, bias in ((3, 0.0, math.inf, 1e-3), (1, 0.0, 2.5, 0.0), (3, 0.0, 3.0, 0.02), (1, 2.25, 3.6, 1e-3)):
        P = poses[:T] if near == 0.0 else poses[1:2]
        p = _t(np.concatenate([pts, layers]) if near == 0.0 else layers)
        got = M.point_visibility(p, m, V.K64, P, V.SIZE64, near=near, far=far, bias=bias, return_mask=True)
        for i, view in enumerate(V.make_views(V.K64, P, V.SIZE64, near, far)):
            W = torch.from_numpy(view["w2c"].astype(np.float64).reshape(3, 4))
            q = p.double().cpu()                                                     # (fp64 on the host: one rounding per operation)
            x, y, z = (((W[k, 0] * q[:, 0] + W[k, 1] * q[:, 1]) + W[k, 2] * q[:, 2]) + W[k, 3] for k in range(3))
            u, v = (x / z) * float(view["fu"]) + float(view["cu"]), (y / z) * float(view["fv"]) + float(view["cv"])
            inside = (z > 0) & (z >= float(view["near"])) & (z <= float(view["far"])) & (u + 0.5 >= 0) & (u + 0.5 < 64) & (v + 0.5 >= 0) & (v + 0.5 < 64)
            o = torch.from_numpy(view["c2w"].reshape(3, 4)[:, 3].copy()).expand(len(p), 3)
            d = (q - o.double()).float().cuda()
            o, inside = o.contiguous().cuda(), inside.cuda()
            free = torch.zeros(len(p), dtype=torch.bool, device="cuda")
            t_min = (float(view["near"]) / z).cuda()
            groups = [0.0] if near == 0.0 else torch.unique(t_min[inside]).tolist()
            assert len(groups) <= 64
            for tm in groups:
                sel = inside if near == 0.0 else inside & (t_min == tm)
                if tm <= 1.0 - float(np.float32(bias)):
                    hit = M.ray_mesh_intersect(o[sel].contiguous(), d[sel].contiguous(), m, t_min=tm, t_max=1.0 - float(np.float32(bias)))["face"]
                    free[sel] = hit < 0
                else:
                    free[sel] = True                                                 # an empty range occludes nothing
            assert torch.equal(got["mask"][i], free), "T %d near %g far %g: view %d" % (T, near, far, i)
            assert 0 < int(free.sum()) < int(inside.sum()) <= len(p)
        assert torch.equal(got["count"], got["mask"].sum(0).int())


def test_point_visibility_opengl_offset_and_ranges_against_the_restatement():
    from spann3r_amd import mesh as M
    sv, sf = R.icosphere(3)
    m = _mesh(sv, sf)
    grid, bvh = M.TriangleGrid(m), M.TriangleBVH(m)
    rng = np.random.default_rng(12)
    pts = np.concatenate([sv, rng.uniform(-1.5, 1.5, (256, 3)).astype(np.float32)])
    poses = np.stack([V.look_at(V.SPHERE_EYE), V.look_at((0, 0, 3)), V.look_at((-2.5, 0.4, 0.3))])
    gl = poses * np.array([1.0, -1.0, -1.0, 1.0])
    for kw in (dict(opengl=True), dict(pixel_offset=0.5), dict(near=1.9, far=2.6), dict(near=0.5, far=2.2, pixel_offset=0.5, cull="back"), dict(bias=0.3)):
        for T in (1, 3):
            P = (gl if kw.get("opengl") else poses)[:T]
            ref_kw = {k: v for k, v in kw.items() if k in ("bias", "pixel_offset", "cull")}
            want = V.point_visibility(pts, sv, sf, V.make_views(V.K64, P, V.SIZE64, kw.get("near", 0.0), kw.get("far", math.inf), kw.get("opengl", False)), **ref_kw)
            for acc in (dict(grid=grid), dict(bvh=bvh)):
                got = M.point_visibility(_t(pts), m, V.K64, P, V.SIZE64, return_mask=True, **acc, **kw)
                assert np.array_equal(_np(got["mask"]), want["mask"]) and np.array_equal(_np(got["count"]), want["count"]), (kw, T, list(acc))
            assert 0 < want["mask"].sum() < want["mask"].size
    # opengl=True on the flipped poses is the plain call on the plain ones
    a = M.point_visibility(_t(pts), m, V.K64, gl, V.SIZE64, opengl=True, grid=grid, return_mask=True)
    b = M.point_visibility(_t(pts), m, V.K64, poses, V.SIZE64, grid=grid, return_mask=True)
    assert torch.equal(a["mask"], b["mask"]) and torch.equal(a["count"], b["count"])
    # vertex_visibility is point_visibility of the mesh's own vertices; the same bits a second time
    vv = M.vertex_visibility(m, V.K64, poses, V.SIZE64, bvh=bvh, return_mask=True)
    assert torch.equal(vv["mask"][:, :], b["mask"][:, :len(sv)]) and torch.equal(vv["count"], M.vertex_visibility(m, V.K64, poses, V.SIZE64, grid=grid)["count"])


def test_point_visibility_empty_sizes_and_argument_errors():
    from spann3r_amd import lib as L, mesh as M
    sv, sf = R.icosphere(1)
    m = _mesh(sv, sf)
    P = V.look_at((0, 0, 3))
    e = torch.empty((0, 3), dtype=torch.float32, device="cuda")
    for acc in (dict(), dict(bvh=True)):
        r = M.point_visibility(e, m, V.K64, P, V.SIZE64, return_mask=True, return_stats=True, **acc)
        assert r["count"].shape == (0,) and r["mask"].shape == (1, 0) and r["stats"]["faces_evaluated"] == 0
        r = M.point_visibility(_t(sv), m, V.K64, np.zeros((0, 4, 4)), V.SIZE64, return_mask=True, **acc)
        assert r["count"].shape == (len(sv),) and not bool(r["count"].any()) and r["mask"].shape == (0, len(sv)) and r["views"] == 0
    p = _t(sv)
    for bias in (-0.1, 1.0, 1.0 - 1e-9, math.nan):
        with pytest.raises(ValueError, match="bias"):
            M.point_visibility(p, m, V.K64, P, V.SIZE64, bias=bias)
    with pytest.raises(ValueError, match="near"):
        M.point_visibility(p, m, V.K64, P, V.SIZE64, near=2.0, far=1.0)
    with pytest.raises(ValueError, match="skew"):
        M.point_visibility(p, m, np.array([[40.0, 1, 31.5], [0, 40.0, 31.5], [0, 0, 1]]), P, V.SIZE64)
    with pytest.raises(ValueError, match="singular"):
        M.point_visibility(p, m, V.K64, np.zeros((4, 4)), V.SIZE64)
    with pytest.raises(ValueError, match="cull"):
        M.point_visibility(p, m, V.K64, P, V.SIZE64, cull="both")
    with pytest.raises(RuntimeError, match=r"fp32 \[N, 3\]"):
        M.point_visibility(p.double(), m, V.K64, P, V.SIZE64)
    with pytest.raises(ValueError, match="no faces"):
        M.vertex_visibility(dict(vertices=m["vertices"], faces=None), V.K64, P, V.SIZE64)
    # the C entry points: the table of views is validated on the host before anything is launched
    lib = L.load()
    g = M.TriangleGrid(m)
    gp = C.byref(g.g)
    assert lib.sp3_mesh_point_views(None, None, 0, 0.0, 0.001, 0, None, None, 5, None, 3, None, 1, None, 0, None, gp, None, None, None, None) == 0
    assert lib.sp3_mesh_point_views(None, None, 2, 0.0, 0.001, 0, None, None, 0, None, 3, None, 1, None, 0, None, gp, None, None, None, None) == 0
    assert lib.sp3_mesh_point_views(None, None, 2, 0.0, 0.001, 0, None, None, 5, None, 3, None, 1, None, 0, None, gp, None, None, None, None) != 0 \
        and b"null pointer" in lib.sp3_last_error()
    assert lib.sp3_mesh_point_views(None, None, 70000, 0.0, 0.001, 0, None, None, 5, None, 3, None, 1, None, 0, None, gp, None, None, None, None) != 0 \
        and b"65535" in lib.sp3_last_error()
    assert lib.sp3_mesh_point_views(None, None, 2, 0.0, 1.0, 0, None, None, 5, None, 3, None, 1, None, 0, None, gp, None, None, None, None) != 0 \
        and b"bias" in lib.sp3_last_error()
    table = (L.MeshVisView * 1)()
    table[0].w, table[0].h, table[0].fu, table[0].fv, table[0].near, table[0].far = 4, 0, 1.0, 1.0, 0.0, 1.0
    ws = torch.zeros(32, dtype=torch.uint8, device="cuda")
    count = torch.zeros(len(sv), dtype=torch.int32, device="cuda")
    args = (p.data_ptr(), None, len(sv), m["vertices"].data_ptr(), len(sv), m["faces"].data_ptr(), len(sf), L.ptr(g.pair_face), g.pairs,
            L.ptr(g.cell_start), gp, ws.data_ptr(), count.data_ptr(), None, None)
    assert lib.sp3_mesh_point_views(table, ws.data_ptr(), 1, 0.0, 0.001, 0, *args) != 0 and b"bad geometry" in lib.sp3_last_error()
    table[0].h, table[0].fu = 4, 0.0
    assert lib.sp3_mesh_point_views(table, ws.data_ptr(), 1, 0.0, 0.001, 0, *args) != 0 and b"focal" in lib.sp3_last_error()
    table[0].fu, table[0].near = 1.0, 2.0
    assert lib.sp3_mesh_point_views(table, ws.data_ptr(), 1, 0.0, 0.001, 0, *args) != 0 and b"near" in lib.sp3_last_error()
    assert not bool(count.any())


# ------------------------------------------------------------------------------------------------ 3. cull_to_views
def _assert_culled_like(got, want, what):
    assert got["vertices"].dtype == torch.float32 and got["faces"].dtype == torch.int32
    assert np.array_equal(_np(got["faces"]), want["faces"]), what
    assert np.array_equal(_np(got["vertices"]).view(np.uint32), want["vertices"].view(np.uint32)), what
    assert got["visibility"]["faces_kept"] == len(want["faces"])


@pytest.mark.parametrize("route", ["grid", "bvh"])
def test_cull_to_views_on_the_icosphere_row_for_row(cases, route):
    from spann3r_amd import mesh as M
    sv, sf = R.icosphere(3)
    colors = np.stack([np.arange(len(sv)) % 256, np.arange(len(sv)) // 256, np.full(len(sv), 7), np.full(len(sv), 255)], 1).astype(np.uint8)
    m = dict(_mesh(sv, sf), colors=_t(colors), label="kept as it is")
    acc = dict(bvh=M.TriangleBVH(m)) if route == "bvh" else dict(grid=M.TriangleGrid(m))
    one = [w for c, w in cases if c["name"] == "icosphere, one camera"][0]
    six = [w for c, w in cases if c["name"] == "icosphere, six cameras"][0]
    P1, P6 = V.look_at(V.SPHERE_EYE), np.stack([V.look_at(e) for e in V.SPHERE_AXES])
    towards = V.facing(sv, sf, V.SPHERE_EYE) > 0
    for mode in ("all", "any"):
        got = M.cull_to_views(m, V.K64, P1, V.SIZE64, mode=mode, return_map=True, **acc)
        want = V.cull_to_views(sv, sf, one["count"], mode=mode)
        _assert_culled_like(got, want, "one camera, %s" % mode)
        assert np.array_equal(_np(got["vertex_views"]), one["count"]) and np.array_equal(_np(got["colors"]), colors[want["vertex_index"]])
        assert got["label"] == "kept as it is" and got["bounds"].shape == (2, 3)
        assert np.array_equal(got["bounds"], np.stack([want["vertices"].min(0), want["vertices"].max(0)]))
        assert got["visibility"] == dict(views=1, vertices_seen=int((one["count"] >= 1).sum()), faces_in=len(sf), faces_kept=len(want["faces"]))
    # mode="all": every face towards the camera, and beyond them only faces AT the silhouette (tests/test_mesh_visibility_cpu.py says why)
    kept_all = V.cull_to_views(sv, sf, one["count"], mode="all")["face_index"]
    assert towards[kept_all].sum() == towards.sum() and len(kept_all) - towards.sum() < towards.sum() // 10
    whole = M.cull_to_views(m, V.K64, P6, V.SIZE64, **acc)
    assert torch.equal(whole["faces"], m["faces"]) and torch.equal(whole["vertices"], m["vertices"]) and torch.equal(whole["colors"], m["colors"])
    two = M.cull_to_views(m, V.K64, P6, V.SIZE64, mode="all", min_views=2, return_map=True, **acc)
    want2 = V.cull_to_views(sv, sf, six["count"], mode="all", min_views=2)
    _assert_culled_like(two, want2, "six cameras, two views")
    assert 0 < two["faces"].shape[0] < len(sf) and bool((two["vertex_views"][_t(want2["vertex_index"])] >= 2).all())
    # faces with an index out of range are dropped and never dereferenced; everything culled is an empty mesh
    broken = np.concatenate([sf[:300], [[0, 1, len(sv)], [-1, 2, 3]], sf[300:]]).astype(np.int32)
    mb = _mesh(sv, broken)
    gotb = M.cull_to_views(mb, V.K64, P6, V.SIZE64, **({"bvh": True} if route == "bvh" else {}))
    assert np.array_equal(_np(gotb["faces"]), sf) and gotb["visibility"]["faces_in"] == len(sf) + 2
    away = M.cull_to_views(m, V.K64, V.look_at((0, 0, 3), target=(0, 0, 6)), V.SIZE64, **acc)
    assert away["faces"].shape == (0, 3) and away["vertices"].shape == (0, 3) and away["colors"].shape == (0, 4) and away["visibility"]["faces_kept"] == 0
    assert M.cull_to_views(m, V.K64, P6, V.SIZE64, min_views=7, **acc)["faces"].shape == (0, 3)
    with pytest.raises(ValueError, match="mode"):
        M.cull_to_views(m, V.K64, P6, V.SIZE64, mode="some")
    with pytest.raises(ValueError, match="min_views"):
        M.cull_to_views(m, V.K64, P6, V.SIZE64, min_views=-1)
    with pytest.raises(ValueError, match="no faces"):
        M.cull_to_views(dict(vertices=m["vertices"], colors=m["colors"], faces=None), V.K64, P6, V.SIZE64)


@pytest.mark.parametrize("direct", [True, False])
def test_the_fused_surface_culled_to_its_own_cameras(brick, direct):
    """Culling the result again changes nothing with mode="all", min_views=1: every kept face has three seen vertices, removing
    faces can only unblock shadow rays, so every vertex of the result is still seen and every face kept."""
    from spann3r_amd import mesh as M
    vol, frs = brick
    mesh = vol.extract_mesh(direct=direct)
    K = np.stack([np.asarray(f["K"], np.float64) for f in frs])
    P = np.stack([np.asarray(f["cam2world"], np.float64) for f in frs])
    size = frs[0]["valid"].shape[-2:]
    g = M.cull_to_views(mesh, K, P, size, mode="all", return_map=True)
    b = M.cull_to_views(mesh, K, P, size, mode="all", bvh=True, return_map=True)
    assert all(torch.equal(g[k], b[k]) for k in ("vertices", "faces", "colors", "vertex_views")) and g["visibility"] == b["visibility"]
    vis = g["visibility"]
    print("brick scene (%s): %d views, %d of %d vertices seen, %d of %d faces kept" %
          ("direct" if direct else "dense", vis["views"], vis["vertices_seen"], mesh["vertices"].shape[0], vis["faces_kept"], vis["faces_in"]))
    assert vis["views"] == len(frs) and 0 < vis["faces_kept"] <= vis["faces_in"] == mesh["faces"].shape[0]
    again = M.cull_to_views(g, K, P, size, mode="all")
    assert torch.equal(again["faces"], g["faces"]) and torch.equal(again["vertices"], g["vertices"]) and torch.equal(again["colors"], g["colors"])
    anyv = M.cull_to_views(mesh, K, P, size, mode="any")
    assert vis["faces_kept"] <= anyv["visibility"]["faces_kept"] <= vis["faces_in"]
    # the restatement on a slice of the vertices (the whole mesh against every vertex is too slow for numpy)
    v, f = _np(mesh["vertices"]), _np(mesh["faces"])
    idx = np.arange(0, len(v), max(len(v) // 24, 1))
    want = V.point_visibility(v[idx], v, f, V.make_views(K, P, size))
    assert np.array_equal(_np(g["vertex_views"])[idx], want["count"])


def test_evaluate_meshes_culls_both_meshes_to_the_views():
    """The plane of tests/test_mesh_distance_gpu.py tessellated twice, seen whole by one camera; the ground truth alone has an extra
    patch BEHIND the camera.  Without culling its samples lie 6 units from the prediction; culled, the two are one plane again."""
    from spann3r_amd import evaluate as E
    (va, fa), (vb, fb) = _plane(False), _plane(True)
    n = len(vb)
    patch_v = np.array([(0, 0, -6), (2, 0, -6), (2, 1, -6), (0, 1, -6)], np.float32)
    patch_f = np.array([(n, n + 1, n + 2), (n, n + 2, n + 3)], np.int32)
    a, b = _mesh(va, fa), _mesh(np.concatenate([vb, patch_v]), np.concatenate([fb, patch_f]))
    P = np.eye(4)
    P[:3, 3] = (1.0, 0.5, -3.0)                                                     # above the plane's centre, looking down +z at it
    views = dict(intrinsics=np.array([[40.0, 0, 31.5], [0, 40.0, 15.5], [0, 0, 1]]), cam2world=P, size=(32, 64))
    plain = E.evaluate_meshes(a, b, n_samples=65536, icp=False, exact=True)
    assert plain["comp"] > 1e-3 and plain["acc"] < 1e-12
    for accel in ("grid", "bvh"):
        r = E.evaluate_meshes(a, b, n_samples=65536, icp=False, exact=True, accel=accel, cull_views=views)
        print("culled (%s): acc %.3e comp %.3e, faces kept %d and %d" % (accel, r["acc"], r["comp"], r["pred_faces_kept"], r["gt_faces_kept"]))
        assert r["acc"] < 1e-12 and r["comp"] < 1e-12 and r["comp_med"] < 1e-12
        assert r["pred_faces_kept"] == len(fa) and r["gt_faces_kept"] == len(fb) and r["gt_area"] == r["pred_area"] == 2.0
        assert sorted(r) == sorted(list(plain) + ["pred_faces_kept", "gt_faces_kept"])
    # cull_views=None: the dict it was
    none = E.evaluate_meshes(a, b, n_samples=65536, icp=False, exact=True, cull_views=None)
    assert sorted(none) == sorted(plain) and all(np.array_equal(none[k], plain[k]) for k in plain)
    sampled = E.evaluate_meshes(a, b, n_samples=4096, icp=False, cull_views=views)
    assert sampled["gt_faces_kept"] == len(fb) and "exact" not in sampled


def test_demo_loop_rejects_eval_cull_without_eval_samples(monkeypatch, capsys):
    import demo_loop
    for extra in ([], ["--fused"], ["--fused", "--eval"]):
        monkeypatch.setattr(sys, "argv", ["demo_loop.py", "--tiny", "--eval_cull"] + extra)
        with pytest.raises(SystemExit) as e:
            demo_loop.main()
        assert e.value.code == 2 and "--eval_cull needs --eval_samples" in capsys.readouterr().err
