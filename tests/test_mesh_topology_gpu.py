"""sp3_mesh_edge_keys / sp3_mesh_edge_table / sp3_mesh_adjacency_* / sp3_mesh_smooth_pass on the device (csrc/mesh_topology.hip;
include/spann3r_hip.h "Mesh topology and smoothing") and what drives them: mesh.MeshTopology, mesh.topology, mesh.smooth and the
smooth_iters argument of the fusion extractors.

The anchor is tests/mesh_topology_ref.py (the numpy restatement, checked in tests/test_mesh_topology_cpu.py).  Every comparison with
it is exact: integer arrays equal in dtype and value, positions bit for bit.  The inputs are the smallest that reach each failure
mode: every edge class with unusable faces mixed in, runs of one edge longer than two 256-element tiles that start at several
offsets within a tile, a row of 10 000 neighbours under one lane, and a sheet of more than 1024 scan tiles."""
import sys

import numpy as np
import pytest
import torch

import bricks_ref as BR
import fusion_ref as FR
import mesh_ray_ref as RR
import mesh_topology_ref as T
import raycast_ref as RC

pytestmark = pytest.mark.gpu

S = BR.SCENE
DTYPES = dict(edges=torch.int32, edge_first=torch.int32, half_edges=torch.int32, edge_uses=torch.int32, edge_fwd=torch.int32,
              edge_class=torch.uint8, vertex_offsets=torch.int32, vertex_neighbors=torch.int32, vertex_boundary=torch.uint8)


def _t(x):
    return torch.from_numpy(np.array(x)).cuda()


def _mesh(verts, faces):
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    colors = (np.arange(4 * len(verts), dtype=np.uint32) * np.uint32(40503) >> 3).astype(np.uint8).reshape(-1, 4)
    return dict(vertices=_t(verts), colors=_t(colors), faces=_t(np.asarray(faces, np.int32).reshape(-1, 3)),
                bounds=np.zeros((2, 3), np.float32), label="kept")


def _positions(nv, seed=1):
    return np.random.default_rng(seed).standard_normal((nv, 3)).astype(np.float32)


def _tables(topo):
    for k, dt in DTYPES.items():
        x = getattr(topo, k)
        assert x.dtype == dt and x.is_cuda and x.is_contiguous(), k
    return {k: getattr(topo, k).cpu().numpy() for k in DTYPES}


def _assert_topology(topo, ref):
    got = _tables(topo)
    for k in T.TABLES:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    assert tuple(topo.report) == T.REPORT_KEYS and topo.report == ref["report"]
    assert all(type(v) is (bool if k == "closed" else int) for k, v in topo.report.items())
    assert topo.n_edges == ref["report"]["edges"] and topo.boundary_vertices == int(ref["vertex_boundary"].sum())
    return got


def _topology(faces, nv):
    from spann3r_amd import mesh as M
    return M.topology(_mesh(_positions(nv), faces))


def _bits(x):
    return (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x, np.float32)).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. every class, small
@pytest.mark.parametrize("name", sorted(T.SMALL))
def test_small_cases_equal_the_restatement(name):
    nv, faces = T.SMALL[name]
    ref = T.topology(faces, nv)
    _assert_topology(_topology(faces, nv), ref)
    mixed, _ = T.with_unusable(faces)
    refm = T.topology(mixed, nv)
    assert refm["report"] == dict(ref["report"], faces_unusable=len(T.UNUSABLE) + 2 * len(faces))
    got = _assert_topology(_topology(mixed, nv), refm)
    for k in T.TABLES:
        if k != "half_edges":
            assert np.array_equal(got[k], ref[k]), k


def test_the_classes_are_what_the_rule_says():
    r = {name: _topology(f, nv).report for name, (nv, f) in T.SMALL.items()}
    assert (r["triangle"]["boundary"], r["triangle"]["edges"], r["triangle"]["closed"]) == (3, 3, False)
    assert (r["tetrahedron"]["edges"], r["tetrahedron"]["interior"], r["tetrahedron"]["euler"], r["tetrahedron"]["closed"]) == (6, 6, 2, True)
    assert (r["pair_consistent"]["interior"], r["pair_consistent"]["inconsistent"]) == (1, 0)
    assert (r["pair_inconsistent"]["interior"], r["pair_inconsistent"]["inconsistent"]) == (0, 1)
    assert (r["duplicate"]["inconsistent"], r["duplicate"]["edges"]) == (3, 3)
    assert (r["three_on_an_edge"]["nonmanifold"], r["three_on_an_edge"]["boundary"]) == (1, 6)


# ------------------------------------------------------------------------------------------------ 2. runs across tile borders
@pytest.mark.parametrize("reverse_every", [0, 2])
@pytest.mark.parametrize("shift", [0, 1, 85, 170, 255, 300])
def test_a_run_longer_than_two_tiles_starting_anywhere_in_a_tile(reverse_every, shift):
    """the book of 600 pages (0, 1, k) behind `shift` separate triangles below it in key order: the edges of those triangles sort first,
    three keys each, so the run of edge (0, 1) starts at offset 3 * shift % 256 of a tile and crosses two or three tile borders"""
    nv = 3 * shift + 602
    lead = np.arange(3 * shift).reshape(-1, 3)
    pages = T.book(600, reverse_every=reverse_every) + 3 * shift
    faces = np.concatenate([lead, pages]).astype(np.int32)
    ref = T.topology(faces, nv)
    e = 3 * shift                                                                # the edge (3 shift, 3 shift + 1)
    assert ref["edges"][e].tolist() == [3 * shift, 3 * shift + 1] and ref["edge_first"][e] == 3 * shift and ref["edge_uses"][e] == 600
    assert ref["edge_fwd"][e] == (300 if reverse_every else 600) and ref["edge_class"][e] == 3
    _assert_topology(_topology(faces, nv), ref)


# ------------------------------------------------------------------------------------------------ 3. one long row
def test_a_row_of_ten_thousand_neighbours_is_summed_in_order():
    from spann3r_amd import mesh as M
    verts, faces = T.closed_fan(10000)
    m = _mesh(verts, faces)
    topo = M.topology(m)
    ref = T.topology(faces, len(verts))
    got = _assert_topology(topo, ref)
    row = got["vertex_neighbors"][got["vertex_offsets"][0]:got["vertex_offsets"][1]]
    assert np.array_equal(row, np.arange(1, 10001)) and topo.report["boundary"] == 10000
    for c in (0.5, -0.53):
        out = topo.smooth_pass(m["vertices"], c)
        assert np.array_equal(_bits(out), _bits(T.smooth_pass(verts, ref["vertex_offsets"], ref["vertex_neighbors"], c)))
    assert np.array_equal(_bits(m["vertices"]), _bits(verts))                      # (the input is only read)


# ------------------------------------------------------------------------------------------------ 4. more than 1024 scan tiles
def test_the_sheet_needs_more_than_one_count_per_scan_thread():
    verts, faces = T.grid_sheet(600, 0.01)
    assert len(faces) == 717602 and (3 * len(faces) + 255) // 256 > 1024
    topo = _topology(faces, len(verts))
    r = topo.report
    assert (r["edges"], r["boundary"], r["euler"], r["inconsistent"], r["nonmanifold"]) == (1077601, 2396, 1, 0, 0)
    assert r["faces_usable"] == 717602 and r["vertices_referenced"] == 360000 and not r["closed"]
    _assert_topology(topo, T.topology(faces, len(verts)))


# ------------------------------------------------------------------------------------------------ 5. permuted faces
def test_a_permuted_face_list_gives_the_same_tables_and_the_same_smoothing():
    from spann3r_amd import mesh as M
    verts, faces = RR.icosphere(3)
    rng = np.random.default_rng(2)
    noisy = (verts * (1 + 0.02 * rng.uniform(-1, 1, (len(verts), 1)))).astype(np.float32)
    perm = rng.permutation(len(faces))
    a, b = M.topology(_mesh(noisy, faces)), M.topology(_mesh(noisy, faces[perm]))
    ta, tb = _assert_topology(a, T.topology(faces, len(verts))), _assert_topology(b, T.topology(faces[perm], len(verts)))
    for k in ("edges", "edge_first", "edge_uses", "edge_class", "vertex_offsets", "vertex_neighbors", "vertex_boundary"):
        assert np.array_equal(ta[k], tb[k]), k
    assert a.report == b.report and a.report["closed"] and a.report["euler"] == 2 and a.report["edges"] == 1920
    # face perm[i] of the first list is face i of the second: the half-edge lists are the permutation's image
    inverse = np.argsort(perm)
    image = 3 * inverse[ta["half_edges"] // 3] + ta["half_edges"] % 3
    for e in range(0, 1920, 7):
        s, t = ta["edge_first"][e], ta["edge_first"][e + 1]
        assert sorted(image[s:t]) == tb["half_edges"][s:t].tolist()
    sa, sb = M.smooth(_mesh(noisy, faces), 10), M.smooth(_mesh(noisy, faces[perm]), 10)
    assert torch.equal(sa["vertices"].view(torch.int32), sb["vertices"].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 6. smoothing against the restatement
@pytest.fixture(scope="module")
def noisy_sheet():
    verts, faces = T.grid_sheet(17, 1.0 / 16)
    verts[:, 2] = np.random.default_rng(13).uniform(-0.02, 0.02, len(verts)).astype(np.float32)
    return verts, faces


def _assert_smooth(m, verts, faces, **kw):
    from spann3r_amd import mesh as M
    kw_ref = dict(kw)
    n = kw_ref.pop("iterations", 10)
    out = M.smooth(m, **kw)
    ref = T.smooth(verts, faces, n, **kw_ref)
    assert out["vertices"].dtype == torch.float32 and out["vertices"].data_ptr() != m["vertices"].data_ptr()
    assert np.array_equal(_bits(out["vertices"]), _bits(ref))
    assert np.array_equal(_bits(m["vertices"]), _bits(verts))                      # the caller's positions are not written
    assert sorted(out) == sorted(list(m) + ["smooth"]) and out["label"] == "kept"
    assert out["faces"] is m["faces"] and out["colors"] is m["colors"]
    assert out["bounds"].dtype == np.float32 and np.array_equal(out["bounds"], np.stack([ref.min(0), ref.max(0)]))
    fixed = int(T.topology(faces, len(verts))["vertex_boundary"].sum()) if kw.get("boundary", "fixed") == "fixed" else 0
    assert out["smooth"] == dict(iterations=n, lam=kw.get("lam", 0.5), mu=kw.get("mu", -0.53), boundary=kw.get("boundary", "fixed"),
                                 fixed_vertices=fixed)
    return out


def test_smooth_equals_the_restatement(noisy_sheet):
    verts, faces = RR.icosphere(3)
    noisy = (verts * (1 + 0.02 * np.random.default_rng(11).uniform(-1, 1, (len(verts), 1)))).astype(np.float32)
    out = _assert_smooth(_mesh(noisy, faces), noisy, faces)
    r0, r = np.linalg.norm(noisy.astype(np.float64), axis=1), np.linalg.norm(out["vertices"].cpu().numpy().astype(np.float64), axis=1)
    assert r.std() <= 0.5 * r0.std() and abs(r.mean() - 1) <= 0.01                 # (what the filter is for, on the device's own output)
    _assert_smooth(_mesh(noisy, faces), noisy, faces, iterations=3, lam=0.3, mu=-0.34)
    sv, sf = noisy_sheet
    fixed = _assert_smooth(_mesh(sv, sf), sv, sf, boundary="fixed")
    assert fixed["smooth"]["fixed_vertices"] == 64
    rim = T.topology(sf, len(sv))["vertex_boundary"] == 1
    assert np.array_equal(_bits(fixed["vertices"])[rim], _bits(sv)[rim])
    free = _assert_smooth(_mesh(sv, sf), sv, sf, boundary="free")
    assert float(free["vertices"][:, 0].min()) > 0.005
    _assert_smooth(_mesh(sv, sf), sv, sf, iterations=4, mu=0)
    _assert_smooth(_mesh(sv, sf), sv, sf, iterations=4, mu=0.0, boundary="free")
    same = _assert_smooth(_mesh(sv, sf), sv, sf, iterations=0)
    assert np.array_equal(_bits(same["vertices"]), _bits(sv))


def test_a_nan_spreads_one_ring_per_pass_and_nowhere_else():
    from spann3r_amd import mesh as M
    verts, faces = T.grid_sheet(17, 1.0 / 16)
    verts[8 * 17 + 8] = (np.nan, 0.5, np.inf)
    out = M.smooth(_mesh(verts, faces), 3, boundary="free")["vertices"].cpu().numpy()
    ref = T.smooth(verts, faces, 3, boundary="free")
    assert np.array_equal(np.isnan(out), np.isnan(ref)) and 0 < np.isnan(ref).any(1).sum() < len(verts)
    ok = ~np.isnan(ref)
    assert np.array_equal(out.view(np.uint32)[ok], ref.view(np.uint32)[ok])


def test_vertices_without_a_usable_face_do_not_move():
    from spann3r_amd import mesh as M
    nv, tet = T.SMALL["tetrahedron"]
    faces = np.concatenate([tet, [(4, 4, 5), (6, 7, 99), (5, 6, 5)]]).astype(np.int32)      # 4..7: named by unusable faces only; 8, 9: by none
    verts = _positions(10, seed=4)
    verts[9] = (np.nan, -0.0, np.inf)
    out = M.smooth(_mesh(verts, faces), 5, boundary="free")
    assert np.array_equal(_bits(out["vertices"])[4:], _bits(verts)[4:]) and not np.array_equal(_bits(out["vertices"])[:4], _bits(verts)[:4])
    assert np.array_equal(_bits(out["vertices"]), _bits(T.smooth(verts, faces, 5, boundary="free")))
    topo = M.topology(_mesh(verts, faces))
    assert topo.report["faces_unusable"] == 3 and topo.report["vertices_referenced"] == 4 and topo.report["closed"]


def test_a_topology_is_reusable_and_a_foreign_one_is_refused(noisy_sheet):
    from spann3r_amd import mesh as M
    sv, sf = noisy_sheet
    m = _mesh(sv, sf)
    topo = M.topology(m)
    fresh = M.smooth(m, 5)
    again = M.smooth(m, 5, topology=topo)
    moved = M.smooth(dict(again, faces=m["faces"].clone()), 5, topology=topo)       # other positions, an equal face list elsewhere
    assert torch.equal(fresh["vertices"].view(torch.int32), again["vertices"].view(torch.int32))
    assert np.array_equal(_bits(moved["vertices"]), _bits(T.smooth(sv, sf, 10)))
    with pytest.raises(ValueError, match="another mesh"):
        M.smooth(_mesh(sv, sf[:-1]), 5, topology=topo)                              # another F
    with pytest.raises(ValueError, match="another mesh"):
        M.smooth(_mesh(np.concatenate([sv, sv[:1]]), sf), 5, topology=topo)         # another V
    with pytest.raises(ValueError, match="another mesh"):
        M.smooth(_mesh(sv, sf[::-1]), 5, topology=topo)                             # the same sizes, other faces
    with pytest.raises(TypeError):
        M.smooth(m, 5, topology=dict(vertex_offsets=None))


# ------------------------------------------------------------------------------------------------ 7. empty sizes, argument errors
def test_empty_sizes_launch_nothing_and_report_an_open_nothing():
    from spann3r_amd import mesh as M
    none = np.zeros((0, 3), np.int32)
    for nv, faces in ((5, none), (0, none), (0, np.array([[0, 1, 2]], np.int32)), (4, np.array([[0, 0, 1], [1, 2, 7]], np.int32))):
        verts = _positions(nv)
        topo = M.topology(_mesh(verts, faces))
        _assert_topology(topo, T.topology(faces, nv))
        assert topo.report["edges"] == 0 and not topo.report["closed"] and topo.report["faces_unusable"] == len(faces)
        assert topo.vertex_offsets.shape == (nv + 1,) and not bool(topo.vertex_offsets.any()) and topo.edge_first.tolist() == [0]
        out = M.smooth(_mesh(verts, faces), 3)
        assert np.array_equal(_bits(out["vertices"]), _bits(verts)) and out["smooth"]["fixed_vertices"] == 0
    cloud = dict(_mesh(_positions(4), none), faces=None)
    for fn in (M.topology, M.MeshTopology, M.smooth):
        with pytest.raises(ValueError, match="point cloud"):
            fn(cloud)


def test_arguments_are_checked_before_anything_is_launched(noisy_sheet):
    from spann3r_amd import lib as L, mesh as M
    sv, sf = noisy_sheet
    m = _mesh(sv, sf)
    for bad in (dict(m, faces=m["faces"].long()), dict(m, faces=m["faces"].reshape(-1)), dict(m, faces=m["faces"][:, :2]),
                dict(m, vertices=m["vertices"][:, :2])):
        for fn in (M.topology, M.smooth):
            with pytest.raises(RuntimeError):
                fn(bad)
    with pytest.raises(RuntimeError, match="CUDA|GPU"):
        M.topology(dict(m, faces=m["faces"].cpu()))
    with pytest.raises(ValueError, match="boundary"):
        M.smooth(m, boundary="pinned")
    with pytest.raises(ValueError, match="iterations"):
        M.smooth(m, iterations=-1)
    # the entry points refuse what the wrappers never pass
    lib = L.load()
    p = m["vertices"]
    topo = M.topology(m)
    assert lib.sp3_mesh_smooth_pass(p.data_ptr(), len(sv), topo.vertex_offsets.data_ptr(), topo.vertex_neighbors.data_ptr(), 0, 0.5, p.data_ptr(),
                                    L.stream_ptr()) == 1 and b"never reads what it writes" in lib.sp3_last_error()
    keys = torch.empty(3, dtype=torch.int64, device="cuda")
    info = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert lib.sp3_mesh_edge_keys(m["faces"].data_ptr(), 2 ** 31 // 3 + 1, 5, keys.data_ptr(), info.data_ptr(), L.stream_ptr()) == 1
    assert lib.sp3_mesh_edge_keys(m["faces"].data_ptr(), 1, 2 ** 31 - 1, keys.data_ptr(), info.data_ptr(), L.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert not bool(info.any())


# ------------------------------------------------------------------------------------------------ 8. the brick scene, both routes
@pytest.fixture(scope="module")
def brick():
    from spann3r_amd import fusion as F_
    frs = RC.scene_frames()
    vol = F_.BrickTSDFVolume(S["origin"], S["voxel"], S["dims"], trunc=S["trunc"], band=S["band"])
    vol.integrate(intrinsics=[f["K"] for f in frs], cam2world=[f["cam2world"] for f in frs], valid=[_t(f["valid"]) for f in frs],
                  pts=[_t(f["pts"]) for f in frs], images=[_t(f["images"]) for f in frs])
    return vol, vol.extract_mesh(direct=True), vol.extract_mesh()


def _assert_same_mesh(a, b):
    for k in ("vertices", "colors", "faces"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    assert np.array_equal(_bits(a["vertices"]), _bits(b["vertices"])) and np.array_equal(a["bounds"], b["bounds"])


@pytest.mark.parametrize("direct", [True, False])
def test_the_brick_scene_report_and_smooth_iters(brick, direct):
    from spann3r_amd import mesh as M
    vol, raw_direct, raw_dense = brick
    raw = raw_direct if direct else raw_dense
    topo = M.topology(raw)
    ref = FR.manifold_report(raw["faces"].cpu().numpy())
    r = topo.report
    assert r["inconsistent"] + r["nonmanifold"] == 0 and r["boundary"] == len(ref["boundary"]) > 0
    assert r["faces_usable"] + r["faces_unusable"] == raw["faces"].shape[0]
    _assert_topology(topo, T.topology(raw["faces"].cpu().numpy(), raw["vertices"].shape[0]))
    got = vol.extract_mesh(direct=direct, smooth_iters=5)
    want = M.smooth(raw, 5)
    assert sorted(got) == ["bounds", "colors", "faces", "smooth", "vertices"] and got["smooth"] == want["smooth"]
    assert got["smooth"]["iterations"] == 5 and got["smooth"]["fixed_vertices"] == topo.boundary_vertices > 0
    _assert_same_mesh(got, want)
    assert np.array_equal(_bits(got["vertices"]), _bits(T.smooth(raw["vertices"].cpu().numpy(), raw["faces"].cpu().numpy(), 5)))
    assert not torch.equal(got["vertices"], raw["vertices"])
    normals = M.vertex_normals(got)
    assert normals.shape == got["vertices"].shape and bool(torch.isfinite(normals).all()) and bool((normals.norm(dim=1) > 0.99).any())
    # the filter first, then the smoothing, then the clustering
    cell = 2 * S["voxel"]
    origin = vol.origin if direct else vol.to_dense().origin
    all3 = vol.extract_mesh(direct=direct, min_component_faces=9, simplify_cell=cell, smooth_iters=5)
    step = M.simplify(M.smooth(M.filter_components(raw, min_faces=9), 5), cell, origin=origin)
    assert all3["components"] == step["components"] and all3["simplify"] == step["simplify"] and all3["smooth"] == step["smooth"]
    _assert_same_mesh(all3, step)


def test_the_defaults_run_nothing_new_and_scale_follows_the_smoothing(brick):
    from spann3r_amd import fusion as F_
    vol, raw_direct, raw_dense = brick
    for direct, raw in ((True, raw_direct), (False, raw_dense)):
        got = vol.extract_mesh(direct=direct, smooth_iters=0)
        assert sorted(got) == sorted(raw) == ["bounds", "colors", "faces", "vertices"]
        _assert_same_mesh(got, raw)
    with pytest.raises(ValueError, match="smooth_iters"):
        vol.extract_mesh(direct=True, smooth_iters=-1)
    plain = vol.extract_mesh(direct=True, smooth_iters=3)
    scaled = vol.extract_mesh(direct=True, smooth_iters=3, scale=10.0, transform=np.diag([-1.0, -1.0, 1.0, 1.0]))
    assert torch.equal(scaled["faces"], plain["faces"]) and torch.equal(scaled["colors"], plain["colors"])
    assert torch.equal(scaled["vertices"], plain["vertices"] * 10.0 * torch.tensor([-1.0, -1.0, 1.0], device="cuda"))
    assert np.array_equal(scaled["bounds"], np.stack([scaled["vertices"].amin(0).cpu().numpy(), scaled["vertices"].amax(0).cpu().numpy()]))
    # the drivers pass the argument through
    frs = RC.scene_frames()
    args = (torch.stack([_t(f["pts"]) for f in frs]), np.stack([f["K"] for f in frs]), np.stack([f["cam2world"] for f in frs]),
            torch.stack([_t(f["valid"]) for f in frs]).bool(), torch.stack([_t(f["images"]) for f in frs]))
    from spann3r_amd import mesh as M
    a = F_.fuse_pointmaps(*args, voxel_size=S["voxel"], bricks=True, direct_mesh=True, smooth_iters=3)
    assert a["smooth"]["iterations"] == 3
    _assert_same_mesh(a, M.smooth(F_.fuse_pointmaps(*args, voxel_size=S["voxel"], bricks=True, direct_mesh=True), 3))
    d = F_.fuse_pointmaps(*args, voxel_size=S["voxel"], smooth_iters=2)
    _assert_same_mesh(d, M.smooth(F_.fuse_pointmaps(*args, voxel_size=S["voxel"]), 2))


def test_two_spheres_stay_closed_under_smoothing():
    from spann3r_amd import fusion as F_, mesh as M
    dims, trunc = (48, 32, 32), 3.0
    big, small = FR.sphere_volume(dims, (0, 0, 0), 1.0, (14.3, 16.2, 15.9), 10.0, trunc), FR.sphere_volume(dims, (0, 0, 0), 1.0, (38.3, 16.2, 15.9), 3.0, trunc)
    vol = F_.TSDFVolume((0, 0, 0), 1.0, dims, trunc=trunc, color=False)
    vol.tsdf.copy_(_t(np.minimum(big[0], small[0])))
    vol.weight.copy_(_t(big[1]))
    both = vol.extract_mesh()
    before = M.topology(both).report
    assert before["closed"] and before["euler"] == 4 and before["boundary"] == 0
    smoothed = vol.extract_mesh(smooth_iters=10)
    assert smoothed["smooth"]["fixed_vertices"] == 0 and torch.equal(smoothed["faces"], both["faces"])
    assert M.topology(smoothed).report == before
    assert bool(torch.isfinite(smoothed["vertices"]).all()) and not torch.equal(smoothed["vertices"], both["vertices"])


# ------------------------------------------------------------------------------------------------ 9. the demo's arguments
@pytest.mark.parametrize("flag", [["--smooth", "5"], ["--mesh_report"]])
def test_demo_loop_rejects_the_flags_without_fused(monkeypatch, capsys, flag):
    import demo_loop
    monkeypatch.setattr(sys, "argv", ["demo_loop.py", "--tiny"] + flag)
    with pytest.raises(SystemExit) as e:
        demo_loop.main()
    assert e.value.code == 2 and "--fused" in capsys.readouterr().err
