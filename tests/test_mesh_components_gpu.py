"""sp3_mesh_components / sp3_mesh_select_faces on the device (csrc/mesh_components.hip; include/spann3r_hip.h "Mesh components")
and what drives them: mesh.components, mesh.filter_components and the min_component_faces / keep_largest arguments of the fusion
extractors.

The anchor is tests/mesh_components_ref.py (the numpy restatement, checked against scipy in tests/test_mesh_components_cpu.py).
Every comparison with it is exact equality of integer arrays, or bit equality of vertex rows.  The graphs are the smallest that
reach each failure mode: deep chains in three face orders (the strips), maximal contention on one root that must end at the minimum
(the star), many components of mixed size with unreferenced vertices and ties (the random graph), more than 1024 scan tiles (the
sheet), touching fans, duplicated, degenerate and invalid faces (the fans).

The brick scene: bricks_ref.SCENE's own surface has 37 components, 23 of them with fewer than 9 faces, so
`filter_components(min_faces=9)` cannot give back the rows of the raw scene mesh with an octahedron appended; it gives back the rows of
the scene mesh without its own specks.  The test states both: against the restatement on the raw mesh, and -- literally -- that a
mesh whose components all have 9 faces or more comes back exactly when the octahedron of 8 faces is appended and filtered away."""
import sys

import numpy as np
import pytest
import torch

import bricks_ref as BR
import fusion_ref as FR
import mesh_components_ref as MC
import raycast_ref as RC
from test_brick_mesh_cpu import face_rows

pytestmark = pytest.mark.gpu

S = BR.SCENE
ARRAYS = ("vertex_component", "face_component", "component_faces", "component_vertices")


def _t(x):
    return torch.from_numpy(np.array(x)).cuda()                                   # (a copy: the shared graphs are read-only)


def _components(faces, nv):
    from spann3r_amd import mesh as M
    r = M.components(_t(faces).reshape(-1, 3), nv)
    for k in ARRAYS:
        assert r[k].dtype == torch.int32 and r[k].is_cuda, k
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def _assert_equal(got, ref):
    assert (got["n_components"], got["invalid_faces"]) == (ref["n_components"], ref["invalid_faces"])
    for k in ARRAYS:
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k


def _mesh(nv, faces, seed=9):
    """a mesh dict over random positions and colours, and the same on the host"""
    rng = np.random.default_rng(seed)
    verts, rgba = rng.standard_normal((nv, 3)).astype(np.float32), rng.integers(0, 2 ** 32, nv, dtype=np.uint32)
    m = dict(vertices=_t(verts), colors=_t(rgba.view(np.uint8).reshape(-1, 4)), faces=_t(faces),
             bounds=np.stack([verts.min(0), verts.max(0)]))
    return m, verts, rgba


def _assert_mesh_equals(m, v, c, f):
    """a mesh dict against host rows: faces exactly, vertex rows bit for bit, bounds recomputed"""
    gv, gc, gf = m["vertices"].cpu().numpy(), m["colors"].cpu().numpy().view(np.uint32).ravel(), m["faces"].cpu().numpy()
    assert m["faces"].dtype == torch.int32 and m["colors"].dtype == torch.uint8 and m["colors"].shape == (len(v), 4)
    assert gf.shape == f.shape and np.array_equal(gf, f)
    assert gv.shape == v.shape and np.array_equal(gv.view(np.uint32), np.ascontiguousarray(v, np.float32).view(np.uint32))
    assert np.array_equal(gc, np.asarray(c, np.uint32))
    if len(v):
        assert np.array_equal(m["bounds"], np.stack([v.min(0), v.max(0)]))
    else:
        assert np.isinf(m["bounds"]).all()


def _host(m):
    return m["vertices"].cpu().numpy(), m["colors"].cpu().numpy().view(np.uint32).ravel(), m["faces"].cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the graphs
@pytest.mark.parametrize("name", MC.GRAPHS)
def test_components_equal_the_restatement(name):
    faces, nv, ref = MC.graph(name)
    got = _components(faces, nv)
    _assert_equal(got, ref)
    _assert_equal(_components(faces, nv), ref)                                     # the same bits every run


def test_strip_orders_and_the_star_end_at_the_minimum():
    asc = _components(*MC.graph("strip_ascending")[:2])
    for name in ("strip_descending", "strip_shuffled"):
        assert np.array_equal(_components(*MC.graph(name)[:2])["vertex_component"], asc["vertex_component"])
    assert (asc["vertex_component"] == 0).all() and asc["component_faces"].tolist() == [4094] and asc["component_vertices"].tolist() == [4096]
    faces, nv, _ = MC.graph("star")
    star = _components(faces, nv)
    assert (faces[:, 2] == nv - 1).all() and (star["vertex_component"] == 0).all() and (star["face_component"] == 0).all()
    assert star["component_faces"].tolist() == [10000] and star["component_vertices"].tolist() == [nv]


def test_a_permuted_face_list_gives_the_same_vertex_labels():
    faces, nv, ref = MC.graph("random")
    for seed in (5, 6):
        p = np.random.default_rng(seed).permutation(len(faces))
        got = _components(faces[p], nv)
        assert np.array_equal(got["vertex_component"], ref["vertex_component"])
        assert np.array_equal(got["face_component"], ref["face_component"][p])
        assert np.array_equal(got["component_faces"], ref["component_faces"])


def test_the_sheet_needs_more_than_one_count_per_scan_thread():
    faces, nv, ref = MC.graph("sheet")
    assert (nv + 255) // 256 > 1024 and ref["n_components"] == 12
    got = _components(faces, nv)
    assert got["component_vertices"].tolist() == [50 * 450] * 12 and got["component_faces"].tolist() == [2 * 49 * 449] * 12
    assert (got["vertex_component"].reshape(450, 600) == (np.arange(600) // 50)[None]).all()


def test_invalid_faces_are_counted_and_otherwise_absent():
    faces, nv, ref = MC.graph("fans")
    got = _components(faces, nv)
    _assert_equal(got, ref)
    assert got["invalid_faces"] == 4 and got["face_component"][8:12].tolist() == [-1] * 4
    clean = _components(faces[ref["face_component"] >= 0], nv)                     # everything else as if they were absent
    for k in ("vertex_component", "component_faces", "component_vertices"):
        assert np.array_equal(clean[k], got[k]), k
    assert np.array_equal(clean["face_component"], got["face_component"][got["face_component"] >= 0])


# ------------------------------------------------------------------------------------------------ 2. edge sizes, capacity, limits
def test_edge_sizes():
    from spann3r_amd import lib as L
    for faces, nv in ((np.zeros((0, 3), np.int32), 7), (np.array([[0, 1, 2], [3, 4, 5]], np.int32), 0), (np.array([[2, 0, 1]], np.int32), 3),
                      (np.zeros((0, 3), np.int32), 0)):
        _assert_equal(_components(faces, nv), MC.components(faces, nv))
    # the C entry point itself on the empty sizes: info is written, nothing else is touched
    lib = L.load()
    info = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    L.check(lib.sp3_mesh_components(None, 0, 0, None, 0, None, None, None, None, info.data_ptr(), L.stream_ptr()), "sp3_mesh_components")
    assert info.cpu().tolist() == [0, 0]
    fc = torch.full((5,), 9, dtype=torch.int32, device="cuda")
    f = _t(np.array([[0, 1, 2], [3, 4, 5], [0, 0, 0]], np.int32))
    L.check(lib.sp3_mesh_components(f.data_ptr(), 3, 0, None, 0, None, fc.data_ptr(), None, None, info.data_ptr(), L.stream_ptr()), "sp3_mesh_components")
    assert info.cpu().tolist() == [0, 3] and fc.cpu().tolist() == [-1, -1, -1, 9, 9]
    count = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    L.check(lib.sp3_mesh_select_faces(None, None, 0, None, 0, None, None, count.data_ptr(), L.stream_ptr()), "sp3_mesh_select_faces")
    assert count.cpu().tolist() == [0]
    assert lib.sp3_mesh_components_ws_bytes(0) == 0 and lib.sp3_mesh_select_faces_ws_bytes(0) == 0
    assert lib.sp3_mesh_components_ws_bytes(1000) >= 4 * 4 * 1000 and lib.sp3_mesh_select_faces_ws_bytes(1000) >= 4 * 5


def test_limits_are_checked_before_anything_is_launched():
    from spann3r_amd import lib as L
    lib = L.load()
    top = 2 ** 31 - 1
    info = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert lib.sp3_mesh_components(None, 1, top, None, 0, None, None, None, None, info.data_ptr(), None) != 0
    assert b"out of range" in lib.sp3_last_error()
    assert lib.sp3_mesh_components(None, top, 5, None, 0, None, None, None, None, info.data_ptr(), None) != 0
    assert lib.sp3_mesh_components(None, 1, 5, None, 0, None, None, None, None, None, None) != 0 and b"null info" in lib.sp3_last_error()
    assert lib.sp3_mesh_select_faces(None, None, top, None, 1, None, None, info.data_ptr(), None) != 0
    assert lib.sp3_mesh_components_ws_bytes(top) == 0 and lib.sp3_mesh_select_faces_ws_bytes(top) == 0


def test_nothing_is_written_beyond_the_capacity_and_info_holds_the_need():
    from spann3r_amd import lib as L
    faces, nv, ref = MC.graph("random")
    lib, cap, room = L.load(), 100, 600
    f = _t(faces)
    vc, fc = torch.empty(nv, dtype=torch.int32, device="cuda"), torch.empty(len(faces), dtype=torch.int32, device="cuda")
    cf, cv = (torch.full((room,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    info = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.sp3_mesh_components_ws_bytes(nv)), dtype=torch.uint8, device="cuda")
    L.check(lib.sp3_mesh_components(f.data_ptr(), len(faces), nv, ws.data_ptr(), cap, vc.data_ptr(), fc.data_ptr(), cf.data_ptr(), cv.data_ptr(),
                                    info.data_ptr(), L.stream_ptr()), "sp3_mesh_components")
    assert info.cpu().tolist() == [ref["n_components"], 0] and ref["n_components"] > cap          # the need, not the capacity
    assert np.array_equal(cf[:cap].cpu().numpy(), ref["component_faces"][:cap]) and np.array_equal(cv[:cap].cpu().numpy(), ref["component_vertices"][:cap])
    assert (cf[cap:] == -7).all() and (cv[cap:] == -7).all()
    assert np.array_equal(vc.cpu().numpy(), ref["vertex_component"]) and np.array_equal(fc.cpu().numpy(), ref["face_component"])


def test_components_runs_once_more_when_its_first_guess_is_short():
    """5000 separate triangles over 15000 vertices: more components than the first capacity of max(4096, V / 16)"""
    faces = np.arange(15000, dtype=np.int32).reshape(5000, 3)[::-1].copy()
    got = _components(faces, 15000)
    assert got["n_components"] == 5000 > max(4096, 15000 // 16)
    assert got["component_faces"].tolist() == [1] * 5000 and got["component_vertices"].tolist() == [3] * 5000
    assert np.array_equal(got["vertex_component"], np.arange(15000) // 3) and np.array_equal(got["face_component"], np.arange(5000)[::-1])


# ------------------------------------------------------------------------------------------------ 3. selection
@pytest.mark.parametrize("min_faces,keep_largest", [(1, None), (2, None), (5, None), (0, 1), (0, 3), (2, 3), (5, 1)])
def test_filter_components_equals_the_restatement_row_for_row(min_faces, keep_largest):
    from spann3r_amd import mesh as M
    faces, nv, ref = MC.graph("random")
    m, verts, rgba = _mesh(nv, faces)
    out = M.filter_components(m, min_faces, keep_largest)
    v, c, f, stats = MC.filter_mesh(verts, rgba, faces, min_faces, keep_largest)
    assert out["components"] == stats and sorted(out) == ["bounds", "colors", "components", "faces", "vertices"]
    _assert_mesh_equals(out, v, c, f)
    assert torch.equal(m["faces"], _t(faces))                                      # the input mesh stays as it was
    if keep_largest == 1 and min_faces == 0:                                       # two components of 44 faces: the lower id is kept
        big = np.flatnonzero(ref["component_faces"] == 44)
        assert len(big) == 2 and len(f) == 44 and (ref["face_component"] == big[0]).sum() == 44
        assert np.array_equal(face_rows(v, c, f.astype(np.int64)), face_rows(verts, rgba, faces.astype(np.int64))[ref["face_component"] == big[0]])


def test_select_faces_reports_its_count_and_keeps_the_order():
    from spann3r_amd import lib as L
    faces, nv, ref = MC.graph("fans")
    lib = L.load()
    keep = np.array([1, 0, 1], np.uint8)
    out = torch.full((len(faces) + 2, 3), -9, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(int(lib.sp3_mesh_select_faces_ws_bytes(len(faces))), 16), dtype=torch.uint8, device="cuda")
    f, fc, k = _t(faces), _t(ref["face_component"]), _t(keep)
    L.check(lib.sp3_mesh_select_faces(f.data_ptr(), fc.data_ptr(), len(faces), k.data_ptr(), 3, ws.data_ptr(), out.data_ptr(), count.data_ptr(),
                                      L.stream_ptr()), "sp3_mesh_select_faces")
    want = MC.select_faces(faces, ref["face_component"], keep)
    assert count.cpu().tolist() == [len(want)] == [8]
    assert np.array_equal(out[:8].cpu().numpy(), want) and (out[8:] == -9).all()
    # a component id at or beyond ncomponents keeps nothing of it
    L.check(lib.sp3_mesh_select_faces(f.data_ptr(), fc.data_ptr(), len(faces), k.data_ptr(), 2, ws.data_ptr(), out.data_ptr(), count.data_ptr(),
                                      L.stream_ptr()), "sp3_mesh_select_faces")
    assert count.cpu().tolist() == [7]


def test_everything_removed_is_an_empty_mesh_and_a_cloud_is_refused():
    from spann3r_amd import mesh as M
    faces, nv, ref = MC.graph("random")
    m, verts, rgba = _mesh(nv, faces)
    for kw in (dict(min_faces=10 ** 6), dict(keep_largest=0)):
        out = M.filter_components(m, **kw)
        assert out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3) and out["colors"].shape == (0, 4)
        assert out["components"] == dict(total=ref["n_components"], kept=0, faces_removed=len(faces)) and np.isinf(out["bounds"]).all()
    empty = M.filter_components(dict(m, faces=m["faces"][:0]), 3)
    assert empty["faces"].shape == (0, 3) and empty["components"] == dict(total=0, kept=0, faces_removed=0)
    with pytest.raises(ValueError, match="no faces"):
        M.filter_components(dict(m, faces=None))
    with pytest.raises(ValueError, match="keep_largest"):
        M.filter_components(m, keep_largest=-1)


# ------------------------------------------------------------------------------------------------ 4. the brick scene, end to end
def _brick_volume():
    from spann3r_amd import fusion as F_
    frs = RC.scene_frames()
    vol = F_.BrickTSDFVolume(S["origin"], S["voxel"], S["dims"], trunc=S["trunc"], band=S["band"])
    return vol.integrate(intrinsics=[f["K"] for f in frs], cam2world=[f["cam2world"] for f in frs], valid=[_t(f["valid"]) for f in frs],
                         pts=[_t(f["pts"]) for f in frs], images=[_t(f["images"]) for f in frs])


@pytest.fixture(scope="module")
def brick():
    """(the fused brick scene, its unfiltered direct mesh, its unfiltered dense-route mesh)"""
    vol = _brick_volume()
    return vol, vol.extract_mesh(direct=True), vol.extract_mesh()


def _with_octahedron(m, far=(40.0, -30.0, 25.0)):
    v, c, f = _host(m)
    of, opos = MC.octahedron(len(v))
    return dict(vertices=_t(np.concatenate([v, opos * np.float32(0.05) + np.float32(far)])),
                colors=_t(np.concatenate([c, np.full(6, 0xff00ff00, np.uint32)]).view(np.uint8).reshape(-1, 4)),
                faces=_t(np.concatenate([f, of])), bounds=m["bounds"])


def test_an_octahedron_far_outside_the_brick_scene_is_filtered_away(brick):
    from spann3r_amd import mesh as M
    _, raw, _ = brick
    v, c, f = _host(raw)
    ref = MC.components(f, len(v))
    assert len(f) == 86084 and ref["n_components"] == 37 and ref["invalid_faces"] == 0
    # the raw scene with the octahedron: the restatement's rows, which are those of the scene without its own specks
    out = M.filter_components(_with_octahedron(raw), min_faces=9)
    wv, wc, wf, wstats = MC.filter_mesh(v, c, f, min_faces=9)
    _assert_mesh_equals(out, wv, wc, wf)
    assert out["components"] == dict(total=38, kept=wstats["kept"], faces_removed=wstats["faces_removed"] + 8)
    assert out["bounds"][1, 0] < 2.0                                               # the bounds no longer reach the octahedron
    # literally: a mesh whose components all have 9 faces or more comes back exactly, rows and order
    clean = M.filter_components(raw, min_faces=9)
    _assert_mesh_equals(clean, wv, wc, wf)
    back = M.filter_components(_with_octahedron(clean), min_faces=9)
    _assert_mesh_equals(back, *_host(clean))
    assert back["components"] == dict(total=wstats["kept"] + 1, kept=wstats["kept"], faces_removed=8)
    assert np.array_equal(back["bounds"], clean["bounds"])


@pytest.mark.parametrize("direct", [True, False])
@pytest.mark.parametrize("kw", [dict(min_component_faces=9), dict(min_component_faces=100), dict(keep_largest=1), dict(min_component_faces=20, keep_largest=3)])
def test_extract_mesh_with_the_filter_equals_the_restatement_on_the_unfiltered_mesh(brick, direct, kw):
    vol, raw_direct, raw_dense = brick
    got = vol.extract_mesh(direct=direct, **kw)
    v, c, f = _host(raw_direct if direct else raw_dense)
    wv, wc, wf, stats = MC.filter_mesh(v, c, f, kw.get("min_component_faces", 0), kw.get("keep_largest"))
    assert 0 < len(wf) < len(f) and got["components"] == stats
    _assert_mesh_equals(got, wv, wc, wf)


def test_the_defaults_return_what_a_call_without_the_arguments_returns(brick):
    from spann3r_amd import fusion as F_
    vol, raw_direct, raw_dense = brick
    for direct, raw in ((True, raw_direct), (False, raw_dense)):
        got = vol.extract_mesh(direct=direct, min_component_faces=0, keep_largest=None)
        assert sorted(got) == sorted(raw) == ["bounds", "colors", "faces", "vertices"]
        for k in ("vertices", "colors", "faces"):
            assert torch.equal(got[k], raw[k]), k
        assert np.array_equal(got["bounds"], raw["bounds"])
    with pytest.raises(ValueError, match="min_component_faces"):
        vol.extract_mesh(direct=True, min_component_faces=-1)
    # the drivers pass the arguments through
    frs = RC.scene_frames()
    args = (torch.stack([_t(f["pts"]) for f in frs]), np.stack([f["K"] for f in frs]), np.stack([f["cam2world"] for f in frs]),
            torch.stack([_t(f["valid"]) for f in frs]).bool(), torch.stack([_t(f["images"]) for f in frs]))
    a = F_.fuse_pointmaps(*args, voxel_size=S["voxel"], bricks=True, direct_mesh=True, keep_largest=1)
    b = F_.fuse_pointmaps(*args, voxel_size=S["voxel"], bricks=True, direct_mesh=True)
    assert "components" not in b and a["components"]["kept"] == 1 and 0 < a["faces"].shape[0] < b["faces"].shape[0]
    _assert_mesh_equals(a, *MC.filter_mesh(*_host(b), keep_largest=1)[:3])
    d = F_.fuse_pointmaps(*args, voxel_size=S["voxel"], min_component_faces=50)
    _assert_mesh_equals(d, *MC.filter_mesh(*_host(F_.fuse_pointmaps(*args, voxel_size=S["voxel"])), min_faces=50)[:3])


# ------------------------------------------------------------------------------------------------ 5. an analytic volume
def test_two_spheres_two_components_and_the_largest_is_a_closed_manifold():
    from spann3r_amd import fusion as F_, mesh as M
    dims, trunc = (48, 32, 32), 3.0
    big, small = FR.sphere_volume(dims, (0, 0, 0), 1.0, (14.3, 16.2, 15.9), 10.0, trunc), FR.sphere_volume(dims, (0, 0, 0), 1.0, (38.3, 16.2, 15.9), 3.0, trunc)
    vol = F_.TSDFVolume((0, 0, 0), 1.0, dims, trunc=trunc, color=False)
    vol.tsdf.copy_(_t(np.minimum(big[0], small[0])))
    vol.weight.copy_(_t(big[1]))
    both = vol.extract_mesh()
    comp = M.components(both["faces"], both["vertices"].shape[0])
    cf = comp["component_faces"].cpu().tolist()
    assert comp["n_components"] == 2 and comp["invalid_faces"] == 0 and cf[0] > 5 * cf[1] > 0 and sum(cf) == both["faces"].shape[0]
    assert int((comp["vertex_component"] < 0).sum()) == 0
    one = vol.extract_mesh(keep_largest=1)
    rep = FR.manifold_report(one["faces"].cpu().numpy())
    assert one["components"] == dict(total=2, kept=1, faces_removed=cf[1]) and one["faces"].shape[0] == cf[0]
    assert rep["closed"] and rep["euler"] == 2 and one["vertices"].shape[0] == comp["component_vertices"][0].item()
    assert one["bounds"][1, 0] < 25.0 < both["bounds"][1, 0]
    other = vol.extract_mesh(min_component_faces=cf[1] + 1)
    assert torch.equal(other["faces"], one["faces"]) and torch.equal(other["vertices"], one["vertices"])


# ------------------------------------------------------------------------------------------------ 6. the demo's arguments
def test_demo_loop_rejects_the_component_flags_without_fused(monkeypatch, capsys):
    import demo_loop
    monkeypatch.setattr(sys, "argv", ["demo_loop.py", "--tiny", "--min_component", "20"])
    with pytest.raises(SystemExit) as e:
        demo_loop.main()
    assert e.value.code == 2 and "need --fused" in capsys.readouterr().err
