"""sp3_mesh_cluster / sp3_mesh_cluster_faces on the device (csrc/mesh_simplify.hip; include/spann3r_hip.h "Mesh simplification") and
what drives them: mesh.cluster_vertices, mesh.simplify and the simplify_cell argument of the fusion extractors.

The anchor is tests/mesh_simplify_ref.py (the numpy restatement, checked against a vertex-by-vertex loop in
tests/test_mesh_simplify_cpu.py).  Every comparison with it is exact: integer arrays equal, vertex rows bit for bit.  The inputs are
the smallest that reach each failure mode: a table nearly full (long probe chains, wrap-around), one cell under maximal contention
with sums beyond 32 bits, the floor of negative coordinates, unusable vertices and invalid faces, every kind of duplicate, and a
sheet of more than 1024 scan tiles."""
import sys

import numpy as np
import pytest
import torch

import bricks_ref as BR
import mesh_components_ref as MC
import mesh_simplify_ref as MS
import raycast_ref as RC

pytestmark = pytest.mark.gpu

S = BR.SCENE


def _t(x):
    return torch.from_numpy(np.array(x)).cuda()


def _mesh(verts, rgba, faces):
    verts = np.asarray(verts, np.float32)
    return dict(vertices=_t(verts), colors=_t(np.asarray(rgba, np.uint32).view(np.uint8).reshape(-1, 4)),
                faces=None if faces is None else _t(np.asarray(faces, np.int32).reshape(-1, 3)), bounds=None)


def _host(m):
    return (m["vertices"].cpu().numpy(), m["colors"].cpu().numpy().view(np.uint32).ravel(), None if m["faces"] is None else m["faces"].cpu().numpy())


def _assert_simplified(out, want, return_map=True):
    """a simplified mesh dict against the restatement's (vertices, rgba, faces, stats, vertex_cluster)"""
    v, c, f, stats, vc = want
    gv, gc, gf = _host(out)
    assert out["vertices"].dtype == torch.float32 and out["colors"].dtype == torch.uint8 and out["colors"].shape == (len(v), 4)
    assert out["simplify"] == stats
    if f is None:
        assert gf is None
    else:
        assert out["faces"].dtype == torch.int32 and gf.shape == f.shape and np.array_equal(gf, f)
    assert gv.shape == v.shape and np.array_equal(gv.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(gc, c)
    if len(v):
        assert np.array_equal(out["bounds"], np.stack([v.min(0), v.max(0)]))
    else:
        assert np.isinf(out["bounds"]).all()
    if return_map:
        assert out["vertex_cluster"].dtype == torch.int32 and np.array_equal(out["vertex_cluster"].cpu().numpy(), vc)


def _check(verts, rgba, faces, cell, origin=None, dedup=True):
    from spann3r_amd import mesh as M
    out = M.simplify(_mesh(verts, rgba, faces), cell, origin=origin, dedup=dedup, return_map=True)
    want = MS.simplify(verts, rgba, faces, cell, origin, dedup)
    _assert_simplified(out, want)
    return out, want


def _assert_clusters(got, ref):
    assert got["n_clusters"] == ref["n_clusters"]
    assert np.array_equal(got["vertex_cluster"].cpu().numpy(), ref["vertex_cluster"])
    assert np.array_equal(got["positions"].cpu().numpy().view(np.uint32), ref["positions"].view(np.uint32))
    if ref["rgba"] is None:
        assert got["rgba"] is None
    else:
        assert np.array_equal(got["rgba"].cpu().numpy().view(np.uint32), ref["rgba"])


# ------------------------------------------------------------------------------------------------ 1. a nearly full table
def _block():
    rng = np.random.default_rng(11)
    verts = (rng.random((1000, 3)) * 3).astype(np.float32)                         # a 3 x 3 x 3 block of unit cells
    return verts, rng.integers(0, 2 ** 32, 1000, dtype=np.uint32), rng.integers(0, 1000, (3000, 3)).astype(np.int32)


def test_random_block_equals_the_restatement_whatever_the_table_size():
    from spann3r_amd import lib as L, mesh as M
    verts, rgba, faces = _block()
    out, want = _check(verts, rgba, faces, 1.0)
    assert want[3]["clusters"] == 27 and 0 < len(want[2]) < 3000 and want[3]["faces_collapsed"] > 0 and want[3]["faces_duplicate"] > 0
    ref = MS.cluster(verts, 1.0, rgba=rgba)
    default = M.cluster_vertices(_t(verts), 1.0, rgba=_t(rgba.view(np.int32)))
    tight = M.cluster_vertices(_t(verts), 1.0, rgba=_t(rgba.view(np.int32)), table_log2=10)      # 1024 slots for 1000 vertices
    huge = M.cluster_vertices(_t(verts), 1.0, rgba=_t(rgba.view(np.int32)), table_log2=20)
    for got in (default, tight, huge):
        _assert_clusters(got, ref)
    no_colour = M.cluster_vertices(_t(verts), 1.0, table_log2=10)
    assert no_colour["rgba"] is None and torch.equal(no_colour["positions"], default["positions"])
    # the faces through a table of 4096 slots for 3000 faces and through the default of 8192: the same rows
    lib, vc, f = L.load(), default["vertex_cluster"], _t(faces)
    rows = []
    for log2 in (12, 13, 16):
        kept = torch.full((3000, 3), -9, dtype=torch.int32, device="cuda")
        info = torch.zeros(4, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(lib.sp3_mesh_cluster_faces_ws_bytes(3000, log2)), dtype=torch.uint8, device="cuda")
        L.check(lib.sp3_mesh_cluster_faces(f.data_ptr(), 3000, vc.data_ptr(), 1000, 1, log2, ws.data_ptr(), kept.data_ptr(), info.data_ptr(),
                                           L.stream_ptr()), "sp3_mesh_cluster_faces")
        rows.append((kept.cpu().numpy(), info.cpu().tolist()))
    wf, counts = MS.cluster_faces(faces, ref["vertex_cluster"])
    for kept, info in rows:
        assert info == [len(wf), counts["invalid"], counts["collapsed"], counts["duplicate"]]
        assert np.array_equal(kept[:len(wf)], wf) and (kept[len(wf):] == -9).all()


# ------------------------------------------------------------------------------------------------ 2. one cell, maximal contention
def test_one_cell_of_100000_vertices_sums_beyond_32_bits():
    from spann3r_amd import mesh as M
    n = 100000
    rng = np.random.default_rng(4)
    verts = np.minimum(np.float32(1) - rng.random((n, 3)).astype(np.float32) * np.float32(2.0 ** -12), np.nextafter(np.float32(1), np.float32(0)))
    rgba = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    _, q, _ = MS.cells(verts, 1.0)
    assert q.min() > 65000 and int(q[:, 0].sum()) > 2 ** 32
    ref = MS.cluster(verts, 1.0, rgba=rgba)
    assert ref["n_clusters"] == 1
    for _ in range(2):                                                             # the same bits every run
        _assert_clusters(M.cluster_vertices(_t(verts), 1.0, rgba=_t(rgba.view(np.int32))), ref)


# ------------------------------------------------------------------------------------------------ 3. negatives, unusable, duplicates
def test_negative_coordinates_and_an_origin_off_the_lattice():
    rng = np.random.default_rng(5)
    verts = (rng.random((2000, 3)) * 4 - 3).astype(np.float32)
    origin, cell = (0.13, -0.41, 0.055), 0.37
    o, c = np.asarray(origin, np.float32), np.float32(cell)
    verts[0] = o + c * np.float32(-2)                                              # on a cell corner
    verts[1] = (o[0] + c * np.float32(-3), -0.7, 0.2)                              # on a cell face
    verts[2] = (-1e-9, -1e-9, -1e-9)                                               # just below zero
    verts[3] = o - np.float32(1e-9)
    rgba = rng.integers(0, 2 ** 32, 2000, dtype=np.uint32)
    faces = rng.integers(0, 2000, (6000, 3)).astype(np.int32)
    _check(verts, rgba, faces, cell, origin)
    out, want = _check(verts, rgba, faces, 1.0, (0, 0, 0))
    i, q, ok = MS.cells(verts, 1.0)
    assert ok.all() and i.min() == -3 and (i[2] == -1).all() and (q[2] == 65535).all()


def test_unusable_vertices_and_invalid_faces_are_counted_and_otherwise_absent():
    rng = np.random.default_rng(6)
    verts = (rng.random((500, 3)) * 2).astype(np.float32)
    verts[7], verts[8, 2], verts[9, 0], verts[10, 1] = np.nan, np.inf, -np.inf, 3e9          # |i| >= 2^30 at cell 0.5: 6e9
    verts[11, 0] = np.float32(0.5 * 2.0 ** 30)                                     # i = 2^30 exactly: unusable
    verts[12, 0] = np.float32(0.5 * (2.0 ** 30 - 64))                              # the last usable magnitudes
    rgba = rng.integers(0, 2 ** 32, 500, dtype=np.uint32)
    faces = rng.integers(12, 500, (1500, 3)).astype(np.int32)
    bad = np.array([[7, 20, 21], [20, 8, 21], [20, 21, 9], [10, 11, 30], [500, 1, 2], [1, -1, 2], [1, 2, 2 ** 31 - 1], [-2 ** 31, 1, 2]], np.int32)
    faces[100:108] = bad
    out, want = _check(verts, rgba, faces, 0.5)
    vc = want[4]
    assert (vc[7:12] == -1).all() and vc[12] >= 0 and want[3]["faces_invalid"] == 8
    clean, _ = _check(verts, rgba, np.delete(faces, np.arange(100, 108), 0), 0.5)   # everything else as if they were absent
    assert torch.equal(clean["faces"], out["faces"]) and torch.equal(clean["vertices"], out["vertices"])


def test_duplicates_one_face_per_winding_survives_in_its_own_rotation():
    verts = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.6, 0.4, 0.5], [1.4, 0.6, 0.5], [2.5, 2.5, 0.5]], np.float32)
    rgba = np.arange(6, dtype=np.uint32) * np.uint32(0x01020304)
    # clusters: {0, 3} -> 0, {1, 4} -> 1, {2} -> 2, {5} -> 3
    faces = np.array([[1, 2, 0], [2, 0, 1], [0, 1, 2], [2, 1, 0], [4, 2, 3], [0, 2, 1], [0, 3, 5], [5, 2, 1], [1, 5, 2]], np.int32)
    out, want = _check(verts, rgba, faces, 1.0)
    assert want[2].tolist() == [[1, 2, 0], [2, 1, 0], [3, 2, 1]]                    # the first of each winding, as it was rotated
    assert want[3] == dict(cell=1.0, clusters=4, faces_in=9, faces_collapsed=1, faces_duplicate=5, faces_invalid=0)
    out, want = _check(verts, rgba, faces, 1.0, dedup=False)
    assert len(want[2]) == 8 and want[3]["faces_duplicate"] == 0 and want[2][4].tolist() == [1, 2, 0]


# ------------------------------------------------------------------------------------------------ 4. more than 1024 scan tiles
def test_a_sheet_of_more_than_1024_scan_tiles():
    n, step = 600, np.float32(0.01)
    y, x = np.mgrid[:n, :n]
    verts = np.stack([(x - 200) * step + np.float32(0.003), (y - 300) * step + np.float32(0.003), 0.05 * np.sin(x * 0.02) * np.cos(y * 0.03)],
                     -1).reshape(-1, 3).astype(np.float32)
    tl = (y[:-1, :-1] * n + x[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([tl, tl + 1, tl + n], 1), np.stack([tl + 1, tl + n + 1, tl + n], 1)]).astype(np.int32)
    rgba = (np.arange(n * n, dtype=np.uint32) * np.uint32(2654435761)).astype(np.uint32)
    assert (n * n + 255) // 256 > 1024
    out, want = _check(verts, rgba, faces, 3 * float(step))
    assert want[3]["clusters"] > 256 * 1024 // 9 and 0 < len(want[2]) < len(faces) // 4


# ------------------------------------------------------------------------------------------------ 5. edge sizes and limits
def test_edge_sizes():
    from spann3r_amd import lib as L, mesh as M
    verts, rgba, faces = _block()
    empty_f = np.zeros((0, 3), np.int32)
    _check(np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), empty_f, 1.0)                  # V = 0
    out, _ = _check(np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), faces[:5], 1.0)       # V = 0 with faces: all invalid
    assert out["simplify"]["faces_invalid"] == 5 and out["faces"].shape == (0, 3)
    out, _ = _check(verts, rgba, empty_f, 1.0)                                                   # F = 0
    assert out["vertices"].shape == (0, 3) and out["simplify"]["clusters"] == 27
    out, want = _check(verts, rgba, None, 1.0)                                                   # a cloud comes back as a cloud
    assert out["faces"] is None and out["vertices"].shape == (27, 3)
    out, _ = _check(verts, rgba, faces, 100.0, (-50, -50, -50))                                  # everything collapsed
    assert out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3) and out["colors"].shape == (0, 4)
    assert out["simplify"]["faces_collapsed"] == 3000 and out["simplify"]["clusters"] == 1
    got = M.cluster_vertices(_t(np.zeros((0, 3), np.float32)), 1.0)
    assert got["n_clusters"] == 0 and got["positions"].shape == (0, 3) and got["vertex_cluster"].shape == (0,)
    # the C entry points on the empty sizes: info is written, nothing else is touched
    lib = L.load()
    origin = (L.C.c_float * 3)(0, 0, 0)
    info = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    L.check(lib.sp3_mesh_cluster(None, None, 0, origin, 1.0, 0, None, None, None, None, info.data_ptr(), L.stream_ptr()), "sp3_mesh_cluster")
    assert info.cpu().tolist() == [0, 77, 77, 77]
    L.check(lib.sp3_mesh_cluster_faces(None, 0, None, 0, 1, 0, None, None, info.data_ptr(), L.stream_ptr()), "sp3_mesh_cluster_faces")
    assert info.cpu().tolist() == [0, 0, 0, 0]
    assert lib.sp3_mesh_cluster_ws_bytes(0, 4) == 0 and lib.sp3_mesh_cluster_faces_ws_bytes(0, 4) == 0
    assert lib.sp3_mesh_cluster_ws_bytes(1000, 11) >= 4 * 2048 + 72 * 1000 and lib.sp3_mesh_cluster_faces_ws_bytes(1000, 11) >= 4 * 2048 + 13 * 1000


def test_limits_and_a_bad_cell_raise_before_anything_is_launched():
    from spann3r_amd import lib as L, mesh as M
    lib = L.load()
    top = 2 ** 31 - 1
    origin = (L.C.c_float * 3)(0, 0, 0)
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert lib.sp3_mesh_cluster(None, None, top, origin, 1.0, 31, None, None, None, None, info.data_ptr(), None) != 0
    assert b"out of range" in lib.sp3_last_error()
    assert lib.sp3_mesh_cluster(None, None, 1000, origin, 1.0, 9, None, None, None, None, info.data_ptr(), None) != 0
    assert b"more slots" in lib.sp3_last_error()
    assert lib.sp3_mesh_cluster(None, None, 1024, origin, 1.0, 10, None, None, None, None, info.data_ptr(), None) != 0      # 2^10 must EXCEED the items
    assert lib.sp3_mesh_cluster(None, None, 1000, origin, 1.0, 32, None, None, None, None, info.data_ptr(), None) != 0
    for cell in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.sp3_mesh_cluster(None, None, 1000, origin, cell, 11, None, None, None, None, info.data_ptr(), None) != 0
        assert b"positive and finite" in lib.sp3_last_error()
    assert lib.sp3_mesh_cluster(None, None, 1000, origin, 1.0, 11, None, None, None, None, None, None) != 0
    assert lib.sp3_mesh_cluster_faces(None, top, None, 5, 1, 31, None, None, info.data_ptr(), None) != 0 and b"out of range" in lib.sp3_last_error()
    assert lib.sp3_mesh_cluster_faces(None, 5, None, top, 1, 4, None, None, info.data_ptr(), None) != 0
    assert lib.sp3_mesh_cluster_faces(None, 1000, None, 5, 1, 9, None, None, info.data_ptr(), None) != 0 and b"more slots" in lib.sp3_last_error()
    assert lib.sp3_mesh_cluster_faces(None, 1000, None, 5, 1, 11, None, None, None, None) != 0 and b"null info" in lib.sp3_last_error()
    assert lib.sp3_mesh_cluster_ws_bytes(top, 31) == 0 and lib.sp3_mesh_cluster_ws_bytes(1000, 9) == 0
    assert lib.sp3_mesh_cluster_faces_ws_bytes(top, 31) == 0 and lib.sp3_mesh_cluster_faces_ws_bytes(1000, 9) == 0
    assert info.cpu().tolist() == [0, 0, 0, 0]
    verts, rgba, faces = _block()
    m = _mesh(verts, rgba, faces)
    for cell in (0, -0.5, float("inf"), float("nan"), 1e-60, "x"):
        with pytest.raises(ValueError, match="cell"):
            M.simplify(m, cell)
        with pytest.raises(ValueError, match="cell"):
            M.cluster_vertices(m["vertices"], cell)
    with pytest.raises(ValueError, match="table_log2"):
        M.cluster_vertices(m["vertices"], 1.0, table_log2=9)
    with pytest.raises(ValueError, match="origin"):
        M.simplify(m, 1.0, origin=(0, 0))
    with pytest.raises(RuntimeError, match="CUDA"):
        M.simplify(dict(m, vertices=m["vertices"].cpu()), 1.0)


# ------------------------------------------------------------------------------------------------ 6. the brick scene, end to end
@pytest.fixture(scope="module")
def brick():
    """(the fused brick scene, its unsimplified direct mesh, its unsimplified dense-route mesh)"""
    from spann3r_amd import fusion as F_
    frs = RC.scene_frames()
    vol = F_.BrickTSDFVolume(S["origin"], S["voxel"], S["dims"], trunc=S["trunc"], band=S["band"])
    vol.integrate(intrinsics=[f["K"] for f in frs], cam2world=[f["cam2world"] for f in frs], valid=[_t(f["valid"]) for f in frs],
                  pts=[_t(f["pts"]) for f in frs], images=[_t(f["images"]) for f in frs])
    return vol, vol.extract_mesh(direct=True), vol.extract_mesh()


@pytest.mark.parametrize("direct", [True, False])
def test_simplify_cell_equals_simplify_of_the_extracted_mesh(brick, direct):
    from spann3r_amd import mesh as M
    vol, raw_direct, raw_dense = brick
    raw = raw_direct if direct else raw_dense
    origin = vol.origin if direct else vol.to_dense().origin
    cell = 2 * S["voxel"]
    got = vol.extract_mesh(direct=direct, simplify_cell=cell)
    again = M.simplify(raw, cell, origin=origin)
    assert sorted(got) == sorted(again) == ["bounds", "colors", "faces", "simplify", "vertices"] and got["simplify"] == again["simplify"]
    for k in ("vertices", "colors", "faces"):
        assert torch.equal(got[k], again[k]), k
    assert np.array_equal(got["bounds"], again["bounds"])
    _assert_simplified(got, MS.simplify(*_host(raw), cell, origin), return_map=False)
    assert 0 < got["faces"].shape[0] < raw["faces"].shape[0] and got["simplify"]["faces_in"] == raw["faces"].shape[0]
    print("brick scene (%s): %d faces -> %d at a cell of 2 voxels" % ("direct" if direct else "dense", raw["faces"].shape[0], got["faces"].shape[0]))


def test_the_defaults_return_todays_tensors_and_the_filter_runs_first(brick):
    from spann3r_amd import fusion as F_
    vol, raw_direct, raw_dense = brick
    for direct, raw in ((True, raw_direct), (False, raw_dense)):
        got = vol.extract_mesh(direct=direct, simplify_cell=None)
        assert sorted(got) == sorted(raw) == ["bounds", "colors", "faces", "vertices"]
        for k in ("vertices", "colors", "faces"):
            assert torch.equal(got[k], raw[k]), k
        assert np.array_equal(got["bounds"], raw["bounds"])
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="simplify_cell"):
            vol.extract_mesh(direct=True, simplify_cell=bad)
    cell = 2 * S["voxel"]
    both = vol.extract_mesh(direct=True, min_component_faces=9, simplify_cell=cell)
    fv, fc, ff, stats = MC.filter_mesh(*_host(raw_direct), min_faces=9)
    assert both["components"] == stats and stats["faces_removed"] > 0
    _assert_simplified(both, MS.simplify(fv, fc, ff, cell, vol.origin), return_map=False)
    # scale and transform are applied to the representatives, by the final compaction
    scaled = vol.extract_mesh(direct=True, simplify_cell=cell, scale=10.0, transform=np.diag([-1.0, -1.0, 1.0, 1.0]))
    plain = vol.extract_mesh(direct=True, simplify_cell=cell)
    assert torch.equal(scaled["faces"], plain["faces"])
    assert torch.equal(scaled["vertices"], plain["vertices"] * 10.0 * torch.tensor([-1.0, -1.0, 1.0], device="cuda"))
    # the drivers pass the argument through
    frs = RC.scene_frames()
    args = (torch.stack([_t(f["pts"]) for f in frs]), np.stack([f["K"] for f in frs]), np.stack([f["cam2world"] for f in frs]),
            torch.stack([_t(f["valid"]) for f in frs]).bool(), torch.stack([_t(f["images"]) for f in frs]))
    a, va = F_.fuse_pointmaps(*args, voxel_size=S["voxel"], simplify_cell=cell, return_volume=True)
    b = F_.fuse_pointmaps(*args, voxel_size=S["voxel"])
    assert "simplify" not in b and 0 < a["faces"].shape[0] < b["faces"].shape[0]
    _assert_simplified(a, MS.simplify(*_host(b), cell, va.origin), return_map=False)


# ------------------------------------------------------------------------------------------------ 7. welding the per-frame sheets
def test_two_sheets_of_one_plane_are_welded_into_one_vertex_set():
    from spann3r_amd import mesh as M
    h, w = 40, 56
    y, x = np.mgrid[:h, :w].astype(np.float32)
    frames = []
    for dx, dy in ((0.0, 0.0), (0.004, -0.003)):                                   # the same plane z = 2, sampled from two slightly shifted frames
        frames.append(np.stack([(x - w / 2) * 0.01 + dx, (y - h / 2) * 0.01 + dy, np.full_like(x, 2.0)], -1))
    pts = np.stack(frames).astype(np.float32)
    rng = np.random.default_rng(8)
    scene = M.scene_mesh(_t(pts), _t(rng.random((2, h, w, 3)).astype(np.float32)), _t(np.full((2, h, w), 5.0, np.float32)), 1e-3)
    assert scene["vertices"].shape[0] == 2 * h * w and scene["faces"].shape[0] == 2 * 2 * (h - 1) * (w - 1)
    cell = 0.25                                                                    # 2.5 pixel steps of the x10 positions
    out = M.simplify(scene, cell, return_map=True)
    _assert_simplified(out, MS.simplify(*_host(scene), cell))
    one = M.simplify(dict(scene, vertices=scene["vertices"][:h * w], colors=scene["colors"][:h * w], faces=scene["faces"][:2 * (h - 1) * (w - 1)]), cell)
    assert out["vertices"].shape[0] < 2 * one["vertices"].shape[0] and out["vertices"].shape[0] < 2 * h * w
    assert out["vertices"].shape[0] <= one["vertices"].shape[0] + 2 * (h + w)        # about one sheet: the shifted border may add cells
    vc = out["vertex_cluster"].cpu().numpy()
    # the clusters hold vertices of both frames (all but a border row and column, which the shift can leave to one frame)
    assert len(np.intersect1d(vc[:h * w], vc[h * w:])) > 0.5 * out["simplify"]["clusters"]


# ------------------------------------------------------------------------------------------------ 8. the demo's arguments
@pytest.mark.parametrize("flags,message", [(["--simplify_voxels", "2"], "needs --fused"), (["--simplify", "0.1"], "needs --fused or --save_glb"),
                                           (["--fused", "--simplify", "-1"], "positive and finite")])
def test_demo_loop_rejects_the_simplify_flags_without_their_prerequisite(monkeypatch, capsys, flags, message):
    import demo_loop
    monkeypatch.setattr(sys, "argv", ["demo_loop.py", "--tiny"] + flags)
    with pytest.raises(SystemExit) as e:
        demo_loop.main()
    assert e.value.code == 2 and message in capsys.readouterr().err
