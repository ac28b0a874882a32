"""sp3_mesh_face_frames / sp3_mesh_sample / sp3_mesh_vertex_normals on the device (csrc/mesh_sample.hip; include/spann3r_hip.h "Mesh
surface sampling and normals") and what drives them: mesh.face_frames / surface_area / sample_surface / vertex_normals and
evaluate.evaluate_meshes.

The anchor is tests/mesh_sample_ref.py (the numpy restatement, checked against a sample-by-sample loop and for its statistics in
tests/test_mesh_sample_cpu.py).  Every comparison with it is exact: integer arrays equal, float rows bit for bit -- so nothing
statistical is run here.  The inputs are the smallest that reach each failure mode: a prefix sum across more than 1024 scan tiles,
faces that must never be drawn (invalid, non-finite, without area, below 2^-32 of the largest), one vertex under maximal contention,
and the empty sizes."""
import sys

import numpy as np
import pytest
import torch

import bricks_ref as BR
import mesh_sample_ref as R
import raycast_ref as RC

pytestmark = pytest.mark.gpu

S = BR.SCENE


def _t(x):
    return torch.from_numpy(np.array(x)).cuda()


def _mesh(verts, rgba, faces):
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    out = dict(vertices=_t(verts), faces=_t(np.asarray(faces, np.int32).reshape(-1, 3)), bounds=None)
    if rgba is not None:
        out["colors"] = _t(np.asarray(rgba, np.uint32).view(np.uint8).reshape(-1, 4))
    return out


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _assert_frames(m, fr):
    """mesh.face_frames of the device mesh against the restatement's dict"""
    from spann3r_amd import mesh as M
    got = M.face_frames(m)
    assert got["cum"].dtype == torch.int64 and got["face_normals"].dtype == torch.float32
    assert np.array_equal(got["cum"].cpu().numpy().view(np.uint64), fr["cum"])
    assert got["W"] == fr["W"] and np.float64(got["dmax"]).view(np.uint64) == np.float64(fr["dmax"]).view(np.uint64)
    assert got["info"].cpu().numpy().view(np.uint64).tolist() == [fr["W"], int(np.float64(fr["dmax"]).view(np.uint64))]
    assert np.array_equal(_bits(got["face_normals"].cpu().numpy()), _bits(fr["face_normals"]))
    assert got["area"] == fr["area"] == M.surface_area(m)
    return got


def _assert_sample(m, verts, rgba, faces, n, seed=0, fr=None):
    """mesh.sample_surface against the restatement, bit for bit; -> (device dict, reference dict)"""
    from spann3r_amd import mesh as M
    fr = R.face_frames(verts, faces) if fr is None else fr
    got = M.sample_surface(m, n, seed=seed, return_faces=True)
    want = R.sample(verts, rgba, faces, n, seed, frames=fr)
    assert got["points"].dtype == got["normals"].dtype == torch.float32 and got["faces"].dtype == torch.int32
    assert got["points"].shape == got["normals"].shape == (n, 3) and got["faces"].shape == (n,)
    assert np.array_equal(got["faces"].cpu().numpy(), want["face_index"])
    assert np.array_equal(_bits(got["points"].cpu().numpy()), _bits(want["points"]))
    assert np.array_equal(_bits(got["normals"].cpu().numpy()), _bits(want["normals"]))
    if rgba is None:
        assert got["colors"] is None
    else:
        assert got["colors"].dtype == torch.uint8 and got["colors"].shape == (n, 4)
        assert np.array_equal(got["colors"].cpu().numpy().view(np.uint32).ravel(), want["rgba"])
    assert got["area"] == fr["area"]
    return got, want


def _assert_vertex_normals(m, verts, faces, fr=None):
    from spann3r_amd import mesh as M
    got = M.vertex_normals(m)
    want = R.vertex_normals(verts, faces, frames=fr)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    return got, want


# ------------------------------------------------------------------------------------------------ 1. the three-face scene
SCENE_V = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (5, 0, 0), (8, 0, 0), (5, 1, 0)], np.float32)
SCENE_F = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6]], np.int32)
SCENE_C = np.array([0xFF0000FF, 0xFF00FF00, 0xFFFF0000, 0x80FFFFFF, 0x00000000, 0xFFFFFFFF, 0x7F7F7F7F], np.uint32)


def test_the_three_face_scene_equals_the_restatement():
    from spann3r_amd import mesh as M
    m = _mesh(SCENE_V, SCENE_C, SCENE_F)
    fr = R.face_frames(SCENE_V, SCENE_F)
    _assert_frames(m, fr)
    got, want = _assert_sample(m, SCENE_V, SCENE_C, SCENE_F, 65536, fr=fr)
    assert np.bincount(want["face_index"]).tolist() == [12916, 13059, 39561]          # (what tests/test_mesh_sample_cpu.py scores)
    _assert_sample(m, SCENE_V, SCENE_C, SCENE_F, 1000, seed=12345, fr=fr)
    _assert_sample(m, SCENE_V, SCENE_C, SCENE_F, 1000, seed=2 ** 64 - 1, fr=fr)
    no_colour = _mesh(SCENE_V, None, SCENE_F)
    _assert_sample(no_colour, SCENE_V, None, SCENE_F, 1000, fr=fr)
    assert "faces" not in M.sample_surface(no_colour, 10)
    _assert_vertex_normals(m, SCENE_V, SCENE_F, fr)
    with pytest.raises(ValueError, match="cloud"):
        M.sample_surface(dict(m, faces=None), 10)
    with pytest.raises(ValueError, match="cloud"):
        M.vertex_normals(dict(m, faces=None))
    with pytest.raises(ValueError, match="cloud"):
        M.surface_area(dict(m, faces=None))
    with pytest.raises(RuntimeError, match="CUDA"):
        M.sample_surface(dict(m, vertices=m["vertices"].cpu()), 10)


# ------------------------------------------------------------------------------------------------ 2. more than 1024 scan tiles
@pytest.fixture(scope="module")
def sheet():
    """the 600 x 600 jittered sheet of tests/test_mesh_simplify_gpu.py: (verts, rgba, faces, the restatement's frames)"""
    n, step = 600, np.float32(0.01)
    y, x = np.mgrid[:n, :n]
    verts = np.stack([(x - 200) * step + np.float32(0.003), (y - 300) * step + np.float32(0.003), 0.05 * np.sin(x * 0.02) * np.cos(y * 0.03)],
                     -1).reshape(-1, 3).astype(np.float32)
    tl = (y[:-1, :-1] * n + x[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([tl, tl + 1, tl + n], 1), np.stack([tl + 1, tl + n + 1, tl + n], 1)]).astype(np.int32)
    rgba = (np.arange(n * n, dtype=np.uint32) * np.uint32(2654435761)).astype(np.uint32)
    assert len(faces) == 2 * 599 * 599 and (len(faces) + 255) // 256 > 1024
    return verts, rgba, faces, R.face_frames(verts, faces)


def test_a_sheet_of_more_than_1024_scan_tiles(sheet):
    verts, rgba, faces, fr = sheet
    m = _mesh(verts, rgba, faces)
    got = _assert_frames(m, fr)
    assert np.array_equal(got["cum"].cpu().numpy().view(np.uint64), np.cumsum(fr["w"], dtype=np.uint64))
    _, want = _assert_sample(m, verts, rgba, faces, 2 ** 18, fr=fr)
    assert want["face_index"].min() < 256 and want["face_index"].max() >= len(faces) - 256      # the first and the last tile are drawn from
    _assert_vertex_normals(m, verts, faces, fr)


# ------------------------------------------------------------------------------------------------ 3. degenerates
def test_degenerate_faces_are_never_drawn_and_leave_their_neighbours_alone():
    rng = np.random.default_rng(21)
    nv = 300
    verts = rng.normal(size=(nv, 3)).astype(np.float32)
    verts[10], verts[11], verts[12] = (2, 4, 6), (1, 2, 3), (3, 6, 9)               # collinear, exactly: zero area
    verts[20, 1] = np.nan
    verts[21, 2] = np.inf
    rgba = rng.integers(0, 2 ** 32, nv, dtype=np.uint32)
    good = rng.integers(30, nv, (900, 3)).astype(np.int32)
    good = good[(good[:, 0] != good[:, 1]) & (good[:, 1] != good[:, 2]) & (good[:, 0] != good[:, 2])]
    bad = np.array([[10, 11, 12], [12, 10, 11], [40, 40, 41], [42, 43, 42], [44, 44, 44], [-1, 50, 51], [50, nv, 51], [50, 51, 2 ** 31 - 1],
                    [-2 ** 31, 50, 51], [20, 60, 61], [60, 21, 61], [20, 21, 62]], np.int32)
    where = np.sort(rng.choice(len(good), len(bad), replace=False))
    faces = np.insert(good, where, bad, axis=0)
    is_bad = np.ones(len(faces), bool)
    is_bad[np.setdiff1d(np.arange(len(faces)), where + np.arange(len(bad)))] = False
    assert np.array_equal(faces[is_bad], bad) and np.array_equal(faces[~is_bad], good)
    fr = R.face_frames(verts, faces)
    assert (fr["w"][is_bad] == 0).all() and (fr["w"][~is_bad] > 0).all() and (fr["face_normals"][is_bad] == 0).all()
    m = _mesh(verts, rgba, faces)
    _assert_frames(m, fr)
    got, want = _assert_sample(m, verts, rgba, faces, 65536, fr=fr)
    assert not is_bad[want["face_index"]].any()
    _, vn = _assert_vertex_normals(m, verts, faces, fr)
    assert np.isfinite(vn).all() and (vn[[20, 21]] == 0).all()
    # the same mesh without them: the same weights, the same draws (of the renumbered faces), the same vertex normals
    clean, _ = _assert_sample(_mesh(verts, rgba, good), verts, rgba, good, 65536)
    assert torch.equal(clean["points"], got["points"]) and torch.equal(clean["colors"], got["colors"]) and torch.equal(clean["normals"], got["normals"])
    assert np.array_equal(np.flatnonzero(~is_bad)[clean["faces"].cpu().numpy()], want["face_index"])
    assert np.array_equal(_bits(R.vertex_normals(verts, good)), _bits(vn))


# ------------------------------------------------------------------------------------------------ 4. sizes and scales
def test_faces_2_to_the_20_and_2_to_the_40_times_smaller_than_the_largest():
    k = 4096
    big = np.array([[0, 0, 0], [1024, 0, 0], [0, 1024, 0]], np.float32)               # d = 2^20
    tiny = np.array([[0, 0, 5], [2.0 ** -10, 0, 5], [0, 2.0 ** -10, 5]], np.float32)  # d = 2^-20: 2^-40 of the largest, w = 0
    mid = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float32)[None] + np.arange(k, dtype=np.float32)[:, None, None] * np.float32(2)      # d = 1: w = 2^12
    verts = np.concatenate([big, tiny, mid.reshape(-1, 3)])
    faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    fr = R.face_frames(verts, faces)
    assert fr["w"][0] == 2 ** 32 and fr["w"][1] == 0 and (fr["w"][2:] == 2 ** 12).all() and fr["d"][1] == 2.0 ** -20
    m = _mesh(verts, None, faces)
    _assert_frames(m, fr)
    _, want = _assert_sample(m, verts, None, faces, 65536, fr=fr)
    hits = np.bincount(want["face_index"], minlength=len(faces))
    assert hits[1] == 0 and 100 < hits[2:].sum() < 500                              # 65536 * 2^-8 = 256 expected on the 4096 small faces together
    _assert_vertex_normals(m, verts, faces, fr)


def test_edge_sizes_and_a_mesh_without_area():
    from spann3r_amd import lib as L, mesh as M
    one = _mesh(SCENE_V, SCENE_C, SCENE_F[2:])                                        # F = 1
    _assert_frames(one, R.face_frames(SCENE_V, SCENE_F[2:]))
    _assert_sample(one, SCENE_V, SCENE_C, SCENE_F[2:], 3000)
    _assert_vertex_normals(one, SCENE_V, SCENE_F[2:])
    empty_f = np.zeros((0, 3), np.int32)
    flat = np.array([[0, 0, 1], [1, 1, 1], [0, 1, 9], [-1, 2, 3]], np.int32)         # all degenerate or invalid
    for faces in (empty_f, flat):
        m = _mesh(SCENE_V, SCENE_C, faces)
        with pytest.raises(ValueError, match="no area to sample"):
            M.sample_surface(m, 5)
        fr = _assert_frames(m, R.face_frames(SCENE_V, faces))
        assert fr["W"] == 0 and fr["dmax"] == 0.0 and fr["area"] == 0.0
        got = M.sample_surface(m, 0, return_faces=True)                              # n = 0: empties of the right dtypes, whatever the mesh
        assert got["points"].shape == (0, 3) and got["normals"].shape == (0, 3) and got["colors"].shape == (0, 4) and got["faces"].shape == (0,)
        assert (got["points"].dtype, got["normals"].dtype, got["colors"].dtype, got["faces"].dtype) == (torch.float32, torch.float32, torch.uint8, torch.int32)
        assert (M.vertex_normals(m) == 0).all() and M.vertex_normals(m).shape == (7, 3)
    got = M.sample_surface(_mesh(SCENE_V, SCENE_C, SCENE_F), 0)
    assert got["points"].shape == (0, 3) and got["area"] == R.face_frames(SCENE_V, SCENE_F)["area"]
    nov = _mesh(np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), SCENE_F)        # V = 0: every face invalid
    assert M.vertex_normals(nov).shape == (0, 3) and M.surface_area(nov) == 0.0
    with pytest.raises(ValueError, match="no area to sample"):
        M.sample_surface(nov, 1)
    with pytest.raises(ValueError, match="n = -1"):
        M.sample_surface(one, -1)
    # the C entry points: nfaces = 0 writes info = 0 and nothing else; the limits raise before anything is launched
    lib = L.load()
    info = torch.full((3,), 77, dtype=torch.int64, device="cuda")
    L.check(lib.sp3_mesh_face_frames(None, 0, None, 0, None, None, None, info.data_ptr(), L.stream_ptr()), "sp3_mesh_face_frames")
    assert info.cpu().tolist() == [0, 0, 77]
    top = 2 ** 31 - 1
    assert lib.sp3_mesh_face_frames(None, top, None, 5, None, None, None, info.data_ptr(), None) != 0 and b"out of range" in lib.sp3_last_error()
    assert lib.sp3_mesh_face_frames(None, 5, None, top, None, None, None, info.data_ptr(), None) != 0 and b"out of range" in lib.sp3_last_error()
    assert lib.sp3_mesh_face_frames(None, 5, None, 5, None, None, None, None, None) != 0 and b"null info" in lib.sp3_last_error()
    assert lib.sp3_mesh_sample(None, None, 5, None, top, None, None, 1, 0, None, None, None, None, None) != 0 and b"out of range" in lib.sp3_last_error()
    assert lib.sp3_mesh_sample(None, None, 5, None, 0, None, None, 1, 0, None, None, None, None, None) != 0 and b"no area to sample" in lib.sp3_last_error()
    assert lib.sp3_mesh_sample(None, None, 5, None, 5, None, None, 0, 0, None, None, None, None, None) == 0      # nsamples = 0 launches nothing
    assert lib.sp3_mesh_vertex_normals(None, top, None, 5, None, None, None, None) != 0 and b"out of range" in lib.sp3_last_error()
    assert lib.sp3_mesh_vertex_normals(None, 0, None, 5, None, None, None, None) == 0
    assert lib.sp3_mesh_face_frames_ws_bytes(0) == 0 and lib.sp3_mesh_face_frames_ws_bytes(top) == 0 and lib.sp3_mesh_face_frames_ws_bytes(257) == 16
    assert lib.sp3_mesh_vertex_normals_ws_bytes(0) == 0 and lib.sp3_mesh_vertex_normals_ws_bytes(top) == 0 and lib.sp3_mesh_vertex_normals_ws_bytes(10) == 240
    assert info.cpu().tolist() == [0, 0, 77]


# ------------------------------------------------------------------------------------------------ 5. vertex normals under contention
def test_a_star_of_10000_faces_on_one_vertex():
    k = 10000
    rng = np.random.default_rng(9)
    ang = np.arange(k) * (2 * np.pi / k)
    ring = np.stack([np.cos(ang) * (1 + 0.3 * rng.random(k)), np.sin(ang) * (1 + 0.3 * rng.random(k)), 0.2 * rng.normal(size=k)], 1)
    verts = np.concatenate([[[0, 0, 0.5]], ring, [[7, 7, 7]]]).astype(np.float32)      # the last vertex: no face names it
    faces = np.stack([np.zeros(k, np.int64), 1 + np.arange(k), 1 + (np.arange(k) + 1) % k], 1).astype(np.int32)
    fr = R.face_frames(verts, faces)
    sums = R.vertex_sums(verts, faces, fr)
    assert abs(int(sums[0, 2])) > 2 ** 32                                           # beyond 32 bits on the one contended sum
    m = _mesh(verts, None, faces)
    for _ in range(2):                                                             # the same bits every run
        got, want = _assert_vertex_normals(m, verts, faces, fr)
    assert (want[-1] == 0).all() and want[0, 2] > 0.9
    # against np.add.at on int64, directly
    f64 = faces.astype(np.int64)
    q = np.rint(fr["n"] / fr["dmax"] * 1073741824.0).astype(np.int64)
    direct = np.zeros((len(verts), 3), np.int64)
    for j in range(3):
        np.add.at(direct, f64[:, j], q)
    assert np.array_equal(direct, sums)


# ------------------------------------------------------------------------------------------------ 6. determinism
def test_two_runs_and_permuted_faces(sheet):
    from spann3r_amd import mesh as M
    verts, rgba, faces, _ = sheet
    keep = np.random.default_rng(2).permutation(len(faces))[:200000]                  # a ragged part of the sheet, in a shuffled order
    part = np.ascontiguousarray(faces[np.sort(keep)])
    perm = np.ascontiguousarray(faces[keep])
    m, mp = _mesh(verts, rgba, part), _mesh(verts, rgba, perm)
    a, b = M.sample_surface(m, 50000, seed=7, return_faces=True), M.sample_surface(m, 50000, seed=7, return_faces=True)
    for k in ("points", "normals", "colors", "faces"):
        assert torch.equal(a[k], b[k]), k
    assert a["area"] == b["area"]
    assert torch.equal(M.sample_surface(m, 20000, seed=7)["points"], a["points"][:20000])      # the first n of a longer draw
    assert not torch.equal(M.sample_surface(m, 50000, seed=8)["points"], a["points"])
    na, nb, npm = M.vertex_normals(m), M.vertex_normals(m), M.vertex_normals(mp)
    assert torch.equal(na, nb) and torch.equal(na, npm)                             # integer sums: the order of the faces does not matter
    _assert_sample(mp, verts, rgba, perm, 50000, seed=7)                            # the permuted mesh equals the restatement run on it
    assert M.surface_area(mp) == M.surface_area(m)                                  # W is an integer sum too, dmax a maximum


# ------------------------------------------------------------------------------------------------ 7. the brick scene, end to end
@pytest.fixture(scope="module")
def brick():
    from spann3r_amd import fusion as F_
    frs = RC.scene_frames()
    vol = F_.BrickTSDFVolume(S["origin"], S["voxel"], S["dims"], trunc=S["trunc"], band=S["band"])
    vol.integrate(intrinsics=[f["K"] for f in frs], cam2world=[f["cam2world"] for f in frs], valid=[_t(f["valid"]) for f in frs],
                  pts=[_t(f["pts"]) for f in frs], images=[_t(f["images"]) for f in frs])
    return vol


@pytest.mark.parametrize("direct", [True, False])
@pytest.mark.parametrize("cells", [None, 2])
def test_the_fused_surface_of_the_brick_scene(brick, direct, cells):
    m = brick.extract_mesh(direct=direct, simplify_cell=None if cells is None else cells * S["voxel"])
    verts, faces = m["vertices"].cpu().numpy(), m["faces"].cpu().numpy()
    rgba = m["colors"].cpu().numpy().view(np.uint32).ravel()
    assert len(faces) > 1000
    fr = R.face_frames(verts, faces)
    _assert_frames(m, fr)
    _assert_sample(m, verts, rgba, faces, 50000, fr=fr)
    _assert_vertex_normals(m, verts, faces, fr)
    print("brick scene (%s%s): %d faces, area %.6f" % ("direct" if direct else "dense", "" if cells is None else ", cell of %d voxels" % cells,
                                                       len(faces), fr["area"]))


# ------------------------------------------------------------------------------------------------ 8. evaluate_meshes
def _plane(mirror):
    """a plane of 2 x 1 units: a 64 x 64 grid of cells on one half, two triangles on the other"""
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


def test_evaluate_meshes_scores_the_surface_and_not_the_tessellation():
    """One plane, tessellated twice (the fine half left, then right).  Measured on the host with the restatement and scipy's cKDTree:
    the area-sampled acc / comp are 0.00276 / 0.00277 at 65536 samples (the expected nearest-neighbour spacing, 0.5 / sqrt(32768));
    the vertex sets give 0.3096 / 0.3096 without ICP and 0.1349 / 0.1349 after a point-to-point ICP from identity, which slides the
    plane by 0.49 along itself.  The bars: below 0.01, and above 0.1."""
    from spann3r_amd import evaluate as E
    (va, fa), (vb, fb) = _plane(False), _plane(True)
    a, b = _mesh(va, np.zeros(len(va), np.uint32), fa), _mesh(vb, np.zeros(len(vb), np.uint32), fb)
    r = E.evaluate_meshes(a, b, n_samples=65536, icp=False)
    print("area-sampled: acc %.5f comp %.5f nc1 %.5f nc2 %.5f, areas %.6f %.6f" % (r["acc"], r["comp"], r["nc1"], r["nc2"], r["pred_area"], r["gt_area"]))
    assert r["acc"] < 0.01 and r["comp"] < 0.01
    assert r["nc1"] == 1.0 and r["nc2"] == 1.0                                      # the exact face normals of one plane
    assert r["pred_area"] == r["gt_area"] == 2.0 and r["samples"] == 65536 and np.array_equal(r["transformation"], np.eye(4))
    assert sorted(r) == sorted(["acc", "comp", "nc1", "nc2", "acc_med", "comp_med", "nc1_med", "nc2_med", "transformation", "pred_area", "gt_area",
                                "samples"])
    rv = E.evaluate_reconstruction(a["vertices"], b["vertices"], threshold=0.1)
    print("vertices: acc %.5f comp %.5f" % (rv["acc"], rv["comp"]))
    assert rv["acc"] > 0.1 and rv["comp"] > 0.1                                     # the bias the area sampling removes
    ri = E.evaluate_meshes(a, b, n_samples=65536, icp=True)
    T = ri["transformation"]
    print("with ICP: acc %.5f comp %.5f, T - I at most %.2e" % (ri["acc"], ri["comp"], np.abs(T - np.eye(4)).max()))
    assert np.isfinite(T).all() and np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-9) and np.linalg.det(T[:3, :3]) > 0
    assert np.array_equal(T[3], [0, 0, 0, 1]) and ri["acc"] < 0.01 and ri["comp"] < 0.01
    with pytest.raises(ValueError, match="n_samples"):
        E.evaluate_meshes(a, b, n_samples=0)
    with pytest.raises(ValueError, match="no area to sample"):
        E.evaluate_meshes(dict(a, faces=a["faces"][:0]), b, n_samples=10)


# ------------------------------------------------------------------------------------------------ 9. the demo's arguments
@pytest.mark.parametrize("flags,message", [(["--eval_samples", "1000"], "needs --fused --rgbd --eval"), (["--glb_normals"], "needs --save_glb"),
                                           (["--glb_normals", "--save_glb", "x.glb", "--as_pointcloud"], "needs a mesh")])
def test_demo_loop_rejects_the_new_flags_without_their_prerequisite(monkeypatch, capsys, flags, message):
    import demo_loop
    monkeypatch.setattr(sys, "argv", ["demo_loop.py", "--tiny"] + flags)
    with pytest.raises(SystemExit) as e:
        demo_loop.main()
    assert e.value.code == 2 and message in capsys.readouterr().err
