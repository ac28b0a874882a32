"""The numpy restatement of the TSDF fusion rules (tests/fusion_ref.py) checked on its own, and the argument errors of
spann3r_amd.fusion that need no device.  No GPU."""
import itertools
import math

import numpy as np
import pytest
import torch

import fusion_ref as FR


# ------------------------------------------------------------------------------------------------ the tetrahedra
def test_kuhn_cut_fills_the_cube_with_positive_tetrahedra():
    vol = 0.0
    for tet in FR.TET:
        p = np.array([FR.corner_offset(c) for c in tet], np.float64)
        det = np.linalg.det(p[1:] - p[0])
        assert det > 0                                      # the header lists every tetrahedron with positive orientation
        vol += det / 6
        assert tet[0] == 0 and tet[3] == 7                  # around the diagonal 0-7
    assert abs(vol - 1.0) < 1e-12
    assert len({tuple(sorted(t)) for t in FR.TET}) == 6


def _face_triangles(axis, side):
    """the triangles (sets of corner coordinates with `axis` dropped) that the six tetrahedra leave on the cube face axis = side"""
    out = set()
    for tet in FR.TET:
        for tri in itertools.combinations(tet, 3):
            pts = [FR.corner_offset(c) for c in tri]
            if all(p[axis] == side for p in pts):
                out.add(frozenset(tuple(v for a, v in enumerate(p) if a != axis) for p in pts))
    return out


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_cut_is_face_compatible_across_neighbours(axis):
    lo, hi = _face_triangles(axis, 0), _face_triangles(axis, 1)
    assert len(lo) == 2 and lo == hi                        # the face a cell shows its +axis neighbour is cut as that neighbour cuts it


def test_every_case_is_oriented_to_the_positive_side():
    """for each tetrahedron and each sign pattern: the triangles the rule emits, with vertices at the edge midpoints, have normals
    that point from the inside vertices to the outside ones"""
    for tet in FR.TET:
        p = np.array([FR.corner_offset(c) for c in tet], np.float64)
        for case in range(1, 15):
            ins = [m for m in range(4) if (case >> m) & 1]
            out = [m for m in range(4) if not (case >> m) & 1]
            tris = FR.CASES[case]
            assert len(tris) == (2 if len(ins) == 2 else 1)
            direction = p[out].mean(0) - p[ins].mean(0)
            for tri in tris:
                assert all(((case >> a) & 1) != ((case >> b) & 1) for a, b in tri)
                q = [(p[a] + p[b]) / 2 for a, b in tri]
                nrm = np.cross(q[1] - q[0], q[2] - q[0])
                assert np.dot(nrm, direction) > 0, (tet, case)


# ------------------------------------------------------------------------------------------------ extraction
N, H_VOX, RADIUS = 20, 0.1, 0.63
ORIGIN = (-0.95, -0.93, -0.97)
CENTRE = (0.013, -0.021, 0.007)
TRUNC = 3 * H_VOX


@pytest.fixture(scope="module")
def sphere():
    tsdf, weight = FR.sphere_volume((N, N, N), ORIGIN, H_VOX, CENTRE, RADIUS, TRUNC)
    return tsdf, weight, FR.extract_ref(tsdf, weight, None, ORIGIN, H_VOX)


def test_sphere_is_a_closed_oriented_manifold(sphere):
    _, _, (verts, rgba, faces) = sphere
    rep = FR.manifold_report(faces)
    assert len(faces) > 500 and rep["closed"] and rep["bad"] == 0
    assert rep["euler"] == 2
    assert len(np.unique(faces)) == len(verts)              # all voxels observed: no vertex without a face
    assert (rgba == 0xffffffff).all()
    # outward: the signed volume is positive and close to the ball's
    a, b, c = (verts[faces[:, k]] - np.asarray(CENTRE) for k in range(3))
    vol = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6
    assert 0.9 < vol / (4 / 3 * math.pi * RADIUS ** 3) < 1.0


def test_sphere_vertices_within_the_interpolation_error(sphere):
    """A vertex is the zero of the linear interpolant of phi (the distance to the sphere) between two voxels a, b that lie on
    opposite sides, |a - b| = L <= sqrt(3) h.  Along that segment the second derivative of phi is e^T (I - n n^T) e / r <= 1 / r with r
    the distance from the centre, and every point of a segment that crosses the sphere has r >= R - L; both endpoints have
    |phi| <= L <= trunc, so neither is clipped.  Linear interpolation of a function with |f''| <= M over a length L errs by at
    most M L^2 / 8, so at the vertex (interpolant = 0): |phi| <= L^2 / (8 (R - L)) = 3 h^2 / (8 (R - sqrt(3) h)).  The stored
    tsdf = phi / trunc is rounded to fp32 (2^-24 relative on values <= 1): another 2^-24 trunc at most."""
    _, _, (verts, _, _) = sphere
    L = math.sqrt(3) * H_VOX
    assert L <= TRUNC
    bound = L * L / (8 * (RADIUS - L)) + 2.0 ** -24 * TRUNC
    err = np.abs(np.linalg.norm(verts - np.asarray(CENTRE), axis=1) - RADIUS)
    assert err.max() <= bound, (err.max(), bound)
    assert err.max() > bound / 50                           # (the bound is not vacuous)


def test_fp32_restatement_has_the_same_topology(sphere):
    tsdf, weight, (verts, _, faces) = sphere
    v32, _, f32 = FR.extract_ref(tsdf, weight, None, np.float32(ORIGIN), np.float32(H_VOX), dtype=np.float32)
    assert v32.dtype == np.float32 and np.array_equal(f32, faces)
    assert np.abs(v32 - verts).max() < 1e-5


def test_sub_box_gives_an_open_surface_bounded_by_the_box(sphere):
    tsdf, weight, _ = sphere
    lo, hi = (3, 2, 4), (12, 17, 15)                        # observed voxels lo..hi per axis (x, y, z): the sphere leaves through the faces
    w = np.zeros_like(weight)
    w[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = 1
    verts, _, faces = FR.extract_ref(tsdf, w, None, ORIGIN, H_VOX)
    rep = FR.manifold_report(faces)
    assert len(faces) > 50 and rep["bad"] == 0 and len(rep["boundary"]) > 0
    plo = np.asarray(ORIGIN) + np.asarray(lo) * H_VOX
    phi = np.asarray(ORIGIN) + np.asarray(hi) * H_VOX
    for a, b in rep["boundary"]:                            # a boundary edge lies in a face of the box of observed voxels
        on = (np.abs(verts[[a, b]] - plo) < 1e-9).all(0) | (np.abs(verts[[a, b]] - phi) < 1e-9).all(0)
        assert on.any(), (verts[a], verts[b])
    used = np.unique(faces)
    assert (verts[used] >= plo - 1e-9).all() and (verts[used] <= phi + 1e-9).all()


def test_nothing_to_extract():
    ones, zeros = np.ones((5, 6, 7), np.float32), np.zeros((5, 6, 7), np.float32)
    for tsdf, weight in ((ones, ones), (-ones, zeros), (ones, zeros)):                # all positive; unobserved
        verts, rgba, faces = FR.extract_ref(tsdf, weight, None, (0, 0, 0), 0.1)
        assert verts.shape == (0, 3) and rgba.shape == (0,) and faces.shape == (0, 3)
    verts, _, faces = FR.extract_ref(-ones, ones, None, (0, 0, 0), 0.1)              # all inside: no crossing either
    assert len(verts) == 0 and len(faces) == 0


def test_colours_follow_the_interpolation():
    tsdf = np.ones((2, 2, 2), np.float32)
    tsdf[0, 0, 0] = -1.0 / 3.0                              # t = 1/4 on the three axis edges, 1/4 on the diagonals too
    rgb = np.zeros((2, 2, 2, 3), np.float32)
    rgb[0, 0, 0] = (1.0, 0.0, 0.5)
    verts, rgba, faces = FR.extract_ref(tsdf, np.ones_like(tsdf), rgb, (0, 0, 0), 1.0)
    assert len(verts) == 7 and len(faces) == 6              # the corner is cut off in each of the six tetrahedra
    assert np.allclose(verts[0], (0.25, 0, 0)) and np.allclose(verts[6], (0.25, 0.25, 0.25))
    r, g, b = rgba & 255, (rgba >> 8) & 255, (rgba >> 16) & 255
    assert (r == 191).all() and (g == 0).all() and (b == 96).all() and (rgba >> 24 == 255).all()      # floor(0.75 * 255 + 0.5), floor(0.375 * 255 + 0.5)
    assert FR.manifold_report(faces)["bad"] == 0


# ------------------------------------------------------------------------------------------------ integration
@pytest.fixture(scope="module")
def frames():
    return FR.scene_frames()


@pytest.mark.parametrize("path", ["depth", "pts"])
def test_integrate_a_then_b_equals_a_plus_b(frames, path):
    S = FR.SCENE
    fr = FR.as_path(frames, path)
    args = (np.float32(S["origin"]), np.float32(S["voxel"]), np.float32(S["trunc"]), np.float32)
    one = FR.integrate_ref(*FR.empty_volume(S["dims"]), fr, *args)
    two = FR.integrate_ref(*FR.integrate_ref(*FR.empty_volume(S["dims"]), fr[:3], *args), fr[3:], *args)
    for a, b in zip(one, two):
        assert a.dtype == np.float32 and np.array_equal(a, b, equal_nan=True)
    tsdf, weight, rgb = one
    assert np.isfinite(tsdf).all() and np.isfinite(weight).all() and np.isfinite(rgb).all()
    assert tsdf.max() == 1.0 and tsdf.min() >= -1.0 and (weight > 0).mean() > 0.3 and (weight == 0).any()
    assert rgb.min() >= 0.0 and rgb.max() <= 1.0 and (rgb[weight == 0] == 0).all() and (tsdf[weight == 0] == 1).all()


def test_scene_reaches_every_skip_rule(frames):
    """the synthetic scene of the GPU tests has voxels behind a camera, outside an image, beyond -trunc, on invalid, non-finite,
    zero and negative pixels and on pixels of zero / non-finite weight"""
    S = FR.SCENE
    cx, cy, cz = FR.centres(S["origin"], S["voxel"], S["dims"])
    X = np.stack(np.meshgrid(cx, cy, cz, indexing="ij"), -1).reshape(-1, 3)
    seen = dict(behind=0, outside=0, invalid=0, nan=0, zero=0, negative=0, beyond=0, weight=0)
    for fr in frames:
        m = fr["w2c"].astype(np.float64).reshape(3, 4)
        Xc = X @ m[:, :3].T + m[:, 3]
        seen["behind"] += int((Xc[:, 2] <= 0).sum())
        front = Xc[Xc[:, 2] > 0]
        px = np.floor(fr["fu"] * front[:, 0] / front[:, 2] + fr["cu"] + 0.5).astype(int)
        py = np.floor(fr["fv"] * front[:, 1] / front[:, 2] + fr["cv"] + 0.5).astype(int)
        inside = (px >= 0) & (px < S["w"]) & (py >= 0) & (py < S["h"])
        seen["outside"] += int((~inside).sum())
        px, py, zc = px[inside], py[inside], front[inside, 2]
        d = fr["depth"][py, px].astype(np.float64)
        seen["invalid"] += int((fr["valid"][py, px] == 0).sum())
        seen["nan"] += int(np.isnan(d).sum())
        seen["zero"] += int((d == 0).sum())
        seen["negative"] += int((d < 0).sum())
        with np.errstate(invalid="ignore"):
            seen["beyond"] += int((d - zc < -S["trunc"]).sum())
        if fr["pixel_weight"] is not None:
            a = fr["pixel_weight"][py, px]
            seen["weight"] += int(((a == 0) | ~np.isfinite(a)).sum())
    assert all(v > 0 for v in seen.values()), seen


def test_fused_scene_float32_against_float64(frames):
    """what the number format alone costs on the scene of the GPU tests (the figures quoted at the top of tests/test_fusion_gpu.py)"""
    S = FR.SCENE
    o, vx, tr = np.float32(S["origin"]), np.float32(S["voxel"]), np.float32(S["trunc"])
    for path in ("depth", "pts"):
        fr = FR.as_path(frames, path)
        a = FR.integrate_ref(*FR.empty_volume(S["dims"]), fr, o, vx, tr, np.float32)
        b = FR.integrate_ref(*FR.empty_volume(S["dims"]), fr, o, vx, tr, np.float64)
        same = np.abs(a[1] - b[1]) < 1e-3                   # voxels whose every decision fell the same way in both formats
        assert same.mean() > 0.97
        assert np.abs(a[0] - b[0])[same].max() < 1e-4
        print(path, "tsdf fp32 vs float64: max abs", np.abs(a[0] - b[0])[same].max(), "weights equal at", same.mean())


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_without_a_device():
    from spann3r_amd import fusion as F
    with pytest.raises(ValueError, match="over the index limit"):
        F.TSDFVolume((0, 0, 0), 0.01, (1024, 1024, 512))
    with pytest.raises(ValueError, match="three sizes"):
        F.TSDFVolume((0, 0, 0), 0.01, (8, 8))
    with pytest.raises(ValueError, match="voxel_size"):
        F.TSDFVolume((0, 0, 0), 0.0, (8, 8, 8))
    with pytest.raises(ValueError, match="trunc"):
        F.TSDFVolume((0, 0, 0), 0.1, (8, 8, 8), trunc=-1.0)
    with pytest.raises(ValueError, match="origin"):
        F.TSDFVolume((0, np.nan, 0), 0.1, (8, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.TSDFVolume((0, 0, 0), 0.1, (8, 8, 8), device="cpu")
    K, P = np.array([[50.0, 0, 16], [0, 50, 12], [0, 0, 1]]), np.eye(4)
    fk, w2c = F.camera_tables(K, [P, FR.look_at((1, 2, 3), (0, 0, 0))], 2)
    assert fk.shape == (2, 4) and w2c.shape == (2, 12) and w2c.dtype == np.float32
    assert np.allclose(w2c[1].reshape(3, 4), np.linalg.inv(FR.look_at((1, 2, 3), (0, 0, 0)))[:3], atol=1e-6)
    Ks = K.copy()
    Ks[0, 1] = 0.5
    with pytest.raises(ValueError, match="skew"):
        F.camera_tables(Ks, [P], 1)
    Pn = P.copy()
    Pn[1, 3] = np.inf
    with pytest.raises(ValueError, match="finite 4x4"):
        F.camera_tables(K, [Pn], 1)
    with pytest.raises(ValueError, match="singular"):
        F.camera_tables(K, [np.zeros((4, 4))], 1)
    with pytest.raises(ValueError, match="must be"):
        F.camera_tables(K, [P, P, P], 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F._frames_list(torch.zeros(2, 4, 4), "depth", ())
    with pytest.raises(TypeError, match="expected a CUDA tensor"):
        F._frames_list([np.zeros((4, 4))], "depth", ())
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.fuse_views([dict(depthmap=torch.zeros(1, 4, 4))])
    with pytest.raises(ValueError, match="no views"):
        F.fuse_views([])
