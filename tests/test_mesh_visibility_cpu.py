"""tests/mesh_visibility_ref.py, the numpy restatement of include/spann3r_hip.h "Mesh visibility", on scenes whose answer geometry
gives: two triangles one in front of the other, the borders of a frustum as exact fp32 inputs, and the level-3 icosphere of the ray
tests seen from outside.  No GPU; tests/test_mesh_visibility_gpu.py runs the same list of cases through the kernels."""
import math

import numpy as np
import pytest

import mesh_ray_ref as R
import mesh_visibility_ref as V


def _case(prefix, **kw):
    hits = [c for c in V.cases() if c["name"].startswith(prefix) and all(c["kw"].get(k) == v for k, v in kw.items())]
    assert len(hits) == 1, (prefix, kw, [c["name"] for c in hits])
    return hits[0]


def test_two_triangles_are_seen_as_geometry_says():
    tt = V.two_triangles()
    n = len(tt["points"])
    got = V.run_case(_case("two triangles", cull=None, bias=1e-3))
    assert got["mask"].shape == (2, n + 6) and got["count"].dtype == np.int32
    assert np.array_equal(got["mask"][:, :n], tt["visible"]) and np.array_equal(got["count"], got["mask"].sum(0))
    # culling flips the cases: camera 0 sees only backs, camera 1 only fronts
    back = V.run_case(_case("two triangles", cull="back", bias=1e-3))["mask"][:, :n]
    front = V.run_case(_case("two triangles", cull="front", bias=1e-3))["mask"][:, :n]
    assert back[0].all() and np.array_equal(back[1], tt["visible"][1])            # backs ignored: nothing hides anything from camera 0
    assert front[1].all() and np.array_equal(front[0], tt["visible"][0])


def test_bias_drops_a_vertex_own_faces_and_nothing_else():
    tt = V.two_triangles()
    n = len(tt["points"])
    views = V.make_views(V.K32, tt["poses"], V.SIZE32)
    on_rear = tt["points"][4:5]                                                     # (0, 0, 4): on the large triangle, behind the small one
    for bias in (0.0, 1e-6, 1e-3, 0.1, 0.49):
        assert not V.point_visibility(on_rear, tt["vertices"], tt["faces"], views[:1], bias=bias)["mask"][0, 0], bias
    # the large triangle's own vertices: visible from both sides at the default, occluded by their own face at bias = 0
    default = V.run_case(_case("two triangles", cull=None, bias=1e-3))["mask"][:, n + 3:]
    zero = V.run_case(_case("two triangles", cull=None, bias=0.0))["mask"][:, n + 3:]
    assert default.all() and not zero.all()
    print("bias = 0: the large triangle's vertices seen per camera", zero.sum(1).tolist(), "of 3")
    assert not zero[1].any()              # camera 1 sees the face unobstructed, every operation is exact: each vertex hits itself at t = 1


@pytest.mark.parametrize("off", [0.0, 0.5])
def test_frustum_borders_as_exact_inputs(off):
    fb = V.frustum_border(off)
    got = V.run_case(_case("frustum borders", pixel_offset=off))
    assert np.array_equal(got["mask"][0], fb["visible"]), np.flatnonzero(got["mask"][0] != fb["visible"])
    view = V.make_views(V.BORDER_K, np.eye(4), V.BORDER_SIZE, near=V.BORDER_NEAR, far=V.BORDER_FAR)[0]
    pr = V.project(fb["points"][:2], view, off)
    assert pr["u"].tolist() == [off - 0.5, 8 + off - 0.5] and pr["in_image"].tolist() == [True, False] and pr["in_range"].all()


def test_per_ray_ranges_agree_with_the_closest_hit_restatement():
    """occluded() with one range per ray (hit_pairs ... any) against mesh_ray_ref.intersect, which takes one range for all"""
    verts, faces = R.bumpy_sheet(12)
    rng = np.random.default_rng(5)
    o = rng.uniform((0, -0.5, 0.3), (1, 0.5, 0.6), (96, 3)).astype(np.float32)
    d = (rng.uniform((0, -0.5, -0.3), (1, 0.5, -0.1), (96, 3)) - o).astype(np.float32)
    for t_min, t_max, cull in ((0.0, math.inf, None), (0.25, 0.75, None), (0.0, 0.999, "back"), (0.5, 0.5, "front")):
        want = R.intersect(o, d, verts, faces, t_min=t_min, t_max=t_max, cull=cull)["face"] >= 0
        assert np.array_equal(V.occluded(o, d, verts, faces, t_min, t_max, cull), want)
        assert np.array_equal(V.occluded(o, d, verts, faces, np.full(96, t_min), t_max, cull), want)
    assert not V.occluded(o, d, verts, faces, np.full(96, 0.8), 0.2).any() and not V.occluded(o, d, verts, faces, 0.8, 0.2).any()      # empty ranges
    bad = o.copy()
    bad[:4, 0] = np.nan
    zero = d.copy()
    zero[4:8] = 0
    assert not V.occluded(bad, zero, verts, faces)[:8].any()                        # a ray that is not ok is not occluded


@pytest.fixture(scope="module")
def sphere():
    verts, faces = R.icosphere(3)
    one = V.run_case(_case("icosphere, one camera"))
    six = V.run_case(_case("icosphere, six cameras"))
    return verts, faces, one, six


def test_the_icosphere_from_outside(sphere):
    verts, faces, one, six = sphere
    front, back = V.vertex_facing(verts, faces, V.SPHERE_EYE)
    vis = one["mask"][0]
    print("icosphere: %d vertices, %d with every face towards the camera, %d with every face away, %d mixed; %d visible" %
          (len(verts), front.sum(), back.sum(), (~front & ~back).sum(), vis.sum()))
    assert front.sum() > 100 and back.sum() > 100 and vis[front].all() and not vis[back].any()
    assert (six["count"] >= 1).all() and six["mask"].shape == (6, len(verts))


def test_cull_to_views_on_the_icosphere(sphere):
    verts, faces, one, six = sphere
    towards = V.facing(verts, faces, V.SPHERE_EYE) > 0
    kept = V.cull_to_views(verts, faces, one["count"], mode="all")
    # mode="all" keeps every face towards the camera and nothing whose vertices all lie beyond the silhouette.  "Only faces towards
    # the camera" holds except AT the silhouette: visibility is decided per vertex, a vertex of the convex sphere is seen iff one of
    # its faces looks at the camera, and a face that looks away next to the silhouette can have three such vertices (2 of the 426
    # kept here; 0 to 14 from other positions).  What geometry gives exactly is the set below.
    _, beyond = V.vertex_facing(verts, faces, V.SPHERE_EYE)
    assert np.array_equal(one["mask"][0], ~beyond)
    want = np.flatnonzero(~beyond[faces].any(1))
    is_kept = np.zeros(len(faces), bool)
    is_kept[kept["face_index"]] = True
    rim = is_kept & ~towards
    print("mode=all: %d faces kept, %d of them towards the camera (all %d such faces), %d look away at the silhouette" %
          (is_kept.sum(), (is_kept & towards).sum(), towards.sum(), rim.sum()))
    assert 0 < len(kept["face_index"]) < len(faces) and np.array_equal(kept["face_index"], want) and is_kept[towards].all()
    assert rim.sum() < towards.sum() // 10                                          # a rim, not a region
    assert np.array_equal(kept["vertices"][kept["faces"]], verts[faces[kept["face_index"]]])       # order, rotation and positions
    assert len(V.cull_to_views(verts, faces, one["count"], mode="any")["face_index"]) > len(kept["face_index"])
    whole = V.cull_to_views(verts, faces, six["count"])
    assert np.array_equal(whole["faces"], faces) and np.array_equal(whole["vertices"], verts)
    two = V.cull_to_views(verts, faces, six["count"], mode="all", min_views=2)
    assert 0 < len(two["face_index"]) < len(faces) and (six["count"][two["vertex_index"]] >= 2).all()
    # faces with an index out of range are dropped whatever the counts, and their vertices are never looked up
    broken = np.concatenate([faces[:4], [[0, 1, len(verts)], [-1, 2, 3]]]).astype(np.int32)
    assert V.cull_to_views(verts, broken, np.ones(len(verts), np.int32))["face_index"].tolist() == [0, 1, 2, 3]
    assert len(V.cull_to_views(verts, faces, np.zeros(len(verts), np.int32))["faces"]) == 0
