"""tests/mesh_bvh_ref.py, the restatement of include/spann3r_hip.h "Mesh BVH", checked without a GPU:
- the level table and the boxes at the counts where the table changes shape;
- the property both walks stand on, on fixed pair sets: the bound of a face's OWN box (the tightest box above it, under the smallest
  slack a mesh holding it can have) never exceeds the evaluated d2 of mesh_distance_ref.closest_pairs, and the clipped range of the
  box holds the t of every hit of mesh_ray_ref.hit_pairs -- slivers, near contact and grazing rays included;
- both walks equal mesh_distance_ref.query / mesh_ray_ref.intersect bit for bit on the 32 x 32 bumpy sheet, and look at fewer than
  F / 8 faces per query doing so (the cap the device tests hold the kernels to)."""
import math

import numpy as np
import pytest

import mesh_bvh_ref as B
import mesh_distance_ref as DR
import mesh_ray_ref as RR


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------------------------------------ 1. the level table and the boxes
@pytest.mark.parametrize("usable", B.COUNTS)
def test_level_table_and_boxes(usable):
    from spann3r_amd import cell_grid as G
    verts, faces = RR.bumpy_sheet()
    assert len(faces) == 1922
    faces = faces[np.random.default_rng(usable).permutation(len(faces))[:usable]]
    sizes, offsets = B.level_table(usable)
    assert (G.BVH_LEAF, G.BVH_ARITY) == (B.LEAF, B.ARITY) and G.bvh_levels(usable) == (sizes, offsets)
    assert sizes[0] == -(-usable // B.LEAF) and sizes[-1] == 1 and all(sizes[l + 1] == -(-sizes[l] // B.ARITY) for l in range(len(sizes) - 1))
    assert all(n > 1 for n in sizes[:-1]) and offsets[0] == 0 and np.array_equal(np.diff(offsets), sizes) and len(sizes) <= 16
    assert len(sizes) == {1: 1, 4: 1, 5: 2, 16: 2, 17: 3, 65: 4, 1922: 6}[usable]
    tree = B.build(verts, faces)
    assert tree["usable"] == usable and sorted(tree["order"].tolist()) == list(range(usable)) and tree["levels"] == len(sizes)
    tri = verts[faces[tree["order"]]]
    for l, n in enumerate(sizes):
        span = B.LEAF * B.ARITY ** l
        for k in range(n):
            under = tri[k * span:(k + 1) * span].reshape(-1, 3)
            assert len(under) > 0                                                      # existence follows from the counts
            assert np.array_equal(tree["node_lo"][offsets[l] + k], under.min(0)) and np.array_equal(tree["node_hi"][offsets[l] + k], under.max(0))
    assert np.array_equal(tree["node_lo"][-1], verts[faces].reshape(-1, 3).min(0))


def test_keys_sort_faces_along_the_curve_and_mark_unusable_ones():
    verts = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1), (0, 0, 1), (np.nan, 0, 0)], np.float32)
    faces = np.array([(3, 2, 1), (0, 1, 2), (0, 0, 1), (0, 1, 5), (0, 1, 9), (0, 2, 4)], np.int32)
    keys = B.face_keys(verts, faces)
    assert (keys[[2, 3, 4]] == B.KEY_NONE).all() and (keys[[0, 1, 5]] < B.KEY_NONE - 1).all() and keys[1] < keys[0]
    box = B.finite_box(verts)
    pk = B.point_keys(np.array([(0, 0, 0), (1, 1, 1), (5, 5, 5), (-3, 0, 0), (np.inf, 0, 0)], np.float32), box)
    assert pk[0] == 0 and pk[4] == B.KEY_NONE and pk[1] == pk[2] == 2 ** 63 - 2 and pk[3] == 0      # clamped into the box
    flat = B.point_keys(np.array([(0.5, 0.25, 7)], np.float32), np.array([(0, 0, 7), (1, 1, 7.0)]))
    assert flat[0] < 2 ** 62 and flat[0] & 0x4924924924924924 == 0                     # an axis of no extent contributes 0


# ------------------------------------------------------------------------------------------------ 2. the bound property
def _pair_faces(rng, n):
    """n triangles of sizes 1e-3 .. 1e2 centred up to 1e2 from the origin, every fourth a sliver (height 1e-6 .. 1e-3 of its length)"""
    size = 10.0 ** rng.uniform(-3, 2, (n, 1))
    centre = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-2, 2, (n, 1))
    tri = centre[:, None] + rng.normal(size=(n, 3, 3)) * size[:, None]
    s = np.arange(n) % 4 == 0
    t = rng.uniform(0.1, 0.9, (n, 1))
    thin = tri[:, 0] + t * (tri[:, 1] - tri[:, 0]) + rng.normal(size=(n, 3)) * size * 10.0 ** rng.uniform(-6, -3, (n, 1))
    tri[s, 2] = thin[s]
    tri = tri.astype(np.float32)
    ok = DR.usable(tri.reshape(-1, 3), np.arange(3 * n).reshape(n, 3))
    return tri[ok], size[ok], s[ok]


def _own_box(tri):
    """the fp32 box of every face and the smallest slack a mesh that holds it can have (the face alone)"""
    lo, hi = tri.min(1), tri.max(1)
    slack = np.array([B.slack_of(np.stack([l, h]).astype(np.float64)) for l, h in zip(lo, hi)])
    return lo, hi, slack


def test_the_distance_bound_of_a_faces_own_box_never_exceeds_its_d2():
    rng = np.random.default_rng(11)
    tri, size, sliver = _pair_faces(rng, 6000)
    n = len(tri)
    assert n >= 4000 and sliver.sum() >= n // 5
    w = rng.dirichlet((1, 1, 1), n)
    w[::7] = np.eye(3)[rng.integers(0, 3, len(w[::7]))]                                 # at a corner
    w[1::7, 0] = 0
    w[1::7] /= w[1::7].sum(1, keepdims=True)                                           # on an edge
    on = (tri.astype(np.float64) * w[:, :, None]).sum(1)
    away = rng.normal(size=(n, 3))
    away[2::5] = np.eye(3)[rng.integers(0, 3, len(away[2::5]))] * rng.choice([-1.0, 1.0], (len(away[2::5]), 1))      # along an axis: off a box face
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    reach = 10.0 ** rng.uniform(-7, 3, (n, 1))
    q = (on + away * size * reach).astype(np.float32)
    lo, hi, slack = _own_box(tri)
    d2 = DR.closest_pairs(q.astype(np.float64), *(tri[:, k].astype(np.float64) for k in range(3)))[0]
    lb = B.dist_bound(lo, hi, q.astype(np.float64), slack)
    assert np.isfinite(d2).all() and (lb >= 0).all()
    far = lb > 0
    print("distance bound: %d pairs (%d slivers), %d with lb > 0, largest lb / d2 %.12f, reach %.1e .. %.1e face sizes" %
          (n, sliver.sum(), far.sum(), (lb[far] / d2[far]).max(), reach.min(), reach.max()))
    assert far.sum() > n // 4 and (~far).sum() > 100                                   # (a query beside the box, and one in it: lb = 0)
    bad = np.flatnonzero(lb > d2)
    assert len(bad) == 0, "pair %d: lb %r > d2 %r" % (bad[0], lb[bad[0]], d2[bad[0]])


def test_the_clipped_range_of_a_faces_own_box_holds_every_hit():
    rng = np.random.default_rng(12)
    tri, size, sliver = _pair_faces(rng, 6000)
    n = len(tri)
    w = rng.dirichlet((1, 1, 1), n)
    w[::7] = np.eye(3)[rng.integers(0, 3, len(w[::7]))]
    w[1::7, 0] = 0
    w[1::7] /= w[1::7].sum(1, keepdims=True)
    t64 = tri.astype(np.float64)
    target = (t64 * w[:, :, None]).sum(1)
    normal = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    along = t64[:, 1] - t64[:, 0]
    along /= np.linalg.norm(along, axis=1, keepdims=True)
    # every third ray grazes: 1e-6 .. 1e-2 rad off the face's plane; the others come from anywhere
    graze = np.arange(n) % 3 == 0
    angle = 10.0 ** rng.uniform(-6, -2, (n, 1))
    back = np.where(graze[:, None], along * np.cos(angle) + normal * np.sin(angle), rng.normal(size=(n, 3)))
    back /= np.linalg.norm(back, axis=1, keepdims=True)
    o = (target + back * size * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)
    d = ((target - o.astype(np.float64)) * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)
    d[5::11, 0] = 0                                                                    # a zero component: a test of o on that axis
    r = RR.hit_pairs(o.astype(np.float64), d.astype(np.float64), *(t64[:, k] for k in range(3)))
    hit = r["hit"]
    lo, hi, slack = _own_box(tri)
    ok, t0, t1 = B.ray_clip(lo, hi, o.astype(np.float64), d.astype(np.float64), slack)
    print("ray clip: %d pairs, %d hits (%d grazing, %d on slivers, %d with a zero component)" %
          (n, hit.sum(), (hit & graze).sum(), (hit & sliver).sum(), (hit & (d == 0).any(1)).sum()))
    assert hit.sum() >= 4000 and (hit & graze).sum() > 500 and (hit & sliver).sum() > 300 and (hit & (d == 0).any(1)).sum() > 50
    bad = np.flatnonzero(hit & ~(ok & (t0 <= r["t"]) & (r["t"] <= t1)))
    assert len(bad) == 0, "pair %d: t %r outside [%r, %r] (clip %s)" % (bad[0], r["t"][bad[0]], t0[bad[0]], t1[bad[0]], ok[bad[0]])
    # a range that ends exactly at the hit keeps it
    ok2, a2, b2 = B.ray_clip(lo[hit], hi[hit], o[hit].astype(np.float64), d[hit].astype(np.float64), slack[hit], t_min=0.0, t_max=1e300)
    assert ok2.all()


# ------------------------------------------------------------------------------------------------ 3. the walks on the bumpy sheet
@pytest.fixture(scope="module")
def sheet_tree():
    verts, faces = RR.bumpy_sheet()
    return verts, faces, B.build(verts, faces)


def sheet_queries():
    """256 near the sheet, 256 inside its box, 1024 outside it by up to 1000 extents, 64 broadside at z = 1000"""
    verts, faces = RR.bumpy_sheet()
    rng = np.random.default_rng(5)
    f = faces[rng.integers(0, len(faces), 256)]
    near = (verts[f] * rng.dirichlet((1, 1, 1), 256)[:, :, None]).sum(1) + rng.uniform(-0.005, 0.005, (256, 3))
    lo, hi = verts.min(0), verts.max(0)
    inside = rng.uniform(lo, hi, (256, 3))
    direction = rng.normal(size=(1024, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    outside = (lo + hi) / 2 + direction * (10.0 ** rng.uniform(0, 3, (1024, 1)))
    broad = np.concatenate([rng.uniform(lo, hi, (64, 3))[:, :2], np.full((64, 1), 1000.0)], 1)
    return np.concatenate([near, inside, outside, broad]).astype(np.float32)


def test_the_distance_walk_equals_the_rule_bit_for_bit(sheet_tree):
    verts, faces, tree = sheet_tree
    q = np.concatenate([sheet_queries(), [(np.nan, 0, 0), (0, np.inf, 0)]]).astype(np.float32)
    want = DR.query(q, verts, faces)
    got = B.dist_query(q, tree)
    assert np.array_equal(got["face"], want["face"]) and np.array_equal(got["region"], want["region"])
    assert np.array_equal(_bits(got["d2"]), _bits(want["d2"])) and np.array_equal(_bits(got["dist"]), _bits(want["dist"]))
    assert np.array_equal(_bits(got["closest"]), _bits(want["closest"]))
    assert (got["evals"][-2:] == 0).all() and (got["nodes"][-2:] == 0).all() and (want["face"][-2:] == -1).all()
    F = len(faces)
    for name, s in (("near", slice(0, 256)), ("inside", slice(256, 512)), ("outside", slice(512, 1536)), ("broadside", slice(1536, 1600))):
        e = got["evals"][s]
        print("%-9s %4d queries: %.1f faces evaluated per query (max %d), %.1f nodes visited" % (name, len(e), e.mean(), e.max(), got["nodes"][s].mean()))
        assert e.sum() <= len(e) * F // 8 and (e >= 1).all()


def test_the_ray_walk_equals_the_rule_bit_for_bit(sheet_tree):
    verts, faces, tree = sheet_tree
    rng = np.random.default_rng(7)
    lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
    centre = (lo + hi) / 2
    dirs = rng.normal(size=(256, 3))
    out_o = centre + 3 * dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    rays = [(out_o, rng.uniform(lo, hi, (256, 3)) - out_o)]                            # from outside the box, towards it
    in_o = rng.uniform(lo, hi, (256, 3))
    rays.append((in_o, rng.normal(size=(256, 3))))                                     # from inside, pointing out
    zo = rng.uniform(lo, hi, (128, 3)) + (0, 0, 0.3)
    zd = rng.normal(size=(128, 3))
    zd[:64, 0] = 0
    zd[64:, :2] = 0                                                                    # zero components
    rays.append((zo, zd))
    rays.append(RR.camera_rays(np.array([[30.0, 0, 7.5], [0, 30.0, 7.5], [0, 0, 1]]), np.array([[1.0, 0, 0, 0.5], [0, -1, 0, 0.1], [0, 0, -1, 0.9], [0, 0, 0, 1]]),
                               (16, 16)))
    miss_o = np.tile(hi + (1.0, 0, 0), (32, 1))
    rays.append((miss_o, np.abs(rng.normal(size=(32, 3))) * (1, 1, 1)))                # beyond the box, pointing away: the root is never entered
    rays.append((np.array([(np.nan, 0, 0), (0.5, 0, 0.5), (0.5, 0, 0.5)]), np.array([(0, 0, -1), (0, 0, 0), (0, np.inf, -1)])))
    o = np.concatenate([np.asarray(r[0], np.float64) for r in rays]).astype(np.float32)
    d = np.concatenate([np.asarray(r[1], np.float64) for r in rays]).astype(np.float32)
    F = len(faces)
    for kw in (dict(), dict(t_min=0.25, t_max=0.95, cull="back"), dict(cull="front")):
        want = RR.intersect(o, d, verts, faces, **kw)
        got = B.ray_query(o, d, tree, **kw)
        assert np.array_equal(got["face"], want["face"]) and np.array_equal(got["side"], want["side"]), kw
        for k in ("t", "bary", "point", "t64"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (kw, k)
        hits = int((want["face"] >= 0).sum())
        print("rays %s: %d of %d hit, %.1f faces evaluated per ray (max %d), %.1f nodes visited" %
              (kw, hits, len(o), got["evals"].mean(), got["evals"].max(), got["nodes"].mean()))
        assert hits > 100 and got["evals"].sum() <= len(o) * F // 8
        assert (got["evals"][-35:] == 0).all() and (got["nodes"][-35:] == 0).all() and (want["face"][-35:] == -1).all()
