"""tests/mesh_ray_ref.py, the numpy restatement of include/spann3r_hip.h "Mesh rays", checked without a GPU: against a second
formulation in exact rationals (Moeller-Trumbore on the fp32 inputs), against a pair-by-pair loop over Python floats (bit for bit),
for watertightness on the icosphere, for exact depths on a tessellated plane, and the camera rule of mesh.render_depth_maps with the
refusals it shares with fusion.camera_tables."""
import math
from fractions import Fraction

import numpy as np
import pytest

import mesh_ray_ref as R

N_PAIRS = 4000
EPS_BARY = Fraction(1, 2 ** 40)
# the largest relative error of t against the rational value over the pairs both call a hit, measured by this test (it prints it):
# 9.87e-13 over the 1 999 exact hits of this input set (slivers and grazing rays lose the digits their small det costs).  The bar
# is four times that, the margin tests/test_mesh_distance_cpu.py gives d2.
T_REL_MEASURED = 9.87e-13
T_REL_BAR = 4 * T_REL_MEASURED


def _pairs(seed=11):
    """4 000 (ray, triangle) pairs, fp32: [0, 1000) slivers, [1000, 2000) grazing rays (|cos| < 1e-3 to the plane), the rest general;
    every second one is aimed inside the triangle, the others past an edge"""
    rng = np.random.default_rng(seed)
    n = N_PAIRS
    a = rng.uniform(-1, 1, (n, 3))
    b = rng.uniform(-1, 1, (n, 3))
    c = rng.uniform(-1, 1, (n, 3))
    sl = slice(0, n // 4)                                          # slivers: C a hair off the line AB
    s = rng.uniform(0.1, 0.9, (n // 4, 1))
    c[sl] = a[sl] + s * (b[sl] - a[sl]) + 1e-4 * rng.normal(size=(n // 4, 3))
    a, b, c = (x.astype(np.float32).astype(np.float64) for x in (a, b, c))
    w = rng.dirichlet((1, 1, 1), n)
    out = np.arange(n) % 2 == 1                                    # aimed outside: one weight negative
    k = rng.integers(0, 3, n)
    rows = np.flatnonzero(out)
    neg = rng.uniform(0.02, 1.0, len(rows))
    w[rows, (k[rows] + 1) % 3] += w[rows, k[rows]] + neg           # (the weights still sum to one)
    w[rows, k[rows]] = -neg
    target = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tan = b - a
    tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    cosang = rng.uniform(0.2, 1.0, n) * rng.choice([-1.0, 1.0], n)
    gz = slice(n // 4, n // 2)
    cosang[gz] = rng.uniform(1e-5, 9e-4, n // 4) * rng.choice([-1.0, 1.0], n // 4)
    rot = np.cross(nrm, tan)
    phi = rng.uniform(0, 2 * np.pi, (n, 1))
    inplane = np.cos(phi) * tan + np.sin(phi) * rot
    direction = cosang[:, None] * nrm + np.sqrt(1 - cosang[:, None] ** 2) * inplane
    dist = rng.uniform(0.5, 3.0, (n, 1))
    o = (target - dist * direction).astype(np.float32)
    d = (direction * rng.uniform(0.1, 10.0, (n, 1))).astype(np.float32)
    return o, d, a.astype(np.float32), b.astype(np.float32), c.astype(np.float32)


@pytest.fixture(scope="module")
def pairs():
    o, d, a, b, c = _pairs()
    return o, d, a, b, c, R.hit_pairs(o, d, a, b, c)


def test_hit_or_miss_and_t_against_exact_rationals(pairs):
    o, d, a, b, c, r = pairs
    between = hits = misses = 0
    worst = 0.0
    grazing = 0
    for i in range(N_PAIRS):
        ex = R.exact_hit(o[i], d[i], a[i], b[i], c[i])
        if i in range(N_PAIRS // 4, N_PAIRS // 2):
            dd, nn = d[i].astype(np.float64), np.cross(b[i].astype(np.float64) - a[i], c[i].astype(np.float64) - a[i])
            grazing += abs(dd @ nn) / (np.linalg.norm(dd) * np.linalg.norm(nn)) < 1e-3
        if ex is None:
            between += 1
            continue
        t, w = ex
        assert t > 0                                               # every ray starts in front of its plane: the range never decides
        if all(x >= EPS_BARY for x in w):
            hits += 1
            assert r["hit"][i], "pair %d: exactly inside (weights %s) but the rule misses" % (i, [float(x) for x in w])
            rel = abs(Fraction(float(r["t"][i])) - t) / t
            worst = max(worst, float(rel))
        elif any(x <= -EPS_BARY for x in w):
            misses += 1
            assert not r["hit"][i], "pair %d: exactly outside (weights %s) but the rule hits" % (i, [float(x) for x in w])
        else:
            between += 1
    print("pairs: %d hits, %d misses, %d between; grazing %d; largest relative error of t %.3e (bar %.3e)" %
          (hits, misses, between, grazing, worst, T_REL_BAR))
    assert between <= N_PAIRS // 100
    assert grazing == N_PAIRS // 4
    assert 0.4 * N_PAIRS <= hits <= 0.6 * N_PAIRS and 0.4 * N_PAIRS <= misses <= 0.6 * N_PAIRS
    assert worst <= T_REL_BAR


def test_the_restatement_equals_a_loop_over_python_floats(pairs):
    o, d, a, b, c, r = pairs
    bits = lambda x: np.float64(x).view(np.uint64)
    for i in range(N_PAIRS):
        hit, t, uvw, det = R.hit_pair_loop(o[i], d[i], a[i], b[i], c[i])
        assert hit == bool(r["hit"][i]), i
        assert all(bits(uvw[k]) == bits(r[n][i]) for k, n in enumerate("UVW")), i
        if hit:
            assert bits(t) == bits(r["t"][i]) and bits(det) == bits(r["det"][i]), i


def test_special_rays_of_the_restatement():
    a, b, c = (0, 0, 1), (1, 0, 1), (0, 1, 1)
    for o, d in (((np.nan, 0, 0), (0, 0, 1)), ((0.2, 0.2, 0), (0, 0, 0)), ((0.2, 0.2, 0), (0, np.inf, 1)), ((0.2, np.inf, 0), (0, 0, 1))):
        assert not R.hit_pairs(np.array(o, np.float32), np.array(d, np.float32), a, b, c)["hit"]
        assert not R.hit_pair_loop(o, d, a, b, c)[0]
    # side: seen from z < 1 along +z the face (normal +z) shows its back; from above, its front
    below = R.hit_pairs((0.2, 0.2, 0), (0, 0, 1), a, b, c)
    above = R.hit_pairs((0.2, 0.2, 3), (0, 0, -2), a, b, c)
    assert below["hit"] and below["det"] < 0 and below["t"] == 1.0 and above["hit"] and above["det"] > 0 and above["t"] == 1.0
    assert not R.hit_pairs((0.2, 0.2, 0), (0, 0, 1), a, b, c, cull="back")["hit"] and R.hit_pairs((0.2, 0.2, 0), (0, 0, 1), a, b, c, cull="front")["hit"]
    assert R.hit_pairs((0.2, 0.2, 3), (0, 0, -2), a, b, c, cull="back")["hit"] and not R.hit_pairs((0.2, 0.2, 3), (0, 0, -2), a, b, c, cull="front")["hit"]
    # the range cuts on either end and holds exactly at the hit; a start on the face gives +0
    assert R.hit_pairs((0.2, 0.2, 0), (0, 0, 1), a, b, c, 1.0, 1.0)["hit"]
    assert not R.hit_pairs((0.2, 0.2, 0), (0, 0, 1), a, b, c, 0.0, 0.999)["hit"] and not R.hit_pairs((0.2, 0.2, 0), (0, 0, 1), a, b, c, 1.001, 9.0)["hit"]
    on = R.hit_pairs((0.2, 0.2, 1), (0, 0, -1), a, b, c)
    assert on["hit"] and on["t"] == 0 and not np.signbit(on["t"])
    # in the plane: U = V = W = 0, det = 0, a miss
    assert not R.hit_pairs((-1, 0.2, 1), (1, 0, 0), a, b, c)["hit"]


def test_the_icosphere_is_watertight_from_inside():
    verts, faces = R.icosphere(3)
    assert verts.shape == (642, 3) and faces.shape == (1280, 3)
    lo, hi = R.sphere_radial_bounds(verts, faces)
    assert 1 - lo < 0.005
    total = 0
    for origin in R.SPHERE_ORIGINS:
        o, d = R.sphere_rays(verts, faces, origin)
        assert len(d) == 642 + 1920 + 1280 + 2048
        r = R.intersect(o, d, verts, faces)
        total += len(d)
        assert (r["face"] >= 0).all(), "%d rays pass through the closed surface" % (r["face"] < 0).sum()
        p = o.astype(np.float64) + r["t64"][:, None] * d.astype(np.float64)
        rad = np.linalg.norm(p, axis=1)
        assert rad.min() >= lo - 1e-12 and rad.max() <= hi + 1e-12
        if origin == R.SPHERE_ORIGINS[0]:                            # from the centre the radius of the hit IS t |d|
            td = r["t64"] * np.linalg.norm(d.astype(np.float64), axis=1)
            assert td.min() >= lo - 1e-12 and td.max() <= hi + 1e-12
        assert (r["side"] == 1).all()                              # from inside, an outward-facing surface shows its back
    print("icosphere: 0 misses over %d rays" % total)


def test_the_plane_gives_its_depth_exactly():
    verts, faces = R.plane(9, 2.0)
    assert len(faces) == 128
    o, d = R.camera_rays(np.array([[14.0, 0, 10], [0, 14.0, 10], [0, 0, 1]]), np.eye(4), (21, 21))
    assert len(d) == 441 and (d[:, 2] == 1).all() and np.abs(d[:, :2]).max() < 0.75
    r = R.intersect(o, d, verts, faces)
    assert (r["face"] >= 0).all() and (r["t64"] == 2.0).all() and (r["t"] == 2.0).all() and (r["point"][:, 2] == 2.0).all()


def test_the_camera_rule():
    K = np.array([[100.5, 0, 31.25], [0, 99.75, 23.5], [0, 0, 1]])
    ang = 0.3
    P = np.eye(4)
    P[:3, :3] = np.array([[math.cos(ang), 0, math.sin(ang)], [0, 1, 0], [-math.sin(ang), 0, math.cos(ang)]])
    P[:3, 3] = (0.5, -1.0, 2.0)
    o, d = R.camera_rays(K, P, (5, 7), 0.5)
    assert o.dtype == np.float32 and d.dtype == np.float32 and o.shape == d.shape == (35, 3)
    assert (o == np.float32(P[:3, 3])).all()
    v, u = 3, 4                                                     # row-major: pixel (u, v) is ray v w + u
    cam = np.array([((u + 0.5) - 31.25) / 100.5, ((v + 0.5) - 23.5) / 99.75, 1.0])
    want = P[:3, :3].astype(np.float32).astype(np.float64) @ cam
    assert np.abs(d[v * 7 + u] - want).max() <= 2.0 ** -23
    # pixel centres at integer coordinates: the principal point's pixel looks down the optical axis
    o, d = R.camera_rays(np.array([[50.0, 0, 3], [0, 50.0, 2], [0, 0, 1]]), np.eye(4), (5, 7))
    assert d[2 * 7 + 3].tolist() == [0.0, 0.0, 1.0]


def test_render_depth_maps_refuses_what_camera_tables_refuses():
    from spann3r_amd import mesh as M
    from spann3r_amd.fusion import camera_tables
    K, P = np.array([[50.0, 0, 3], [0, 50.0, 2], [0, 0, 1]]), np.eye(4)
    skew = K.copy()
    skew[0, 1] = 0.1
    sing = P.copy()
    sing[2, 2] = 0.0
    nonf = P.copy()
    nonf[0, 3] = np.nan
    for k, p, msg in ((skew, P, "skew"), (K, sing, "singular"), (K, nonf, "finite")):
        with pytest.raises(ValueError, match=msg):
            camera_tables(k, p[None], 1)
        with pytest.raises(ValueError, match=msg):
            M.render_depth_maps(None, k, p, (4, 4))                 # refused before the mesh is looked at
    zero = K.copy()
    zero[0, 0] = 0.0
    with pytest.raises(ValueError, match="focal"):
        M.render_depth_maps(None, zero, P, (4, 4))
    with pytest.raises(ValueError, match="near"):
        M.render_depth_maps(None, K, P, (4, 4), near=2.0, far=1.0)
    with pytest.raises(ValueError, match="size"):
        M.render_depth_maps(None, K, P, (0, 4))
    with pytest.raises(ValueError, match="cam2world"):
        M.render_depth_maps(None, K, np.eye(3), (4, 4))
