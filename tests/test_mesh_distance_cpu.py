"""tests/mesh_distance_ref.py, the numpy restatement of include/spann3r_hip.h "Mesh distance", checked without a GPU: against a
second formulation in exact rationals, against a pair-by-pair loop over Python floats, and for the rule of the minimum (ties, faces
that must never win, queries that have no winner)."""
import numpy as np
import pytest

import mesh_distance_ref as R

N_PAIRS = 4000


@pytest.fixture(scope="module")
def pairs():
    """4000 random fp32 (triangle, point) pairs, seed 0: a quarter of the triangles are slivers (the third vertex within 1e-3 of an
    edge of length ~1), the queries are spread at 0.3 / 1 / 3 times the triangles' own scale"""
    rng = np.random.default_rng(0)
    a, b, c = (rng.normal(size=(N_PAIRS, 3)) for _ in range(3))
    sliver = np.arange(N_PAIRS) % 4 == 0
    t = rng.random((N_PAIRS, 1))
    c = np.where(sliver[:, None], a + t * (b - a) + 1e-3 * rng.uniform(-1, 1, (N_PAIRS, 3)), c)
    scale = np.array([0.3, 1.0, 3.0])[rng.integers(0, 3, N_PAIRS)][:, None]
    centre = (a + b + c) / 3
    p = centre + scale * rng.normal(size=(N_PAIRS, 3))
    return tuple(x.astype(np.float32) for x in (p, a, b, c)) + (sliver,)


def test_the_restatement_against_exact_rationals(pairs):
    """The relative error of d2 against the rational formulation on the fixed scene.  Measured: 3.4e-13 at most over the 4000 pairs
    (slivers 2.1e-15, the others 3.4e-13: the maximum belongs to a query 1.7e-4 from its face, where the 1e-16 of the fp64 closest point
    weighs most; an earlier prototype of this comparison had 1.8e-14 on another draw); the bar is 4x the measured maximum, the
    margin for another libm / numpy build.  All seven regions occur (401 / 396 / 747 / 263 / 576 / 627 / 990 pairs)."""
    p, a, b, c, sliver = pairs
    d2, q, region = R.closest_pairs(p, a, b, c)
    assert sorted(np.unique(region).tolist()) == list(range(7)), np.bincount(region, minlength=7)
    exact = [R.exact_d2(p[i], a[i], b[i], c[i]) for i in range(N_PAIRS)]
    rel = np.array([abs(float((R.Fraction(float(d2[i])) - exact[i]) / exact[i])) for i in range(N_PAIRS)])
    print("regions", np.bincount(region, minlength=7).tolist(), "max rel error of d2: all %.3e slivers %.3e others %.3e"
          % (rel.max(), rel[sliver].max(), rel[~sliver].max()))
    assert rel.max() <= 4 * 3.4e-13
    # the closest point lies where the distance says: |p - q|^2 recomputed from the fp64 q is the d2 returned, bit for bit
    d = p.astype(np.float64) - q
    assert np.array_equal((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], d2)


def test_the_vectorised_form_equals_the_pair_by_pair_loop(pairs):
    p, a, b, c, _ = pairs
    d2, q, region = R.closest_pairs(p, a, b, c)
    for i in range(N_PAIRS):
        ld2, lq, lr = R.closest_pair_loop(p[i], a[i], b[i], c[i])
        assert np.float64(ld2).view(np.uint64) == d2[i].view(np.uint64) and lr == region[i], i
        assert np.array_equal(np.array(lq, np.float64).view(np.uint64), q[i].view(np.uint64)), i


def test_ties_unusable_faces_and_queries_without_a_winner():
    verts = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, -3, 0), (2, 4, 6), (1, 2, 3), (3, 6, 9), (np.nan, 0, 0), (np.inf, 1, 1), (5, 5, 5)],
                     np.float32)
    good = [0, 1, 2]
    # unusable ones first and all of them nearer to the queries' side than they have any right to be
    faces = np.array([[4, 5, 6], [0, 0, 1], [-1, 1, 2], [0, 1, 10], [7, 1, 2], [8, 1, 2], [0, 1, 2 ** 31 - 1], good, [0, 1, 3], good, [2, 0, 1]],
                     np.int32)
    use = R.usable(verts, faces)
    assert use.tolist() == [False] * 7 + [True] * 4
    q = np.array([(0.25, 0.25, 0.5), (0.25, 0.25, 0.0), (-1, 0, 0), (2, 4, -6), (np.nan, 0, 0), (np.inf, 0, 0), (0.5, 0, 0)], np.float32)
    r = R.query(q, verts, faces)
    assert r["face"].tolist() == [7, 7, 7, 7, -1, -1, 7]                            # two copies and a rotation of one face: the smallest index
    assert r["region"].tolist() == [6, 6, 0, 3, 255, 255, 2]
    assert r["dist"][:3].tolist() == [0.5, 0.0, 1.0] and np.isinf(r["dist"][4:6]).all()
    assert np.array_equal(r["closest"][4:6].view(np.uint32), q[4:6].view(np.uint32))   # no winner: the query itself
    assert r["dist"][6] == 0.0 and r["closest"][6].tolist() == [0.5, 0, 0]
    # without the usable faces nothing wins
    none = R.query(q, verts, faces[:7])
    assert (none["face"] == -1).all() and (none["region"] == 255).all() and np.isinf(none["dist"]).all()
    assert np.array_equal(none["closest"].view(np.uint32), q.view(np.uint32))
    # permuting the faces leaves d2 alone
    perm = np.random.default_rng(1).permutation(len(faces))
    rp = R.query(q, verts, faces[perm])
    assert np.array_equal(rp["d2"], r["d2"]) and np.array_equal(rp["dist"].view(np.uint32), r["dist"].view(np.uint32))
    assert R.query(np.zeros((0, 3), np.float32), verts, faces)["dist"].shape == (0,)
