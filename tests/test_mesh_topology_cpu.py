"""tests/mesh_topology_ref.py, the numpy restatement of "Mesh topology and smoothing" (include/spann3r_hip.h), against three
independent statements: fusion_ref.manifold_report (np.unique over rows), a dict-of-sets loop over Python integers for the adjacency
and a vertex-by-vertex loop over Python floats for one pass, bit for bit.  Then the properties that make the filter worth having,
as conditions on the restatement over seeded inputs: Taubin's filter removes noise without shrinking, a plain Laplacian shrinks,
a fixed rim stays where it is and a free one creeps inward.  No GPU."""
import numpy as np
import pytest

import fusion_ref as FR
import mesh_ray_ref as RR
import mesh_topology_ref as T


def _loop_topology(faces, nv):
    """the rule with Python integers: -> (rows: list of sorted neighbour lists, {(lo, hi): [half-edges, ascending]}, usable faces)"""
    rows, edges, usable = [set() for _ in range(nv)], {}, 0
    for fi, f in enumerate(np.asarray(faces).reshape(-1, 3).tolist()):
        if not all(0 <= i < nv for i in f) or len(set(f)) != 3:
            continue
        usable += 1
        for c in range(3):
            a, b = f[c], f[(c + 1) % 3]
            rows[a].add(b)
            rows[b].add(a)
            edges.setdefault((min(a, b), max(a, b)), []).append((3 * fi + c, a < b))
    return [sorted(r) for r in rows], edges, usable


def _assert_matches_the_loop(faces, nv):
    t = T.topology(faces, nv)
    rows, edges, usable = _loop_topology(faces, nv)
    off, nb = t["vertex_offsets"], t["vertex_neighbors"]
    assert off.dtype == nb.dtype == np.int32 and off.shape == (nv + 1,) and off[0] == 0 and off[-1] == len(nb) == 2 * len(edges)
    for v in range(nv):
        assert nb[off[v]:off[v + 1]].tolist() == rows[v], v
    keys = sorted(edges)
    assert t["edges"].tolist() == [list(k) for k in keys]
    boundary = np.zeros(nv, np.uint8)
    for e, k in enumerate(keys):
        hs = edges[k]
        got = t["half_edges"][t["edge_first"][e]:t["edge_first"][e + 1]].tolist()
        assert got == [h for h, _ in hs] and got == sorted(got)
        fwd = sum(f for _, f in hs)
        cls = 0 if len(hs) == 1 else 3 if len(hs) > 2 else 1 if fwd == 1 else 2
        assert (t["edge_uses"][e], t["edge_fwd"][e], t["edge_class"][e]) == (len(hs), fwd, cls)
        if cls == 0:
            boundary[list(k)] = 1
    assert np.array_equal(t["vertex_boundary"], boundary)
    r = t["report"]
    assert tuple(r) == T.REPORT_KEYS
    assert r["faces_usable"] == usable and r["faces_unusable"] == len(np.asarray(faces).reshape(-1, 3)) - usable
    assert r["edges"] == len(keys) and r["vertices_referenced"] == sum(1 for x in rows if x)
    assert r["boundary"] + r["interior"] + r["inconsistent"] + r["nonmanifold"] == r["edges"]
    return t


def _assert_matches_manifold_report(faces, nv):
    t, ref = T.topology(faces, nv), FR.manifold_report(faces)
    r = t["report"]
    assert np.array_equal(t["edges"][t["edge_class"] == 0], ref["boundary"])
    assert r["euler"] == ref["euler"] and r["closed"] == ref["closed"]
    assert (ref["bad"] == 0) == (r["inconsistent"] + r["nonmanifold"] == 0)
    return r


@pytest.fixture(scope="module")
def ico():
    return RR.icosphere(3)


@pytest.fixture(scope="module")
def scene_mesh():
    S = FR.SCENE
    fr = FR.as_path(FR.scene_frames(), "depth")
    tsdf, weight, rgb = FR.integrate_ref(*FR.empty_volume(S["dims"]), fr, np.float32(S["origin"]), np.float32(S["voxel"]), np.float32(S["trunc"]),
                                         np.float32)
    return FR.extract_ref(tsdf, weight, rgb, S["origin"], S["voxel"])


def test_the_report_agrees_with_manifold_report(ico, scene_mesh):
    verts, faces = ico
    r = _assert_matches_manifold_report(faces, len(verts))
    assert (r["edges"], r["interior"], r["euler"], r["closed"]) == (1920, 1920, 2, True) and len(verts) == 642 and len(faces) == 1280
    sv, sf = T.grid_sheet(17, 1.0 / 16)
    r = _assert_matches_manifold_report(sf, len(sv))
    assert (r["edges"], r["boundary"], r["euler"], r["closed"]) == (800, 64, 1, False)
    assert int(T.topology(sf, len(sv))["vertex_boundary"].sum()) == 64
    verts, _, faces = scene_mesh
    r = _assert_matches_manifold_report(faces, len(verts))
    assert r["faces_usable"] == len(faces) > 1000 and r["boundary"] > 0 and r["inconsistent"] + r["nonmanifold"] == 0


@pytest.mark.parametrize("name", sorted(T.SMALL))
def test_small_cases_against_the_loop(name):
    nv, faces = T.SMALL[name]
    t = _assert_matches_the_loop(faces, nv)
    r = t["report"]
    want = dict(triangle=dict(boundary=3, edges=3, euler=1), tetrahedron=dict(closed=True, edges=6, euler=2, interior=6),
                pair_consistent=dict(interior=1, boundary=4), pair_inconsistent=dict(inconsistent=1, boundary=4),
                duplicate=dict(inconsistent=3, edges=3), three_on_an_edge=dict(nonmanifold=1, boundary=6))[name]
    assert {k: r[k] for k in want} == want
    # unusable faces mixed in change nothing but their count and the numbering of the half-edges
    mixed, where = T.with_unusable(faces)
    tm = _assert_matches_the_loop(mixed, nv)
    assert tm["report"] == dict(r, faces_unusable=len(mixed) - len(faces))
    for k in T.TABLES:
        if k != "half_edges":
            assert np.array_equal(tm[k], t[k]), k
    assert np.array_equal(tm["half_edges"], 3 * where[t["half_edges"] // 3] + t["half_edges"] % 3)


def test_larger_cases_against_the_loop(ico):
    _assert_matches_the_loop(ico[1], 642)
    _assert_matches_the_loop(T.book(40, reverse_every=2), 45)
    rng = np.random.default_rng(3)
    _assert_matches_the_loop(rng.integers(-2, 40, (400, 3)), 37)                 # duplicates, repeats, out of range, every class
    fv, ff = T.closed_fan(50)
    t = _assert_matches_the_loop(ff, len(fv))
    assert t["report"]["boundary"] == 50 and np.diff(t["vertex_offsets"])[0] == 50
    for nv, faces in ((0, np.zeros((0, 3), np.int32)), (5, np.zeros((0, 3), np.int32)), (0, [(0, 1, 2)]), (3, [(0, 0, 1)])):
        t = _assert_matches_the_loop(faces, nv)
        assert t["report"]["edges"] == 0 and not t["report"]["closed"] and not t["vertex_offsets"].any()


def _loop_pass(p, rows, c, fixed=None):
    """one pass, vertex by vertex, with Python floats (IEEE doubles, every operation rounded on its own)"""
    out = p.copy()
    for v, row in enumerate(rows):
        if not row or (fixed is not None and fixed[v]):
            continue
        for a in range(3):
            s = float(p[row[0], a])
            for n in row[1:]:
                s = s + float(p[n, a])
            m = s / float(len(row))
            x = float(p[v, a])
            out[v, a] = np.float32(x + c * (m - x))
    return out


def test_one_pass_equals_the_vertex_loop_bit_for_bit(ico):
    rng = np.random.default_rng(5)
    cases = [(ico[0] * (1 + 0.02 * rng.uniform(-1, 1, (642, 1))), ico[1]), T.closed_fan(300)]
    sv, sf = T.grid_sheet(17, 1.0 / 16)
    cases.append((sv + rng.uniform(-0.02, 0.02, sv.shape), sf))
    for verts, faces in cases:
        p = np.ascontiguousarray(verts, np.float32)
        t = T.topology(faces, len(p))
        rows = _loop_topology(faces, len(p))[0]
        for c in (0.5, -0.53, 1.0 / 3.0):
            for fixed in (None, t["vertex_boundary"]):
                got = T.smooth_pass(p, t["vertex_offsets"], t["vertex_neighbors"], c, fixed)
                assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), _loop_pass(p, rows, c, fixed).view(np.uint32))
    # vertices without a row keep their bits, NaN included
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 7, -0.0]], np.float32)
    got = T.smooth_pass(p, *[T.topology([(0, 1, 2)], 4)[k] for k in ("vertex_offsets", "vertex_neighbors")], 0.5)
    assert np.array_equal(got[3].view(np.uint32), p[3].view(np.uint32)) and np.allclose(got[0], (0.25, 0.25, 0))


@pytest.mark.parametrize("amplitude, spread", [(0.01, 0.00572), (0.02, 0.01145)])
def test_taubin_removes_noise_without_shrinking_and_a_laplacian_shrinks(ico, amplitude, spread):
    verts, faces = ico
    u = np.random.default_rng(11).uniform(-1, 1, (len(verts), 1))
    noisy = (verts.astype(np.float64) * (1 + amplitude * u)).astype(np.float32)
    r0 = np.linalg.norm(noisy.astype(np.float64), axis=1)
    assert abs(r0.std() / spread - 1) < 0.05                                        # (the input is the one the figures were taken on, in size)
    r = np.linalg.norm(T.smooth(noisy, faces, 10).astype(np.float64), axis=1)
    assert r.std() <= 0.5 * r0.std(), (r0.std(), r.std())
    assert abs(r.mean() - 1) <= 0.01, r.mean()
    lap = np.linalg.norm(T.smooth(noisy, faces, 10, lam=0.5, mu=0.5).astype(np.float64), axis=1)
    assert lap.mean() < 0.95, lap.mean()


def test_a_fixed_rim_stays_and_a_free_one_creeps_inward():
    verts, faces = T.grid_sheet(17, 1.0 / 16)
    rng = np.random.default_rng(13)
    noisy = verts.copy()
    noisy[:, 2] = rng.uniform(-0.02, 0.02, len(verts)).astype(np.float32)
    t = T.topology(faces, len(verts))
    rim = t["vertex_boundary"] == 1
    assert rim.sum() == 64 and t["report"]["boundary"] == 64 and t["report"]["edges"] == 800
    fixed = T.smooth(noisy, faces, 10, boundary="fixed")
    assert np.array_equal(fixed[rim].view(np.uint32), noisy[rim].view(np.uint32))
    assert fixed[~rim, 2].std() <= 0.5 * noisy[~rim, 2].std(), (noisy[~rim, 2].std(), fixed[~rim, 2].std())
    free = T.smooth(noisy, faces, 10, boundary="free")
    assert free[:, 0].min() > 0.005 and noisy[:, 0].min() == 0, free[:, 0].min()
    assert np.array_equal(T.smooth(noisy, faces, 0).view(np.uint32), noisy.view(np.uint32))
    one = T.smooth(noisy, faces, 3, mu=0.0)
    ref = noisy
    for _ in range(3):
        ref = T.smooth_pass(ref, t["vertex_offsets"], t["vertex_neighbors"], 0.5, t["vertex_boundary"])
    assert np.array_equal(one.view(np.uint32), ref.view(np.uint32))
