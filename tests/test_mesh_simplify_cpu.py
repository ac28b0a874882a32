"""tests/mesh_simplify_ref.py (the numpy restatement of include/spann3r_hip.h "Mesh simplification") against a second, independent
formulation -- a Python dict keyed by the cell tuple, looped vertex by vertex, with Python integers and struct-rounded floats -- and
against what a simplifier must give: representatives inside their cells, a cell below the vertex spacing changes no face, one huge
cell empties the mesh, a second pass on the same grid changes no face, and a permuted face list gives the same surface."""
import math
import struct

import numpy as np
import pytest

import mesh_simplify_ref as MS


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _loop_simplify(verts, rgba, faces, cell, origin, dedup=True):
    """the rule once more, one vertex and one face at a time"""
    cell, o = _f32(cell), [_f32(x) for x in origin]
    inv = float(np.float32(1) / np.float32(cell))
    groups, order, vc = {}, [], []
    for v, p in enumerate(np.asarray(verts, np.float32).tolist()):
        key, qs = [], []
        for a in range(3):
            with np.errstate(all="ignore"):
                u = float((np.float32(p[a]) - np.float32(o[a])) * np.float32(inv))
            if not math.isfinite(u) or abs(math.floor(u)) >= 2 ** 30:
                key = None
                break
            i = math.floor(u)
            r = float(np.float32(u) - np.float32(i))
            key.append(i)
            qs.append(min(int(r * 65536.0), 65535))
        if key is None:
            vc.append(-1)
            continue
        key = tuple(key)
        if key not in groups:                                    # first seen = smallest member: ids ascend with it
            groups[key] = dict(id=len(order), q=[0, 0, 0], c=[0, 0, 0, 0], n=0)
            order.append(key)
        g = groups[key]
        vc.append(g["id"])
        g["n"] += 1
        for a in range(3):
            g["q"][a] += qs[a]
        for k in range(4):
            g["c"][k] += (int(rgba[v]) >> (8 * k)) & 255
    pos, col = [], []
    for key in order:
        g = groups[key]
        pos.append([_f32(o[a] + (float(key[a]) + float(g["q"][a]) / float(g["n"]) / 65536.0) * cell) for a in range(3)])
        col.append(sum(((2 * g["c"][k] + g["n"]) // (2 * g["n"])) << (8 * k) for k in range(4)))
    kept, seen, counts = [], set(), dict(invalid=0, collapsed=0, duplicate=0)
    for f in np.asarray(faces).tolist():
        if any(not 0 <= x < len(vc) for x in f) or any(vc[x] < 0 for x in f):
            counts["invalid"] += 1
            continue
        t = [vc[x] for x in f]
        if len(set(t)) < 3:
            counts["collapsed"] += 1
            continue
        k = t.index(min(t))
        rot = (t[k], t[(k + 1) % 3], t[(k + 2) % 3])
        if dedup and rot in seen:
            counts["duplicate"] += 1
            continue
        seen.add(rot)
        kept.append(t)
    used = sorted({x for t in kept for x in t})
    new = {x: j for j, x in enumerate(used)}
    return (np.array([pos[x] for x in used], np.float32).reshape(-1, 3), np.array([col[x] for x in used], np.uint32),
            np.array([[new[x] for x in t] for t in kept], np.int32).reshape(-1, 3), counts, np.array(vc, np.int32), len(order))


def _random_mesh(seed, nv=300, nf=900, span=2.0):
    rng = np.random.default_rng(seed)
    verts = (rng.random((nv, 3)) * 2 * span - span).astype(np.float32)
    rgba = rng.integers(0, 2 ** 32, nv, dtype=np.uint32)
    faces = rng.integers(0, nv, (nf, 3)).astype(np.int32)
    return verts, rgba, faces


@pytest.mark.parametrize("seed,cell,origin,dedup", [(0, 1.0, (0, 0, 0), True), (1, 0.7, (0.13, -0.4, 2.5), True), (2, 1.3, (-5, 7, 0.001), False),
                                                    (3, 0.25, (0, 0, 0), True)])
def test_the_restatement_equals_the_vertex_by_vertex_loop(seed, cell, origin, dedup):
    verts, rgba, faces = _random_mesh(seed)
    verts[5], verts[17, 1], verts[40, 2] = np.nan, np.inf, np.float32(3e9)       # unusable: NaN, inf, beyond 2^30 cells
    verts[60] = np.asarray(origin, np.float32) + np.float32(cell) * np.float32(-2)  # exactly on a cell corner
    faces[7], faces[8] = (0, 1, 300), (-1, 2, 3)                                   # outside 0..V-1
    faces[9], faces[10], faces[11] = faces[12][[1, 2, 0]], faces[12][[2, 1, 0]], faces[12]      # a rotation, the mirror image, a copy
    v, c, f, stats, vc = MS.simplify(verts, rgba, faces, cell, origin, dedup)
    lv, lc, lf, counts, lvc, n = _loop_simplify(verts, rgba, faces, cell, origin, dedup)
    assert np.array_equal(vc, lvc) and stats["clusters"] == n and (vc[[5, 17, 40]] == -1).all() and vc[60] >= 0
    assert (stats["faces_invalid"], stats["faces_collapsed"], stats["faces_duplicate"]) == (counts["invalid"], counts["collapsed"], counts["duplicate"])
    assert stats["faces_invalid"] >= 2 and stats["faces_in"] == len(faces) == len(f) + sum(counts.values())
    assert f.shape == lf.shape and np.array_equal(f, lf)
    assert np.array_equal(v.view(np.uint32), lv.view(np.uint32)) and np.array_equal(c, lc)
    if not dedup:
        assert stats["faces_duplicate"] == 0


def test_the_sums_are_exact_beyond_32_bits():
    """100 000 vertices in one cell with q near 65 535: the sum of q exceeds 2^32; the mean and the colours are exact"""
    n = 100000
    rng = np.random.default_rng(4)
    verts = (np.float32(1) - rng.random((n, 3)).astype(np.float32) * np.float32(2.0 ** -12)).astype(np.float32)
    verts = np.minimum(verts, np.nextafter(np.float32(1), np.float32(0)))
    rgba = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    r = MS.cluster(verts, 1.0, rgba=rgba)
    i, q, ok = MS.cells(verts, 1.0)
    assert r["n_clusters"] == 1 and ok.all() and (i == 0).all() and q.min() > 65000 and int(q[:, 0].sum()) > 2 ** 32
    for a in range(3):
        want = _f32((0 + int(q[:, a].sum()) / n / 65536.0) * 1.0)
        assert r["positions"][0, a] == np.float32(want)
    want = sum(((2 * int(((rgba >> (8 * k)) & 255).sum()) + n) // (2 * n)) << (8 * k) for k in range(4))
    assert int(r["rgba"][0]) == want


def _sheet(n, step=0.1):
    """an n x n sheet z = 0.03 sin(x) in the first octant region around the origin, two faces per cell"""
    y, x = np.mgrid[:n, :n]
    verts = np.stack([(x - n / 2 + 0.25) * step, (y - n / 2 + 0.25) * step, 0.03 * np.sin(x * step)], -1).reshape(-1, 3).astype(np.float32)
    tl = (y[:-1, :-1] * n + x[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([tl, tl + 1, tl + n], 1), np.stack([tl + 1, tl + n, tl + n + 1], 1)]).astype(np.int32)
    rgba = (np.arange(n * n, dtype=np.uint32) * np.uint32(2654435761)).astype(np.uint32)
    return verts, rgba, faces


@pytest.mark.parametrize("cell,origin", [(0.31, (0, 0, 0)), (1.0, (0.05, 0.02, -0.3)), (0.07, (1, 2, 3))])
def test_every_representative_lies_in_the_closed_box_of_its_cell(cell, origin):
    verts, rgba, _ = _sheet(40)
    r = MS.cluster(verts, cell, origin, rgba)
    i, _, ok = MS.cells(verts, cell, origin)
    assert ok.all() and r["n_clusters"] > 1
    ci = np.zeros((r["n_clusters"], 3), np.int64)
    ci[r["vertex_cluster"]] = i
    o, c = np.asarray(origin, np.float32).astype(np.float64), np.float64(np.float32(cell))
    lo, hi = (o + ci * c).astype(np.float32), (o + (ci + 1) * c).astype(np.float32)
    assert (r["positions"] >= lo).all() and (r["positions"] <= hi).all()


def test_a_cell_below_the_vertex_spacing_changes_no_face_and_barely_moves_a_vertex():
    verts, rgba, faces = _sheet(24)
    cell = 0.01                                                                    # spacing 0.1
    v, c, f, stats, vc = MS.simplify(verts, rgba, faces, cell, (0, 0, 0))
    assert np.array_equal(vc, np.arange(len(verts))) and np.array_equal(f, faces) and np.array_equal(c, rgba)
    assert (stats["faces_collapsed"], stats["faces_duplicate"], stats["faces_invalid"], stats["clusters"]) == (0, 0, 0, len(verts))
    # the 16-bit fraction truncates by at most cell / 65536, and the result rounds once to fp32 (half a unit in its last place).
    # (The two roundings of u can add up to 2 |p| 2^-24 on top in general; on this sheet at this cell they stay inside the bound.)
    bound = cell / 65536 + 0.5 * np.spacing(np.abs(v)).astype(np.float64)
    assert (np.abs(v.astype(np.float64) - verts.astype(np.float64)) <= bound).all()


def test_one_huge_cell_returns_an_empty_mesh():
    verts, rgba, faces = _sheet(12)
    v, c, f, stats, vc = MS.simplify(verts, rgba, faces, 1000.0, (-500, -500, -500))
    assert v.shape == (0, 3) and c.shape == (0,) and f.shape == (0, 3) and (vc == 0).all()
    assert stats["clusters"] == 1 and stats["faces_collapsed"] == len(faces)


@pytest.mark.parametrize("cell", [0.23, 0.4])
def test_simplifying_the_result_again_on_the_same_grid_leaves_the_faces_unchanged(cell):
    verts, rgba, faces = _sheet(40)
    v, c, f, stats, _ = MS.simplify(verts, rgba, faces, cell, (0, 0, 0))
    assert 0 < len(f) < len(faces)
    v2, c2, f2, stats2, vc2 = MS.simplify(v, c, f, cell, (0, 0, 0))
    assert np.array_equal(f2, f) and np.array_equal(vc2, np.arange(len(v))) and np.array_equal(c2, c)
    assert (stats2["faces_collapsed"], stats2["faces_duplicate"], stats2["faces_invalid"]) == (0, 0, 0)


def _rows(v, c, f):
    """the faces as rows of (position bits, colour) per corner, rotated so that the smallest corner row comes first, sorted"""
    corner = np.concatenate([v.view(np.uint32).astype(np.int64), c.astype(np.int64)[:, None]], 1)[f.astype(np.int64)]      # [K, 3, 4]
    out = []
    for t in corner.tolist():
        k = min(range(3), key=lambda j: t[j])
        out.append(tuple(t[k] + t[(k + 1) % 3] + t[(k + 2) % 3]))
    return sorted(out)


def test_a_permuted_face_list_gives_the_same_vertices_and_the_same_set_of_faces():
    verts, rgba, faces = _sheet(30)
    faces = np.concatenate([faces, faces[::7][:, [1, 2, 0]], faces[::11][:, [0, 2, 1]]])      # with duplicates and mirror images
    v, c, f, stats, vc = MS.simplify(verts, rgba, faces, 0.27, (0.01, 0, 0))
    for seed in (1, 2):
        p = np.random.default_rng(seed).permutation(len(faces))
        v2, c2, f2, stats2, vc2 = MS.simplify(verts, rgba, faces[p], 0.27, (0.01, 0, 0))
        assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(c2, c) and np.array_equal(vc2, vc) and stats2 == stats
        assert _rows(v2, c2, f2) == _rows(v, c, f)
