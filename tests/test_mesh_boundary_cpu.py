"""tests/mesh_boundary_ref.py (the numpy restatement of "Mesh boundary loops and hole filling", include/spann3r_hip.h) against a plain
Python walk: a dict from vertex to the element leaving it, followed until it returns or stops.  Runs on every mesh of the GPU tests
that is small enough, and checks by hand what the rule says about the smallest ones."""
import numpy as np
import pytest

import mesh_boundary_ref as B
import mesh_topology_ref as T


def walk(faces, nv):
    """the loops by walking: -> (elements [(e, h, src, dst)] in ascending edge number, next, loops as lists of elements from the head
    in ascending head, the number of irregular vertices)"""
    t = T.topology(faces, nv)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    elements = []
    for e in range(len(t["edge_class"])):
        if t["edge_class"][e] == 0:
            h = int(t["half_edges"][t["edge_first"][e]])
            elements.append((e, h, int(f[h // 3, h % 3]), int(f[h // 3, (h % 3 + 1) % 3])))
    leaving, entering = {}, {}
    for j, (_, _, s, d) in enumerate(elements):
        leaving.setdefault(s, []).append(j)
        entering.setdefault(d, []).append(j)
    regular = {v for v in set(leaving) | set(entering) if len(leaving.get(v, ())) == 1 and len(entering.get(v, ())) == 1}
    nxt = [leaving[d][0] if d in regular else -1 for (_, _, _, d) in elements]
    loops, seen = [], set()
    for j in range(len(elements)):                                                  # ascending: the first element met of a loop is its head
        if j in seen:
            continue
        path, k = [], j
        while k != -1 and k not in path:
            path.append(k)
            k = nxt[k]
        if k == j:
            loops.append(path)
            seen.update(path)
    return elements, nxt, loops, len((set(leaving) | set(entering)) - regular)


def assert_equals_the_walk(faces, nv):
    ref = B.boundary_loops(faces, nv)
    elements, nxt, loops, irregular = walk(faces, nv)
    b = len(elements)
    for k in B.TABLES:
        assert ref[k].dtype == np.int32, k
    for k in B.ELEMENT_TABLES:
        assert ref[k].shape == (b,), k
    assert [tuple(x) for x in np.stack([ref["edge"], ref["half_edge"], ref["src"], ref["dst"]], 1).tolist()] == elements if b else True
    assert ref["next"].tolist() == nxt
    loop, rank = [-1] * b, [-1] * b
    for l, path in enumerate(loops):
        for r, j in enumerate(path):
            loop[j], rank[j] = l, r
    assert ref["loop"].tolist() == loop and ref["rank"].tolist() == rank
    assert ref["loop_first"].tolist() == [0] + np.cumsum([len(p) for p in loops]).tolist()
    assert ref["loop_members"].tolist() == [j for p in loops for j in p]
    assert tuple(ref["report"]) == B.REPORT_KEYS
    assert ref["report"] == dict(boundary=b, loops=len(loops), open=loop.count(-1), irregular_vertices=irregular,
                                 longest=max([len(p) for p in loops], default=0))
    return ref


def fill_by_walk(verts, colors, faces, max_edges):
    elements, _, loops, _ = walk(faces, len(verts))
    p, f = [tuple(x) for x in np.asarray(verts, np.float32)], [tuple(x) for x in np.asarray(faces).tolist()]
    c = None if colors is None else [tuple(x) for x in np.asarray(colors).tolist()]
    nv = len(p)
    for path in loops:
        n = len(path)
        if n > max_edges:
            continue
        if n == 3:
            f.append((elements[path[0]][3], elements[path[0]][2], elements[path[2]][2]))
            continue
        s = np.asarray(verts[elements[path[0]][2]], np.float64)
        for j in path[1:]:
            s = s + np.asarray(verts[elements[j][2]], np.float64)
        p.append(tuple((s / np.float64(n)).astype(np.float32)))
        if c is not None:
            tot = [sum(int(colors[elements[j][2]][ch]) for j in path) for ch in range(4)]
            c.append(tuple((2 * x + n) // (2 * n) for x in tot))
        for j in path:
            f.append((elements[j][3], elements[j][2], len(p) - 1))
    return (np.asarray(p, np.float32).reshape(-1, 3), None if c is None else np.asarray(c, np.uint8).reshape(-1, 4),
            np.asarray(f, np.int32).reshape(-1, 3), len(p) - nv)


def assert_fill_equals_the_walk(verts, colors, faces, max_edges):
    v, c, f, stats = B.fill_holes(verts, colors, faces, max_edges)
    wv, wc, wf, added = fill_by_walk(verts, colors, faces, max_edges)
    assert v.dtype == np.float32 and f.dtype == np.int32 and np.array_equal(v.view(np.uint32), wv.view(np.uint32)) and np.array_equal(f, wf)
    assert (c is None and wc is None) or (c.dtype == np.uint8 and np.array_equal(c, wc))
    assert tuple(stats) == B.FILL_KEYS and stats["vertices_added"] == added and stats["faces_added"] == len(f) - len(faces)
    return v, c, f, stats


def _colors(nv):
    return (np.arange(4 * nv, dtype=np.uint32) * np.uint32(40503) >> 3).astype(np.uint8).reshape(-1, 4)


SMALL = dict(T.SMALL, bowtie=B.BOWTIE)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_cases_equal_the_walk(name):
    nv, faces = SMALL[name]
    ref = assert_equals_the_walk(faces, nv)
    mixed, _ = T.with_unusable(faces)
    refm = assert_equals_the_walk(mixed, nv)
    for k in B.TABLES:                                                              # unusable faces change h and nothing else
        if k != "half_edge":
            assert np.array_equal(ref[k], refm[k]), k
    assert refm["report"] == ref["report"]


def test_the_small_cases_are_what_the_rule_says():
    r = {name: B.boundary_loops(f, nv) for name, (nv, f) in SMALL.items()}
    tri = r["triangle"]
    assert tri["report"] == dict(boundary=3, loops=1, open=0, irregular_vertices=0, longest=3)
    assert tri["loop_first"].tolist() == [0, 3] and tri["rank"][tri["loop_members"]].tolist() == [0, 1, 2]
    assert tri["dst"][tri["loop_members"]].tolist() == tri["src"][np.roll(tri["loop_members"], -1)].tolist()
    tet = r["tetrahedron"]
    assert tet["report"] == dict(boundary=0, loops=0, open=0, irregular_vertices=0, longest=0)
    assert all(tet[k].shape == (0,) for k in B.ELEMENT_TABLES + ("loop_members",)) and tet["loop_first"].tolist() == [0]
    for name, b in (("three_on_an_edge", 6), ("pair_inconsistent", 4), ("bowtie", 6)):
        rep = r[name]["report"]
        assert (rep["boundary"], rep["loops"], rep["open"], rep["longest"]) == (b, 0, b, 0) and rep["irregular_vertices"] > 0, name
        assert (r[name]["loop"] == -1).all() and (r[name]["rank"] == -1).all() and r[name]["loop_first"].tolist() == [0]
    assert r["bowtie"]["report"]["irregular_vertices"] == 1 and (r["bowtie"]["next"] == -1).sum() == 2
    assert r["pair_consistent"]["report"] == dict(boundary=4, loops=1, open=0, irregular_vertices=0, longest=4)
    assert r["duplicate"]["report"]["boundary"] == 0


@pytest.mark.parametrize("n", B.FAN_SIZES)
def test_a_fan_rim_is_one_loop_of_its_length(n):
    verts, faces = T.closed_fan(n)
    ref = assert_equals_the_walk(faces, len(verts))
    assert ref["report"] == dict(boundary=n, loops=1, open=0, irregular_vertices=0, longest=n)
    assert sorted(ref["rank"].tolist()) == list(range(n)) and ref["loop_members"][0] == 0


def test_fans_of_every_length_in_one_mesh():
    verts, faces = B.all_fans()
    ref = assert_equals_the_walk(faces, len(verts))
    assert np.diff(ref["loop_first"]).tolist() == list(B.FAN_SIZES) and ref["report"]["longest"] == 1000
    perm = np.random.default_rng(3).permutation(len(faces))
    refp = assert_equals_the_walk(faces[perm], len(verts))
    for k in B.TABLES:                                                              # the order of the faces changes only half_edge
        assert np.array_equal(ref[k], refp[k]) == (k != "half_edge"), k


@pytest.mark.parametrize("bowtie", [False, True])
def test_the_punched_sheet(bowtie):
    verts, faces, holes, open_ = B.punched_sheet(33, bowtie)
    ref = assert_equals_the_walk(faces, len(verts))
    lengths = np.diff(ref["loop_first"])
    assert ref["report"] == dict(boundary=128 + 4 * holes + open_, loops=holes + 1, open=open_, irregular_vertices=1 if bowtie else 0, longest=128)
    assert sorted(lengths.tolist()) == [4] * holes + [128]
    for n, left in ((4, 128 + open_), (127, 128 + open_), (128, open_)):
        v, c, f, stats = assert_fill_equals_the_walk(verts, _colors(len(verts)), faces, n)
        t = T.topology(f, len(v))["report"]
        assert (t["boundary"], t["inconsistent"], t["nonmanifold"]) == (left, 0, 0)
        assert stats["filled"] == holes + (n >= 128) and stats["open"] == open_
        if not bowtie and n >= 128:
            assert t["closed"] and t["euler"] == 2
    assert_fill_equals_the_walk(verts, None, faces, 4)
    same = B.fill_holes(verts, None, faces, 3)
    assert same[3]["filled"] == 0 and np.array_equal(same[0], verts) and np.array_equal(same[2], faces) and same[1] is None


def test_the_icosphere_with_faces_dropped_comes_back_closed():
    verts, faces = B.icosphere(2)
    assert T.topology(faces, len(verts))["report"]["closed"] and len(faces) == 320
    drop = [0, 77, 150, 231, 319]
    kept = np.delete(faces, drop, 0)
    ref = assert_equals_the_walk(kept, len(verts))
    assert ref["report"] == dict(boundary=15, loops=5, open=0, irregular_vertices=0, longest=3)
    v, c, f, stats = assert_fill_equals_the_walk(verts, _colors(len(verts)), kept, 3)
    t = T.topology(f, len(v))["report"]
    assert t["closed"] and t["euler"] == 2 and t["inconsistent"] == 0 and stats["vertices_added"] == 0 and stats["faces_added"] == 5
    assert sorted(map(tuple, np.sort(f[-5:], 1).tolist())) == sorted(map(tuple, np.sort(faces[drop], 1).tolist()))
    # a 3-loop and a 4-loop in one mesh: the offsets of the new vertices and of the new faces disagree
    a, b = faces[5], None
    for g in range(len(faces)):
        if g not in drop and g != 5 and len(set(faces[g]) & set(a)) == 2 and not any(set(faces[g]) & set(faces[d]) for d in drop):
            b = g
            break
    kept2 = np.delete(faces, drop[:2] + [5, b] + drop[2:], 0)
    ref2 = assert_equals_the_walk(kept2, len(verts))
    assert sorted(np.diff(ref2["loop_first"]).tolist()) == [3, 3, 3, 3, 3, 4]
    v, c, f, stats = assert_fill_equals_the_walk(verts, _colors(len(verts)), kept2, 4)
    t = T.topology(f, len(v))["report"]
    assert t["closed"] and t["euler"] == 2 and t["inconsistent"] == 0 and stats["vertices_added"] == 1 and stats["faces_added"] == 9
    v3, _, f3, s3 = assert_fill_equals_the_walk(verts, None, kept2, 3)
    assert s3["filled"] == 5 and T.topology(f3, len(v3))["report"]["boundary"] == 4


def test_a_few_triangles_in_front_of_a_long_fan():
    verts, faces = B.cat([B.triangles(3), T.closed_fan(300), B.triangles(2)])
    ref = assert_equals_the_walk(faces, len(verts))
    assert np.diff(ref["loop_first"]).tolist() == [3, 3, 3, 300, 3, 3]
    assert_fill_equals_the_walk(verts, _colors(len(verts)), faces, 300)


def test_the_rounds():
    assert [B.rounds(b) for b in (0, 1, 2, 3, 4, 5, 255, 256, 257, 2 ** 17, 2 ** 17 + 1)] == [1, 1, 1, 2, 2, 3, 8, 8, 9, 17, 18]
