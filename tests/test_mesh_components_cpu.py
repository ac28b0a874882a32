"""tests/mesh_components_ref.py, the numpy restatement of include/spann3r_hip.h "Mesh components", against
scipy.sparse.csgraph.connected_components on every graph the device tests use, its own properties, and the selection with the
order-preserving renumbering.  No GPU."""
import numpy as np
import pytest

import mesh_components_ref as MC
from test_brick_mesh_cpu import face_rows


def _scipy_partition(faces, nv):
    """(labels [V] of scipy's components of the graph with an edge per pair of a valid face, the valid mask)"""
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    ok = MC.valid_faces(faces, nv)
    g = np.asarray(faces, np.int64)[ok]
    u, v = np.concatenate([g[:, 0], g[:, 0], g[:, 1]]), np.concatenate([g[:, 1], g[:, 2], g[:, 2]])
    adj = sp.coo_matrix((np.ones(len(u), np.int8), (u, v)), shape=(nv, nv)).tocsr()
    return connected_components(adj, directed=False)[1], ok


@pytest.mark.parametrize("name", MC.GRAPHS)
def test_the_restatement_equals_scipy_on_every_graph(name):
    faces, nv, ref = MC.graph(name)
    labels, ok = _scipy_partition(faces, nv)
    vc, fc = ref["vertex_component"], ref["face_component"]
    named = np.zeros(nv, bool)
    named[np.asarray(faces, np.int64)[ok].reshape(-1)] = True
    assert np.array_equal(vc >= 0, named) and np.array_equal(fc >= 0, ok) and ref["invalid_faces"] == int((~ok).sum())
    # the same partition of the named vertices: the pairs (ours, scipy's) are a bijection
    pairs = np.unique(np.stack([vc[named], labels[named]], 1), axis=0)
    assert len(pairs) == ref["n_components"] == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1]))
    # scipy gives a vertex no face names a class of its own
    assert len(np.unique(labels)) == ref["n_components"] + int((~named).sum())
    # a face lies in the component of each of its vertices
    g = np.asarray(faces, np.int64)[ok]
    assert (vc[g] == fc[ok][:, None]).all()


@pytest.mark.parametrize("name", MC.GRAPHS)
def test_ids_ascend_with_the_smallest_vertex_and_the_counts_add_up(name):
    faces, nv, ref = MC.graph(name)
    vc, c = ref["vertex_component"].astype(np.int64), ref["n_components"]
    first = np.full(c, nv, np.int64)
    np.minimum.at(first, vc[vc >= 0], np.flatnonzero(vc >= 0))
    assert (np.diff(first) > 0).all()                                              # id order = minimum-vertex order
    assert ref["component_faces"].sum() == MC.valid_faces(faces, nv).sum() == len(faces) - ref["invalid_faces"]
    assert ref["component_vertices"].sum() == (vc >= 0).sum() and (ref["component_faces"] > 0).all()
    assert np.array_equal(ref["component_faces"], np.bincount(ref["face_component"][ref["face_component"] >= 0], minlength=c))


def test_pinned_shapes_of_the_graphs():
    """what each graph is there for"""
    got = {n: (MC.graph(n)[2]["n_components"], MC.graph(n)[2]["invalid_faces"]) for n in MC.GRAPHS}
    assert got["strip_ascending"] == got["strip_descending"] == got["strip_shuffled"] == (1, 0) and got["star"] == (1, 0)
    assert got["sheet"] == (12, 0) and MC.graph("sheet")[1] == 270000 > 1024 * 256          # more than 1024 scan tiles of 256 vertices
    assert got["fans"] == (3, 4)
    f = MC.graph("fans")[2]
    assert f["vertex_component"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, -1, 1, 2, 2, -1, -1, -1, -1]           # the two fans are ONE component
    assert f["face_component"].tolist() == [0, 0, 0, 0, 0, 0, 1, 2, -1, -1, -1, -1, 0]
    assert f["component_faces"].tolist() == [7, 1, 1] and f["component_vertices"].tolist() == [8, 1, 2]
    r = MC.graph("random")[2]
    sizes = np.bincount(r["component_faces"])
    assert r["n_components"] == 525 and (r["vertex_component"] < 0).sum() == 1068 and sizes[1] == 151 and sizes[2] == 71
    assert np.sort(r["component_faces"])[-3:].tolist() == [41, 44, 44]            # keep_largest = 1 has a tie to break
    for name in ("strip_descending", "strip_shuffled"):
        assert np.array_equal(MC.graph(name)[2]["vertex_component"], MC.graph("strip_ascending")[2]["vertex_component"])


def test_a_permuted_face_list_gives_the_same_vertex_labels():
    faces, nv, ref = MC.graph("random")
    p = np.random.default_rng(5).permutation(len(faces))
    again = MC.components(faces[p], nv)
    assert np.array_equal(again["vertex_component"], ref["vertex_component"])
    assert np.array_equal(again["face_component"], ref["face_component"][p])


def test_keep_mask_order_and_ties():
    cf = [3, 7, 7, 1, 7, 3]
    assert MC.keep_mask(cf).all()
    assert MC.keep_mask(cf, min_faces=3).tolist() == [True, True, True, False, True, True]
    assert MC.keep_mask(cf, keep_largest=1).tolist() == [False, True, False, False, False, False]          # the lowest id wins a tie
    assert MC.keep_mask(cf, keep_largest=2).tolist() == [False, True, True, False, False, False]
    assert MC.keep_mask(cf, keep_largest=4).tolist() == [True, True, True, False, True, False]
    assert MC.keep_mask(cf, min_faces=7, keep_largest=4).tolist() == [False, True, True, False, True, False]
    assert MC.keep_mask(cf, min_faces=8, keep_largest=4).sum() == 0 and MC.keep_mask(cf, keep_largest=0).sum() == 0
    assert MC.keep_mask([]).shape == (0,)


@pytest.mark.parametrize("min_faces,keep_largest", [(1, None), (2, None), (5, None), (0, 1), (0, 3), (2, 3), (10 ** 6, None)])
def test_selection_then_renumbering_keeps_a_subsequence_of_the_rows(min_faces, keep_largest):
    faces, nv, ref = MC.graph("random")
    rng = np.random.default_rng(9)
    verts, rgba = rng.standard_normal((nv, 3)).astype(np.float32), rng.integers(0, 2 ** 32, nv, dtype=np.uint32)
    v, c, f, stats = MC.filter_mesh(verts, rgba, faces, min_faces, keep_largest)
    keep = MC.keep_mask(ref["component_faces"], min_faces, keep_largest)
    sel = keep[ref["face_component"]]                                             # (the random graph has no invalid face)
    assert stats == dict(total=ref["n_components"], kept=int(keep.sum()), faces_removed=int((~sel).sum()))
    # rows as position + colour words: the kept rows are the input's, in the input's order
    assert np.array_equal(face_rows(v, c, f.astype(np.int64)), face_rows(verts, rgba, faces.astype(np.int64))[sel])
    assert len(v) == len(np.unique(faces[sel])) and (len(f) == 0 or (f.min() == 0 and f.max() == len(v) - 1))
    used = np.unique(faces[sel])
    assert np.array_equal(v.view(np.uint32), verts[used].view(np.uint32)) and np.array_equal(c, rgba[used])      # index order kept
    if keep_largest is not None and min_faces == 0:
        assert stats["kept"] == keep_largest
    if min_faces == 10 ** 6:
        assert len(v) == 0 and f.shape == (0, 3)                                  # everything removed: an empty mesh


def test_invalid_faces_never_survive_a_selection():
    faces, nv, ref = MC.graph("fans")
    kept = MC.select_faces(faces, ref["face_component"], np.ones(ref["n_components"], bool))
    assert len(kept) == len(faces) - 4 and MC.valid_faces(kept, nv).all()
    assert np.array_equal(kept, faces[ref["face_component"] >= 0])


def test_edge_sizes():
    for faces, nv, want in ((np.zeros((0, 3), np.int32), 7, (0, 0)), (np.array([[0, 1, 2]], np.int32), 0, (0, 1)), (np.array([[2, 0, 1]], np.int32), 3, (1, 0))):
        r = MC.components(faces, nv)
        assert (r["n_components"], r["invalid_faces"]) == want
        assert r["vertex_component"].tolist() == ([0, 0, 0] if want == (1, 0) else [-1] * nv)
        assert r["face_component"].tolist() == ([0] if want == (1, 0) else [-1] * len(faces))
