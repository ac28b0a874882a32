"""The rule of include/spann3r_hip.h "Mesh components" in plain numpy: the anchor of every device comparison in
tests/test_mesh_components_gpu.py, itself checked against scipy.sparse.csgraph in tests/test_mesh_components_cpu.py.

The rule.  Vertices 0..V-1, faces [F, 3].  A face is valid when its three indices lie in 0..V-1.  Two vertices are connected when
a valid face names both (vertex connectivity: two fans that touch in one vertex are one component).  A component is a connectivity
class with at least one valid face; components are numbered 0..C-1 by ascending smallest vertex.  vertex_component is -1 for a vertex
no valid face names, face_component -1 for an invalid face.  Degenerate and duplicated faces are valid and count.

Selection: a component is kept when it has at least min_faces faces and, with keep_largest = k, is among the first k in the order
(faces descending, id ascending).  The kept faces stay in their original order; the vertices they name stay in index order and are
renumbered densely; everything else goes."""
import functools

import numpy as np


def valid_faces(faces, n_vertices):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < n_vertices)).all(1)


def components(faces, n_vertices):
    """-> dict(vertex_component int32 [V], face_component int32 [F], component_faces int32 [C], component_vertices int32 [C],
    n_components, invalid_faces).  Every vertex carries the smallest vertex index of its class: the labels of the two ends of every
    edge are lowered to their minimum, then every label is replaced by its label's label until nothing moves; repeated until stable."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(f, n_vertices)
    g = f[ok]
    u, v = np.concatenate([g[:, 0], g[:, 0]]), np.concatenate([g[:, 1], g[:, 2]])
    label = np.arange(n_vertices, dtype=np.int64)
    while len(u):
        new = label.copy()
        m = np.minimum(label[u], label[v])
        for target in (u, v, label[u], label[v]):
            np.minimum.at(new, target, m)
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            break
        label = new
    named = np.zeros(n_vertices, bool)
    named[g.reshape(-1)] = True
    roots = np.unique(label[named])                       # ascending smallest vertex = the numbering
    ident = np.full(n_vertices, -1, np.int64)
    ident[roots] = np.arange(len(roots))
    vertex_component = np.where(named, ident[label], -1)
    face_component = np.full(len(f), -1, np.int64)
    face_component[ok] = vertex_component[g[:, 0]]
    return dict(vertex_component=vertex_component.astype(np.int32), face_component=face_component.astype(np.int32),
                component_faces=np.bincount(face_component[ok], minlength=len(roots)).astype(np.int32),
                component_vertices=np.bincount(vertex_component[named], minlength=len(roots)).astype(np.int32),
                n_components=len(roots), invalid_faces=int((~ok).sum()))


def keep_mask(component_faces, min_faces=0, keep_largest=None):
    """bool [C]: at least min_faces faces and, with keep_largest = k, among the first k by (faces descending, id ascending)"""
    cf = [int(x) for x in component_faces]
    first = sorted(range(len(cf)), key=lambda i: (-cf[i], i))
    if keep_largest is not None:
        first = first[:keep_largest]
    first = set(first)
    return np.array([cf[i] >= min_faces and i in first for i in range(len(cf))], bool)


def select_faces(faces, face_component, keep):
    """the rows of faces whose component is kept, in their original order, indices unchanged"""
    f, fc = np.asarray(faces).reshape(-1, 3), np.asarray(face_component, np.int64)
    keep = np.asarray(keep, bool)
    sel = np.zeros(len(f), bool)
    inside = (fc >= 0) & (fc < len(keep))
    sel[inside] = keep[fc[inside]]
    return f[sel]


def renumber(vertices, rgba, faces):
    """order-preserving renumbering: the vertices the faces name, in index order, and the faces rewritten to their rows"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    used = np.unique(faces)
    remap = np.full(len(vertices), -1, np.int64)
    remap[used] = np.arange(len(used))
    return np.asarray(vertices)[used], np.asarray(rgba)[used], remap[faces].astype(np.int32)


def filter_mesh(vertices, rgba, faces, min_faces=0, keep_largest=None):
    """the whole of mesh.filter_components: -> (vertices, rgba, faces, dict(total, kept, faces_removed))"""
    c = components(faces, len(vertices))
    keep = keep_mask(c["component_faces"], min_faces, keep_largest)
    kept = select_faces(faces, c["face_component"], keep)
    v, col, f = renumber(vertices, rgba, kept)
    return v, col, f, dict(total=c["n_components"], kept=int(keep.sum()), faces_removed=len(np.asarray(faces).reshape(-1, 3)) - len(kept))


# ------------------------------------------------------------------------------------------------ the graphs of the tests
def strip(n=4096):
    """a path of n vertices as a strip of faces (i, i + 1, i + 2)"""
    i = np.arange(n - 2)
    return np.stack([i, i + 1, i + 2], 1).astype(np.int32), n


def star(n_faces=10000):
    """n_faces faces that touch only in vertex V - 1: (2 i, 2 i + 1, V - 1)"""
    i = np.arange(n_faces)
    nv = 2 * n_faces + 1
    return np.stack([2 * i, 2 * i + 1, np.full(n_faces, nv - 1)], 1).astype(np.int32), nv


def random_graph(nv=5000, nf=3000, seed=9):
    """nf random faces, each within 3 indices of a random vertex: about 500 components of 1 to 44 faces (the two largest tie), a
    fifth of the vertices named by no face"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, nv, nf)
    return np.stack([a, a + rng.integers(-3, 4, nf), a + rng.integers(-3, 4, nf)], 1).clip(0, nv - 1).astype(np.int32), nv


def striped_sheet(w=600, h=450, stripe=50):
    """a w x h grid sheet, two triangles per cell, without the cells of every stripe-th column: w / stripe stripes"""
    y, x = np.meshgrid(np.arange(h - 1), np.arange(w - 1), indexing="ij")
    y, x = y[x % stripe != stripe - 1], x[x % stripe != stripe - 1]
    tl = y * w + x
    tr, bl, br = tl + 1, tl + w, tl + w + 1
    faces = np.stack([np.stack([tl, tr, bl], 1), np.stack([tr, bl, br], 1)], 1).reshape(-1, 3)
    return faces.astype(np.int32), w * h


def fans():
    """two fans touching in vertex 4, a duplicated face, degenerate faces (one of them an island of its own), faces with -1, V and
    2^31 - 1 as an index, and unreferenced vertices; V = 16"""
    nv = 16
    faces = [[4, 0, 1], [4, 1, 2], [4, 2, 3],            # fan one
             [4, 5, 6], [6, 7, 4],                       # fan two: the same vertex 4
             [4, 1, 2],                                  # duplicate
             [9, 9, 9], [10, 10, 11],                    # degenerate: an island of one vertex, an edge
             [-1, 0, 1], [12, nv, 13], [12, 13, 2 ** 31 - 1], [-2 ** 31, 13, 14],      # invalid: 12, 13, 14 stay unnamed
             [0, 3, 3]]                                  # degenerate inside fan one
    return np.array(faces, np.int64).astype(np.int32), nv


def octahedron(first):
    """the 8 faces of an octahedron over vertices first .. first + 5 (+x, -x, +y, -y, +z, -z)"""
    f = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    pos = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    return np.array(f, np.int32) + first, pos


@functools.lru_cache(maxsize=None)
def graph(name):
    """(faces int32 [F, 3], V, the restatement's components of it): computed once, shared, not to be written to"""
    if name.startswith("strip"):
        faces, nv = strip()
        if name == "strip_descending":
            faces = faces[::-1].copy()
        elif name == "strip_shuffled":
            faces = faces[np.random.default_rng(3).permutation(len(faces))]
    else:
        faces, nv = dict(star=star, random=random_graph, sheet=striped_sheet, fans=fans)[name]()
    ref = components(faces, nv)
    for a in (faces,) + tuple(x for x in ref.values() if isinstance(x, np.ndarray)):
        a.setflags(write=False)
    return faces, nv, ref


GRAPHS = ("strip_ascending", "strip_descending", "strip_shuffled", "star", "random", "sheet", "fans")
