"""The rule of "Mesh topology and smoothing" (include/spann3r_hip.h) restated in numpy: the edge table of the usable faces, the
vertex adjacency, the report, one smoothing pass and the lambda|mu filter.  Vectorised -- np.unique on packed keys, and a loop over
the neighbour POSITION rather than over vertices -- so that the large cases of the GPU tests stay fast.
tests/test_mesh_topology_cpu.py checks it against fusion_ref.manifold_report, a dict-of-sets loop and a vertex-by-vertex loop."""
import numpy as np

REPORT_KEYS = ("edges", "boundary", "interior", "inconsistent", "nonmanifold", "faces_usable", "faces_unusable", "vertices_referenced",
               "euler", "closed")
TABLES = ("edges", "edge_first", "half_edges", "edge_uses", "edge_fwd", "edge_class", "vertex_offsets", "vertex_neighbors", "vertex_boundary")


def usable_faces(faces, nv):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    return ((f >= 0) & (f < nv)).all(1) & (a != b) & (b != c) & (a != c)


def topology(faces, nv):
    """-> dict of the arrays in TABLES (dtypes as on the device) and report"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = usable_faces(f, nv)
    fi = np.flatnonzero(ok)
    h = (3 * fi[:, None] + np.arange(3)[None, :]).reshape(-1)                       # ascending
    a, b = f[fi].reshape(-1), f[fi][:, [1, 2, 0]].reshape(-1)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    pair = (lo << 31) | hi
    und, inv, uses = np.unique(pair, return_inverse=True, return_counts=True)
    e = len(und)
    order = np.lexsort((h, inv))                                                    # by edge, then ascending h
    fwd = np.bincount(inv, weights=(a < b), minlength=e).astype(np.int64)
    cls = np.where(uses == 1, 0, np.where(uses > 2, 3, np.where(fwd == 1, 1, 2)))
    edges = np.stack([und >> 31, und & (2 ** 31 - 1)], 1).reshape(-1, 2)
    first = np.concatenate([[0], np.cumsum(uses)])
    directed = np.unique(np.concatenate([(edges[:, 0] << 32) | edges[:, 1], (edges[:, 1] << 32) | edges[:, 0]]))
    offsets = np.searchsorted(directed >> 32, np.arange(nv + 1))
    boundary = np.zeros(nv, np.uint8)
    boundary[edges[cls == 0].reshape(-1)] = 1
    counts = np.bincount(cls, minlength=4)
    referenced = int((np.diff(offsets) > 0).sum())
    report = dict(edges=e, boundary=int(counts[0]), interior=int(counts[1]), inconsistent=int(counts[2]), nonmanifold=int(counts[3]),
                  faces_usable=len(fi), faces_unusable=len(f) - len(fi), vertices_referenced=referenced, euler=referenced - e + len(fi),
                  closed=bool(e > 0 and counts[1] == e))
    return dict(edges=edges.astype(np.int32), edge_first=first.astype(np.int32), half_edges=h[order].astype(np.int32),
                edge_uses=uses.astype(np.int32), edge_fwd=fwd.astype(np.int32), edge_class=cls.astype(np.uint8),
                vertex_offsets=offsets.astype(np.int32), vertex_neighbors=(directed & 0xffffffff).astype(np.int32),
                vertex_boundary=boundary, report=report)


def smooth_pass(p, offsets, neighbors, c, fixed=None):
    """one pass with factor c: p fp32 [V, 3] -> fp32 [V, 3].  The rows are walked by neighbour position j = 0, 1, ..: every vertex with
    more than j neighbours adds its j-th, so each sum has the row's order; the vertices are taken in descending valence, which makes
    the active ones a prefix."""
    p = np.ascontiguousarray(p, np.float32)
    offsets, neighbors = np.asarray(offsets, np.int64), np.asarray(neighbors, np.int64)
    k = np.diff(offsets)
    move = k > 0
    if fixed is not None:
        move &= np.asarray(fixed) == 0
    vs = np.flatnonzero(move)
    vs = vs[np.argsort(-k[vs], kind="stable")]
    out = p.copy()
    if len(vs) == 0:
        return out
    kv, start = k[vs], offsets[vs]
    s = p[neighbors[start]].astype(np.float64)
    for j in range(1, int(kv[0])):
        n = int(np.searchsorted(-kv, -j, side="left"))                             # the vertices with kv > j
        s[:n] = s[:n] + p[neighbors[start[:n] + j]].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        pv = p[vs].astype(np.float64)
        m = s / kv[:, None].astype(np.float64)
        out[vs] = (pv + np.float64(c) * (m - pv)).astype(np.float32)
    return out


def smooth(p, faces, iterations=10, lam=0.5, mu=-0.53, boundary="fixed", topo=None):
    """the lambda|mu filter: -> fp32 [V, 3]"""
    assert boundary in ("fixed", "free")
    p = np.ascontiguousarray(p, np.float32)
    t = topology(faces, len(p)) if topo is None else topo
    fixed = t["vertex_boundary"] if boundary == "fixed" else None
    for _ in range(int(iterations)):
        p = smooth_pass(p, t["vertex_offsets"], t["vertex_neighbors"], lam, fixed)
        if mu != 0:
            p = smooth_pass(p, t["vertex_offsets"], t["vertex_neighbors"], mu, fixed)
    return p


# ------------------------------------------------------------------------------------------------ the meshes of the tests
def grid_sheet(n, step=1.0):
    """an n x n-vertex sheet in z = 0 over [0, (n - 1) step]^2, two consistently wound triangles per cell -> (verts fp32, faces int32)"""
    y, x = np.mgrid[:n, :n]
    verts = np.stack([x * step, y * step, np.zeros_like(x, np.float64)], -1).reshape(-1, 3).astype(np.float32)
    tl = (y[:-1, :-1] * n + x[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([tl, tl + 1, tl + n], 1), np.stack([tl + 1, tl + n + 1, tl + n], 1)]).astype(np.int32)
    return verts, faces


def book(pages, first=2, reverse_every=0):
    """`pages` triangles (0, 1, k) on the one edge (0, 1); with reverse_every = r every r-th page is (1, 0, k) -> faces int32"""
    k = np.arange(first, first + pages)
    f = np.stack([np.zeros_like(k), np.ones_like(k), k], 1)
    if reverse_every:
        f[::reverse_every] = f[::reverse_every][:, [1, 0, 2]]
    return f.astype(np.int32)


def closed_fan(n):
    """n triangles (0, 1 + i, 1 + (i + 1) % n) around vertex 0 -> (verts fp32 [n + 1, 3], faces int32 [n, 3])"""
    i = np.arange(n)
    faces = np.stack([np.zeros_like(i), 1 + i, 1 + (i + 1) % n], 1).astype(np.int32)
    ang = 2 * np.pi * i / n
    rim = np.stack([np.cos(ang), np.sin(ang), 0.1 * np.sin(7 * ang)], 1)
    return np.concatenate([[[0.013, -0.021, 0.3]], rim]).astype(np.float32), faces


SMALL = dict(
    triangle=(3, [(0, 1, 2)]),
    tetrahedron=(4, [(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)]),
    pair_consistent=(4, [(0, 1, 2), (1, 0, 3)]),
    pair_inconsistent=(4, [(0, 1, 2), (0, 1, 3)]),
    duplicate=(3, [(0, 1, 2), (0, 1, 2)]),
    three_on_an_edge=(5, [(0, 1, 2), (1, 0, 3), (0, 1, 4)]),
)
UNUSABLE = [(0, 1, 9), (-1, 0, 1), (2, 2, 1), (1, 0, 0), (2, 1, 2), (0, 0, 0), (2 ** 31 - 1, 0, 1), (-2 ** 31, 1, 2)]


def with_unusable(faces):
    """the faces with UNUSABLE mixed in (for nv <= 9): every usable face keeps its order -> (faces, the positions of the usable ones)"""
    out, where = [], []
    for i, f in enumerate(faces):
        out.append(UNUSABLE[(2 * i) % len(UNUSABLE)])
        where.append(len(out))
        out.append(f)
        out.append(UNUSABLE[(2 * i + 1) % len(UNUSABLE)])
    return np.asarray(out + UNUSABLE, np.int64).astype(np.int32), np.asarray(where)
