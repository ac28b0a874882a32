"""The rule of "Mesh boundary loops and hole filling" (include/spann3r_hip.h) restated in numpy: the boundary elements of an edge
table, their successor links, the loops with rank and CSR, the report, and the fans of fill_holes.  Vectorised -- the loops come
from doubling on whole arrays and one sort by (loop, rank), the centroid sums from a loop over the member POSITION rather than
over loops -- so that the large cases of the GPU tests stay fast.  tests/test_mesh_boundary_cpu.py checks it against a plain walk."""
import numpy as np

import mesh_topology_ref as T

ELEMENT_TABLES = ("edge", "half_edge", "src", "dst", "next", "loop", "rank")
TABLES = ELEMENT_TABLES + ("loop_first", "loop_members")
REPORT_KEYS = ("boundary", "loops", "open", "irregular_vertices", "longest")
FILL_KEYS = ("max_edges", "loops", "filled", "vertices_added", "faces_added", "open")


def rounds(b):
    """ceil(log2(max(b, 2)))"""
    r = 1
    while (1 << r) < b:
        r += 1
    return r


def boundary_loops(faces, nv, topo=None):
    """-> dict of the arrays in TABLES (int32) and report"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    t = T.topology(f, nv) if topo is None else topo
    edge = np.flatnonzero(t["edge_class"] == 0)
    b = len(edge)
    h = t["half_edges"].astype(np.int64)[t["edge_first"].astype(np.int64)[edge]] if b else np.zeros(0, np.int64)
    src, dst = f[h // 3, h % 3], f[h // 3, (h % 3 + 1) % 3]
    out_n, in_n = np.bincount(src, minlength=nv), np.bincount(dst, minlength=nv)
    regular = (out_n == 1) & (in_n == 1)
    leave = np.full(nv, -1, np.int64)
    leave[src] = np.arange(b)                                                       # (any of them where several leave: only read where regular)
    nxt = np.where(regular[dst], leave[dst], -1) if b else np.zeros(0, np.int64)
    # doubling: ptr = the element 2^k steps ahead, label = the smallest element of the window, steps = to its first place
    j = np.arange(b)
    ptr, label, steps = nxt.copy(), j.copy(), np.zeros(b, np.int64)
    for k in range(rounds(b)):
        on = np.flatnonzero(ptr >= 0)
        p = ptr[on]
        far = label[p] < label[on]                                                  # (strictly: on equal labels the near steps stay)
        label_new, steps_new, ptr_new = label.copy(), steps.copy(), ptr.copy()
        label_new[on[far]], steps_new[on[far]] = label[p[far]], steps[p[far]] + (1 << k)
        ptr_new[on] = ptr[p]
        ptr, label, steps = ptr_new, label_new, steps_new
    closed = ptr >= 0
    heads = np.flatnonzero(closed & (label == j))
    nl = len(heads)
    number = np.full(b, -1, np.int64)
    number[heads] = np.arange(nl)
    loop = np.where(closed, number[label], -1) if b else np.zeros(0, np.int64)
    length = np.bincount(loop[closed], minlength=nl) if nl else np.zeros(0, np.int64)
    rank = np.where(closed, (length[loop] - steps) % np.maximum(length[loop], 1), -1) if nl else np.full(b, -1, np.int64)
    on = np.flatnonzero(closed)
    members = on[np.lexsort((rank[on], loop[on]))]
    first = np.concatenate([[0], np.cumsum(length)])
    seen = (out_n + in_n) > 0
    report = dict(boundary=b, loops=nl, open=int(b - closed.sum()), irregular_vertices=int((seen & ~regular).sum()),
                  longest=int(length.max()) if nl else 0)
    i32 = lambda x: np.ascontiguousarray(x, np.int64).astype(np.int32)
    return dict(edge=i32(edge), half_edge=i32(h), src=i32(src), dst=i32(dst), next=i32(nxt), loop=i32(loop), rank=i32(rank),
                loop_first=i32(first), loop_members=i32(members), report=report)


def fill_holes(verts, colors, faces, max_edges, loops=None):
    """-> (vertices fp32 [V + added, 3], colors uint8 [V + added, 4] or None, faces int32 [F + added, 3], fill dict)"""
    assert max_edges >= 3
    p = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    nv = len(p)
    lp = boundary_loops(f, nv) if loops is None else loops
    first, members = lp["loop_first"].astype(np.int64), lp["loop_members"].astype(np.int64)
    src, dst = lp["src"].astype(np.int64), lp["dst"].astype(np.int64)
    length = np.diff(first)
    fill = np.flatnonzero(length <= max_edges)
    fan = fill[length[fill] > 3]
    centre = np.full(len(length), -1, np.int64)
    centre[fan] = nv + np.arange(len(fan))
    # the centres: every fan with more than k members adds the source of its k-th; descending length makes the active fans a prefix
    order = fan[np.argsort(-length[fan], kind="stable")]
    lo, start = length[order], first[order]
    new_p = np.zeros((len(fan), 3), np.float32)
    new_c = None if colors is None else np.zeros((len(fan), 4), np.uint8)
    if len(fan):
        s = p[src[members[start]]].astype(np.float64)
        for k in range(1, int(lo[0])):
            n = int(np.searchsorted(-lo, -k, side="left"))
            s[:n] = s[:n] + p[src[members[start[:n] + k]]].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            new_p[centre[order] - nv] = (s / lo[:, None].astype(np.float64)).astype(np.float32)
        if colors is not None:
            c = np.asarray(colors, np.uint8).reshape(-1, 4).astype(np.int64)
            tot = np.zeros((len(fan), 4), np.int64)
            for k in range(int(lo[0])):
                n = int(np.searchsorted(-lo, -k, side="left"))
                tot[:n] += c[src[members[start[:n] + k]]]
            new_c[centre[order] - nv] = ((2 * tot + lo[:, None]) // (2 * lo[:, None])).astype(np.uint8)
    # the faces, in (loop, rank) order: one per member of a fan, one per triangle
    per = np.where(length[fill] > 3, length[fill], 1)
    which = np.repeat(fill, per)                                                    # the loop of every new face
    k = np.arange(len(which)) - np.repeat(np.cumsum(per) - per, per)                # its rank
    m = members[first[which] + k]
    third = np.where(length[which] > 3, centre[which], src[members[first[which] + 2]])
    new_f = np.stack([dst[m], src[m], third], 1).astype(np.int32).reshape(-1, 3)
    out_c = None if colors is None else np.concatenate([np.asarray(colors, np.uint8).reshape(-1, 4), new_c])
    stats = dict(max_edges=int(max_edges), loops=len(length), filled=len(fill), vertices_added=len(fan), faces_added=len(new_f),
                 open=lp["report"]["open"])
    return np.concatenate([p, new_p]), out_c, np.concatenate([f, new_f]), stats


# ------------------------------------------------------------------------------------------------ the meshes of the tests
BOWTIE = (5, [(0, 1, 2), (0, 3, 4)])
FAN_SIZES = (3, 4, 5, 7, 8, 9, 255, 256, 257, 1000)


def cat(parts):
    """[(verts, faces), ..] -> one mesh with vertex offsets"""
    vs, fs, at = [], [], 0
    for v, f in parts:
        vs.append(np.asarray(v, np.float32).reshape(-1, 3))
        fs.append(np.asarray(f, np.int64).reshape(-1, 3) + at)
        at += len(vs[-1])
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def all_fans():
    return cat([T.closed_fan(n) for n in FAN_SIZES])


def triangles(n):
    """n disjoint triangles -> (verts fp32 [3 n, 3], faces int32 [n, 3])"""
    i = np.arange(3 * n)
    verts = np.stack([i * 0.25, (i % 3 == 1) * 1.0, (i % 3 == 2) * 1.0], 1).astype(np.float32)
    return verts, i.reshape(-1, 3).astype(np.int32)


def punched_sheet(n=33, bowtie=False):
    """grid_sheet(n) without the interior cells (2 i + 1, 2 j + 1): disjoint 4-loops inside the rim of 4 (n - 1) edges.  bowtie: cell (2, 2) goes
    instead of the cells (1, 3), (3, 1) and (3, 3): the holes (1, 1) and (2, 2) are diagonal neighbours, meet in one vertex and come
    out open
    -> (verts, faces, the number of 4-loops, the elements on open chains)"""
    verts, faces = T.grid_sheet(n, 1.0 / (n - 1))
    verts[:, 2] = (0.05 * np.sin(np.arange(len(verts)) * 0.37)).astype(np.float32)
    cy, cx = np.divmod(np.arange((n - 1) ** 2), n - 1)
    gone = (cy % 2 == 1) & (cx % 2 == 1) & (cy < n - 2) & (cx < n - 2)            # (interior cells: the rim stays whole)
    holes = int(gone.sum())
    if bowtie:
        gone &= ~(((cy == 3) | (cx == 3)) & (cy <= 3) & (cx <= 3))
        gone |= (cy == 2) & (cx == 2)
    keep = np.concatenate([~gone, ~gone])
    return verts, faces[keep], holes - (4 if bowtie else 0), 8 if bowtie else 0


def icosphere(level=2):
    """an icosahedron subdivided `level` times at the edge midpoints, on the unit sphere, outward faces -> (verts fp32, faces int32)"""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1),
         (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.asarray(v, np.float32), np.asarray(f, np.int32)
