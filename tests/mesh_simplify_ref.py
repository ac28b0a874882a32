"""The rule of include/spann3r_hip.h "Mesh simplification" in plain numpy: the anchor of every device comparison in
tests/test_mesh_simplify_gpu.py, itself checked against a second formulation (a Python dict keyed by the cell tuple, looped vertex
by vertex) in tests/test_mesh_simplify_cpu.py.  Open3D's simplify_vertex_clustering is not available: parity with it is unpinned.

The rule.  vertices fp32 [V, 3], rgba uint32 [V] (optional), faces int32 [F, 3], origin fp32 [3], cell > 0 fp32, inv = fp32(1) / cell.
1. Per axis u = (p - o) * inv, two rounded fp32 operations; i = floor(u).  A vertex is usable when all three u are finite and
   |i| < 2^30; an unusable vertex has vertex_cluster -1.  r = u - i (one rounded fp32 subtraction: exact unless -0.5 < u < 0) and
   q = min(int(r * 65536), 65535).
2. A cluster is the set of usable vertices of one cell; clusters are numbered by ascending smallest member vertex.
3. Per axis pos = fp32(fp64(o) + (fp64(i) + fp64(sum q) / fp64(n) / 65536) * fp64(cell)), every operation rounded on its own; per colour
   byte (2 sum c + n) // (2 n).
4. A face is valid when its indices lie in 0..V-1 and name usable vertices.  A valid face is remapped to cluster ids and collapsed
   when two ids are equal.  With dedup the survivors are grouped by their triple rotated so that the smallest id comes first (the
   winding stays: a mirror image is another face); the lowest original index of each group is kept.  Kept faces stay in original
   order and rotation.
5. The clusters no kept face names are dropped and the rest renumbered in order (sp3_mesh_compact_vertices)."""
import numpy as np

LIMIT = np.float32(2.0 ** 30)


def cells(vertices, cell, origin=None):
    """-> (i int64 [V, 3], q int64 [V, 3], usable bool [V]); rows of unusable vertices are zero"""
    p = np.asarray(vertices, np.float32).reshape(-1, 3)
    o = np.zeros(3, np.float32) if origin is None else np.asarray(origin, np.float32).reshape(3)
    inv = np.float32(1) / np.float32(cell)
    with np.errstate(all="ignore"):
        u = (p - o[None]) * inv
        fi = np.floor(u)
        usable = (np.isfinite(u) & (np.abs(fi) < LIMIT)).all(1)
        u, fi = np.where(usable[:, None], u, np.float32(0)), np.where(usable[:, None], fi, np.float32(0))
        r = (u - fi).astype(np.float32)
        q = np.minimum((r * np.float32(65536)).astype(np.int64), 65535)
    return fi.astype(np.int64), q, usable


def cluster(vertices, cell, origin=None, rgba=None):
    """-> dict(positions fp32 [C, 3], rgba uint32 [C] or None, vertex_cluster int32 [V], n_clusters)"""
    p = np.asarray(vertices, np.float32).reshape(-1, 3)
    o = np.zeros(3, np.float32) if origin is None else np.asarray(origin, np.float32).reshape(3)
    i, q, usable = cells(p, cell, o)
    idx = np.flatnonzero(usable)
    vertex_cluster = np.full(len(p), -1, np.int64)
    if len(idx) == 0:
        return dict(positions=np.zeros((0, 3), np.float32), rgba=None if rgba is None else np.zeros(0, np.uint32),
                    vertex_cluster=vertex_cluster.astype(np.int32), n_clusters=0)
    keys, group = np.unique(i[idx], axis=0, return_inverse=True)
    group = group.reshape(-1)
    leader = np.full(len(keys), len(p), np.int64)
    np.minimum.at(leader, group, idx)
    ident = np.empty(len(keys), np.int64)
    ident[np.argsort(leader)] = np.arange(len(keys))              # numbered by ascending smallest member
    cid = ident[group]
    vertex_cluster[idx] = cid
    c = len(keys)
    n = np.zeros(c, np.int64)
    np.add.at(n, cid, 1)
    sq = np.zeros((c, 3), np.int64)
    np.add.at(sq, cid, q[idx])
    ci = np.zeros((c, 3), np.int64)
    ci[cid] = i[idx]
    frac = sq.astype(np.float64) / n.astype(np.float64)[:, None] / np.float64(65536.0)
    pos = (o.astype(np.float64)[None] + (ci.astype(np.float64) + frac) * np.float64(np.float32(cell))).astype(np.float32)
    col = None
    if rgba is not None:
        w = np.asarray(rgba).astype(np.uint32).reshape(-1)[idx].astype(np.int64)
        col = np.zeros(c, np.int64)
        for k in range(4):
            sc = np.zeros(c, np.int64)
            np.add.at(sc, cid, (w >> (8 * k)) & 255)
            col |= ((2 * sc + n) // (2 * n)) << (8 * k)
        col = col.astype(np.uint32)
    return dict(positions=pos, rgba=col, vertex_cluster=vertex_cluster.astype(np.int32), n_clusters=c)


def rotate_smallest_first(t):
    t = np.asarray(t, np.int64).reshape(-1, 3)
    k = np.argmin(t, axis=1)
    return np.stack([t[np.arange(len(t)), (k + j) % 3] for j in range(3)], axis=1)


def cluster_faces(faces, vertex_cluster, dedup=True):
    """-> (kept faces int32 [K, 3] in cluster ids, dict(invalid, collapsed, duplicate))"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    vc = np.asarray(vertex_cluster, np.int64).reshape(-1)
    inside = ((f >= 0) & (f < len(vc))).all(1)
    t = np.full(f.shape, -1, np.int64)
    t[inside] = vc[f[inside]]
    valid = (t >= 0).all(1)
    collapsed = valid & ((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2]))
    alive = np.flatnonzero(valid & ~collapsed)
    keep = alive
    if dedup and len(alive):
        _, group = np.unique(rotate_smallest_first(t[alive]), axis=0, return_inverse=True)
        group = group.reshape(-1)
        first = np.full(group.max() + 1, len(f), np.int64)
        np.minimum.at(first, group, alive)
        keep = alive[first[group] == alive]
    return t[keep].astype(np.int32), dict(invalid=int((~valid).sum()), collapsed=int(collapsed.sum()), duplicate=len(alive) - len(keep))


def simplify(vertices, rgba, faces, cell, origin=None, dedup=True):
    """-> (vertices fp32 [V', 3], rgba uint32 [V'], faces int32 [K, 3] or None, stats, vertex_cluster int32 [V]): cluster, remap,
    then drop and renumber the clusters no kept face names (a cloud, faces None, keeps every cluster)"""
    c = cluster(vertices, cell, origin, rgba)
    nf = 0 if faces is None else len(np.asarray(faces).reshape(-1, 3))
    stats = dict(cell=float(np.float32(cell)), clusters=c["n_clusters"], faces_in=nf, faces_collapsed=0, faces_duplicate=0, faces_invalid=0)
    if faces is None:
        return c["positions"], c["rgba"], None, stats, c["vertex_cluster"]
    kept, counts = cluster_faces(faces, c["vertex_cluster"], dedup)
    stats.update(faces_collapsed=counts["collapsed"], faces_duplicate=counts["duplicate"], faces_invalid=counts["invalid"])
    used = np.unique(kept.reshape(-1))
    new = np.full(c["n_clusters"] + 1, -1, np.int64)
    new[used] = np.arange(len(used))
    return c["positions"][used], c["rgba"][used], new[kept.astype(np.int64)].astype(np.int32).reshape(-1, 3), stats, c["vertex_cluster"]
