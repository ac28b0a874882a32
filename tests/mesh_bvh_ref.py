"""The structure and the two walks of include/spann3r_hip.h "Mesh BVH" restated on the host: the anchor of the counts and of the
structure in tests/test_mesh_bvh_gpu.py, itself checked in tests/test_mesh_bvh_cpu.py against tests/mesh_distance_ref.py and
tests/mesh_ray_ref.py (bit for bit: the tree only chooses WHICH faces are looked at, the rule of a face and the lexicographic
minimum are theirs).

The level table, the keys and the boxes are numpy; the walks are loops over Python floats (IEEE doubles, one rounding per
operation, nothing fuses) that evaluate a face with mesh_distance_ref.closest_pair_loop / mesh_ray_ref.hit_pair_loop, which
tests/test_mesh_distance_cpu.py and tests/test_mesh_ray_cpu.py hold to the numpy rules bit for bit.

The structure.  LEAF faces per leaf, ARITY children per node.  Leaf k holds order[k LEAF .. (k + 1) LEAF); node k of level l + 1
holds nodes k ARITY .. of level l; a node exists iff its index is below its level's size.  A node's box is the fp32 min / max of
the vertices below it.  slack = 1e-6 (largest |coordinate| of the box of the finite vertices + its largest extent).
Distance: g = max(max(lo - p, p - hi) - slack, 0) per axis, lb = ((gx gx + gy gy) + gz gz) (1 - 2^-30); skipped iff lb > best d2.
Rays: the slab clip of [t_min, t_max] against the box pushed out by the slack (d = 0 on an axis: a test of o); skipped iff the
range is empty or its entry is > best t.  Both tests when a node is pushed and again when it is popped; children nearest first
(an odd-even transposition sort of (key, child) that swaps on a strict <, absent and skipped children at +inf)."""
import math

import numpy as np

import mesh_distance_ref as DR
import mesh_ray_ref as RR

LEAF = 4
ARITY = 4
KEY_NONE = 2 ** 63 - 1
MARGIN = 1.0 - 2.0 ** -30
COUNTS = (1, LEAF, LEAF + 1, LEAF * ARITY, LEAF * ARITY + 1, LEAF * ARITY ** 2 + 1, 1922)      # usable faces at which the level table changes shape


def level_table(usable, leaf=LEAF, arity=ARITY):
    """-> (sizes, offsets) of the tree over `usable` >= 1 faces"""
    assert usable >= 1
    sizes = [(usable + leaf - 1) // leaf]
    while sizes[-1] > 1:
        sizes.append((sizes[-1] + arity - 1) // arity)
    return sizes, [0] + np.cumsum(sizes).tolist()


def stack_entries(levels, arity=ARITY):
    return (arity - 1) * (levels - 1) + 1


def finite_box(vertices):
    """fp64 [2, 3]: min and max of the finite coordinates per axis, 0 where there is none"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    fin = np.isfinite(v)
    if len(v) == 0:
        return np.zeros((2, 3))
    box = np.stack([np.where(fin, v, np.inf).min(0), np.where(fin, v, -np.inf).max(0)])
    return np.where(np.isfinite(box), box, 0.0)


def slack_of(box):
    return float(np.float32(1e-6 * (float(np.abs(box).max()) + float((box[1] - box[0]).max()))))      # (the descriptor holds an fp32)


def key_box(box):
    """the fp32 box the keys are quantised against (the box of fp32 vertices is exact in fp32) -> (lo, hi) fp32 [3]"""
    return box[0].astype(np.float32), box[1].astype(np.float32)


def _spread3(x):
    v = x.astype(np.uint64) & np.uint64(0x1fffff)
    for shift, mask in ((32, 0x1f00000000ffff), (16, 0x1f0000ff0000ff), (8, 0x100f00f00f00f00f), (4, 0x10c30c30c30c30c3), (2, 0x1249249249249249)):
        v = (v | (v << np.uint64(shift))) & np.uint64(mask)
    return v


def morton_keys(centres, ok, lo, hi):
    """centres fp32 [n, 3], ok bool [n], the fp32 key box -> int64 [n]"""
    c = np.asarray(centres, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        ext = (hi - lo).astype(np.float32)
        scale = np.where(ext > 0, np.float32(2097152.0) / np.where(ext > 0, ext, np.float32(1)), np.float32(0)).astype(np.float32)
        scale = np.where(np.isfinite(scale), scale, np.float32(0)).astype(np.float32)
        t = np.floor(((c - lo).astype(np.float32) * scale).astype(np.float32))
        q = np.minimum(np.maximum(np.where(np.isnan(t), np.float32(0), t), np.float32(0)), np.float32(2097151)).astype(np.uint32)
    m = _spread3(q[:, 0]) | (_spread3(q[:, 1]) << np.uint64(1)) | (_spread3(q[:, 2]) << np.uint64(2))
    return np.where(ok, np.minimum(m, np.uint64(KEY_NONE - 1)), np.uint64(KEY_NONE)).astype(np.int64)


def face_keys(vertices, faces, box=None):
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    box = finite_box(v) if box is None else box
    use = DR.usable(vertices, faces)
    tri = v[np.where(use[:, None], f, 0)] if len(v) else np.zeros((len(f), 3, 3), np.float32)
    with np.errstate(all="ignore"):
        centres = (np.float32(0.5) * tri.min(1) + np.float32(0.5) * tri.max(1)).astype(np.float32)
    return morton_keys(centres, use, *key_box(box))


def point_keys(points, box):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    return morton_keys(p, np.isfinite(p).all(1), *key_box(box))


def build(vertices, faces, order=None):
    """-> dict(usable, order int32 [usable], sizes, offsets, node_lo / node_hi fp32 [nodes, 3], slack, levels).  order: the usable
    faces in any order (the device's, say); None: the stable sort of the keys."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    box = finite_box(v)
    if order is None:
        keys = face_keys(v, f, box)
        order = np.argsort(keys, kind="stable")[:int((keys != KEY_NONE).sum())]
    order = np.asarray(order, np.int32)
    usable = len(order)
    sizes, offsets = level_table(usable)
    lo = np.full((offsets[-1], 3), np.inf, np.float32)
    hi = np.full((offsets[-1], 3), -np.inf, np.float32)
    tri = v[f[order]]                                             # [usable, 3, 3]
    for k in range(sizes[0]):
        lo[k], hi[k] = tri[k * LEAF:(k + 1) * LEAF].reshape(-1, 3).min(0), tri[k * LEAF:(k + 1) * LEAF].reshape(-1, 3).max(0)
    for l in range(1, len(sizes)):
        for k in range(sizes[l]):
            c0, c1 = offsets[l - 1] + k * ARITY, offsets[l - 1] + min((k + 1) * ARITY, sizes[l - 1])
            lo[offsets[l] + k], hi[offsets[l] + k] = lo[c0:c1].min(0), hi[c0:c1].max(0)
    return dict(usable=usable, order=order, sizes=sizes, offsets=offsets, levels=len(sizes), node_lo=lo, node_hi=hi, slack=slack_of(box),
                vertices=v, faces=f)


# ------------------------------------------------------------------------------------------------ the two bounds, elementwise (numpy)
def dist_bound(lo, hi, p, slack):
    """fp32 boxes [..., 3], queries fp64 [..., 3] -> lb fp64 [...]"""
    lo, hi, p = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64), np.asarray(p, np.float64)
    slack = np.asarray(slack, np.float64)[..., None]              # one per box, or one for all
    g = np.maximum(np.maximum(lo - p, p - hi) - slack, 0.0)
    return ((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]) * MARGIN


def ray_clip(lo, hi, o, d, slack, t_min=0.0, t_max=math.inf):
    """fp32 boxes [..., 3], rays fp64 [..., 3] -> (ok bool [...], t0, t1 fp64 [...])"""
    slack = np.asarray(slack, np.float64)[..., None]
    lo, hi = np.asarray(lo, np.float32).astype(np.float64) - slack, np.asarray(hi, np.float32).astype(np.float64) + slack
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    shape = np.broadcast_shapes(lo.shape, o.shape, d.shape)[:-1]
    t0, t1, ok = np.full(shape, float(t_min)), np.full(shape, float(t_max)), np.ones(shape, bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            zero = np.broadcast_to(d[..., k] == 0, shape)
            inside = (o[..., k] >= lo[..., k]) & (o[..., k] <= hi[..., k])
            a, b = (lo[..., k] - o[..., k]) / d[..., k], (hi[..., k] - o[..., k]) / d[..., k]
            t0 = np.where(zero, t0, np.maximum(t0, np.minimum(a, b)))
            t1 = np.where(zero, t1, np.minimum(t1, np.maximum(a, b)))
            ok &= ~zero | inside
    return ok & (t0 <= t1), t0, t1


# ------------------------------------------------------------------------------------------------ the walk (Python floats)
def _walk(tree, bound, visit_face, best):
    """bound(node) -> (inside, key); visit_face(f) updates best[0]; -> (nodes visited, faces evaluated).  best: a one-element list."""
    sizes, offsets, order, usable = tree["sizes"], tree["offsets"], tree["order"], tree["usable"]
    cap = stack_entries(len(sizes))
    nodes = evals = 0
    stack = []
    root = len(sizes) - 1
    ok, key = bound(offsets[root])
    if ok and not key > best[0]:
        stack.append((root, 0))
    while stack:
        l, k = stack.pop()
        ok, key = bound(offsets[l] + k)
        if not (ok and not key > best[0]):
            continue
        nodes += 1
        if l == 0:
            for at in range(k * LEAF, min((k + 1) * LEAF, usable)):
                evals += 1
                visit_face(int(order[at]))
            continue
        kids = []
        for i in range(ARITY):
            ch = k * ARITY + i
            ok, key = bound(offsets[l - 1] + ch) if ch < sizes[l - 1] else (False, math.inf)
            ok = ok and not key > best[0]
            kids.append([key if ok else math.inf, ch if ok else -1])
        for p in range(ARITY):
            for i in range(p & 1, ARITY - 1, 2):
                if kids[i + 1][0] < kids[i][0]:
                    kids[i], kids[i + 1] = kids[i + 1], kids[i]
        for key, ch in reversed(kids):
            if ch >= 0:
                stack.append((l - 1, ch))
        assert len(stack) <= cap
    return nodes, evals


def dist_query(points, tree):
    """-> the dict of mesh_distance_ref.query plus nodes int64 [Q], evals int64 [Q]"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    v, f = tree["vertices"].astype(np.float64), tree["faces"]
    lo, hi, slack = tree["node_lo"].astype(np.float64).tolist(), tree["node_hi"].astype(np.float64).tolist(), float(tree["slack"])
    n = len(pts)
    out = dict(dist=np.full(n, np.inf, np.float32), closest=pts.copy(), face=np.full(n, -1, np.int32), region=np.full(n, DR.NO_REGION, np.uint8),
               d2=np.full(n, np.inf), nodes=np.zeros(n, np.int64), evals=np.zeros(n, np.int64))
    corners = [[v[f[i, c]].tolist() for c in range(3)] for i in range(len(f))] if n else []
    for qi in range(n):
        if not np.isfinite(pts[qi]).all():
            continue                                             # never enters the tree
        p = pts[qi].astype(np.float64).tolist()
        best, win = [math.inf], [-1, None, None]

        def bound(node):
            g = [max(max(lo[node][c] - p[c], p[c] - hi[node][c]) - slack, 0.0) for c in range(3)]
            return True, ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]) * MARGIN

        def visit(face):
            d2, q, region = DR.closest_pair_loop(p, *corners[face])
            if d2 < best[0] or (d2 == best[0] and face < win[0]):
                best[0], win[0], win[1], win[2] = d2, face, q, region

        out["nodes"][qi], out["evals"][qi] = _walk(tree, bound, visit, best)
        if win[0] >= 0:
            out["d2"][qi], out["face"][qi], out["region"][qi] = best[0], win[0], win[2]
            out["dist"][qi] = np.float32(np.sqrt(np.float64(best[0])))
            out["closest"][qi] = np.asarray(win[1], np.float64).astype(np.float32)
    return out


def ray_query(origins, directions, tree, t_min=0.0, t_max=math.inf, cull=None):
    """-> the dict of mesh_ray_ref.intersect plus nodes int64 [N], evals int64 [N]"""
    o32 = np.asarray(origins, np.float32).reshape(-1, 3)
    d32 = np.asarray(directions, np.float32).reshape(-1, 3)
    v, f = tree["vertices"].astype(np.float64), tree["faces"]
    lo, hi, slack = tree["node_lo"].astype(np.float64).tolist(), tree["node_hi"].astype(np.float64).tolist(), float(tree["slack"])
    t_min, t_max, mode = float(t_min), float(t_max), RR.CULL[cull]
    n = len(o32)
    out = dict(t=np.full(n, np.inf, np.float32), face=np.full(n, -1, np.int32), bary=np.zeros((n, 3), np.float32), point=o32.copy(),
               side=np.full(n, RR.MISS_SIDE, np.uint8), t64=np.full(n, np.inf), nodes=np.zeros(n, np.int64), evals=np.zeros(n, np.int64))
    corners = [[v[f[i, c]].tolist() for c in range(3)] for i in range(len(f))] if n else []
    for qi in range(n):
        o, d = o32[qi].astype(np.float64).tolist(), d32[qi].astype(np.float64).tolist()
        if not (np.isfinite(o32[qi]).all() and np.isfinite(d32[qi]).all() and (d32[qi] != 0).any()):
            continue
        best, win = [math.inf], [-1, None, None]

        def bound(node):
            t0, t1 = t_min, t_max
            for c in range(3):
                a, b = lo[node][c] - slack, hi[node][c] + slack
                if d[c] == 0.0:
                    if not (a <= o[c] <= b):
                        return False, t0
                else:
                    ta, tb = (a - o[c]) / d[c], (b - o[c]) / d[c]
                    t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
            return t0 <= t1, t0

        def visit(face):
            hit, t, uvw, det = RR.hit_pair_loop(o, d, *corners[face], t_min, t_max)
            if hit and ((mode == 1 and det < 0) or (mode == 2 and det > 0)):
                hit = False
            if hit and (t < best[0] or (t == best[0] and face < win[0])):
                best[0], win[0], win[1], win[2] = t, face, uvw, det

        out["nodes"][qi], out["evals"][qi] = _walk(tree, bound, visit, best)
        if win[0] >= 0:
            t, (U, V, W), det = best[0], win[1], win[2]
            out["t64"][qi], out["t"][qi], out["face"][qi] = t, np.float32(t), win[0]
            out["bary"][qi] = np.asarray([U / det, V / det, W / det], np.float64).astype(np.float32)
            out["point"][qi] = np.asarray([o[c] + t * d[c] for c in range(3)], np.float64).astype(np.float32)
            out["side"][qi] = 0 if det > 0 else 1
    return out
