"""The host half of the uniform cell grid of the exact searches (csrc/cell_grid.h states the rule; include/spann3r_hip.h sp3_nn_grid):
the cell edge and dims, the descriptor with its slack, the cell-start table of items sorted by cell, the order queries are served in
and the counters a query leaves in its workspace.  evaluate.CellGrid (points) and mesh.TriangleGrid (faces) are built from these."""
import ctypes as C
import math

import numpy as np
import torch

from . import lib as L

MAX_CELLS = 1 << 22
OCCUPANCY = 4.0          # mean points per cell the edge length aims for


def one_cell():      # a fresh descriptor each time: everything in one cell, what the brute-force kernels stand for
    return L.NnGrid(0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1, 1, 1)


def grow_to_cap(ext, h, max_cells=MAX_CELLS):
    """the dims of the extents `ext` at cell edge h, h grown by 1.25 until the cell cap holds -> (h, (nx, ny, nz))"""
    while True:
        dims = tuple(int(math.floor(e / h)) + 1 for e in ext)
        if dims[0] * dims[1] * dims[2] <= max_cells:
            return h, dims
        h *= 1.25


def choose_grid(lo, hi, n, occupancy=OCCUPANCY, max_cells=MAX_CELLS):
    """Cell edge and dims for n points in the box [lo, hi] (host, float64) -> (h, (nx, ny, nz)).
    h aims at `occupancy` points per cell over the axes the cloud really extends along: an axis thinner than h holds one cell and
    leaves the volume (planar, collinear and single-point clouds), every extent is floored, and h grows until the cell cap holds."""
    ext = np.maximum(np.asarray(hi, np.float64) - np.asarray(lo, np.float64), 0.0)
    emax = float(ext.max())
    if not np.isfinite(emax) or emax <= 0.0:
        return 1.0, (1, 1, 1)
    floored = np.maximum(ext, 1e-6 * emax)
    active = [0, 1, 2]
    h = emax
    while active:
        h = float((np.prod(floored[active]) * occupancy / max(n, 1)) ** (1.0 / len(active)))
        thin = [a for a in active if floored[a] < h]
        if not thin:
            break
        active = [a for a in active if a not in thin]
    if not active:
        h = 2.0 * emax                               # fewer points than `occupancy`: one cell
    h = max(h, 1e-30, emax * 2.0 ** -20)
    return grow_to_cap(ext, h, max_cells)


def finite_box(lo, hi):
    """device [3] minimum and maximum -> float64 numpy [2, 3] on the host, non-finite entries 0 (one 48-byte read)"""
    box = torch.stack((lo, hi)).double().cpu().numpy()
    return np.where(np.isfinite(box), box, 0.0)


def make_grid(box, h, dims):
    """the descriptor of the grid of `dims` cells of edge h whose origin is box[0]; the slack covers the fp32 rounding of a cell
    assignment anywhere in the box"""
    slack = 1e-6 * (float(np.abs(box).max()) + float((box[1] - box[0]).max()) + h)
    return L.NnGrid(float(box[0, 0]), float(box[0, 1]), float(box[0, 2]), h, 1.0 / h, slack, *dims)


# ---- the implicit tree of mesh.TriangleBVH (include/spann3r_hip.h "Mesh BVH"; csrc/mesh_bvh.hip holds the same two constants)
BVH_LEAF = 4             # faces per leaf node
BVH_ARITY = 4            # children per node


def bvh_levels(usable, leaf=BVH_LEAF, arity=BVH_ARITY):
    """the level table of a tree over `usable` >= 1 faces -> (sizes, offsets): sizes[0] = ceil(usable / leaf) leaf nodes, every
    level the ceiling quotient of the one below by `arity` until one node is left; level l is stored at offsets[l] .. offsets[l + 1]"""
    if usable < 1:
        raise ValueError("bvh_levels: %d faces: a tree needs one at least" % usable)
    sizes = [-(-usable // leaf)]
    while sizes[-1] > 1:
        sizes.append(-(-sizes[-1] // arity))
    offsets = [0]
    for n in sizes:
        offsets.append(offsets[-1] + n)
    return sizes, offsets


def bvh_slack(box):
    """make_grid's slack without its h term: what the boxes of a tree are pushed out by"""
    return 1e-6 * (float(np.abs(box).max()) + float((box[1] - box[0]).max()))


def make_bvh(box, usable):
    """the descriptor of the tree over `usable` faces in the box of the finite vertices"""
    sizes, offsets = bvh_levels(usable)
    if len(sizes) > L.MeshBvh.MAX_LEVELS:
        raise ValueError("make_bvh: %d levels for %d faces: more than the %d the descriptor holds" % (len(sizes), usable, L.MeshBvh.MAX_LEVELS))
    b = L.MeshBvh(usable=usable, leaves=sizes[0], levels=len(sizes), slack=bvh_slack(box))
    b.level_off[:len(offsets)] = offsets
    return b, sizes, offsets


def cell_table(ids, ncell):
    """cell ids (any integer tensor, values in 0..ncell-1) -> (order, cell_start): the stable order that sorts the items by cell,
    and int32 [ncell + 1] with the sorted items of cell c at cell_start[c] .. cell_start[c + 1] - 1"""
    sorted_ids, order = torch.sort(ids, stable=True)
    cells = torch.arange(ncell + 1, dtype=sorted_ids.dtype, device=ids.device)
    return order, torch.searchsorted(sorted_ids, cells).to(torch.int32)


def read_head(ws):
    """the 32-byte head of a query workspace -> (fallback queries, cells visited, items looked at); one host read"""
    head = ws[:32].cpu().numpy()
    return (int(head[:4].view(np.int32)[0]),) + tuple(int(x) for x in head[16:32].view(np.uint64))


class Grid:
    """what CellGrid and TriangleGrid share: the descriptor `g`"""

    def query_order(self, q):
        """the queries sorted by the cell they fall in (clamped into the grid): the lanes of a wave then walk the same cells"""
        ids = torch.empty(q.shape[0], dtype=torch.int32, device=q.device)
        L.check(L.load().sp3_nn_cell_ids(q.data_ptr(), q.shape[0], C.byref(self.g), ids.data_ptr(), L.stream_ptr()), "sp3_nn_cell_ids")
        return torch.sort(ids, stable=True)[1]
