#!/usr/bin/env python
"""Timing record of the mesh BVH (csrc/mesh_bvh.hip; mesh.TriangleBVH and the bvh= keyword) NEXT TO the uniform grid, both in one
process, on the pools of tools/bench_brick_mesh.py: 50 frames of 224x224 fused in one call into a 256^3 virtual grid (0.93 M
faces), then at half the voxel size into 512^3 (3.5 M faces), extract_mesh(direct=True).  Rows per pool, every one for the grid and
for the tree: the build end to end; mesh.point_mesh_distance on the built structure for near queries (points drawn by area from
the mesh simplified at 2 voxels: what evaluate_meshes asks) and for the same points displaced along z by 0.05, 0.2 and 1 scene
extents -- which the grid hands to its brute-force kernels (the second pool runs only the first count of --far: 200 000
displaced queries against 3.5 M faces take the grid seconds per call); mesh.render_depth_maps for the 50 cameras of the pool and for one
1920x1080 view; with the nodes (cells) visited and the faces evaluated per query.  Last, the per-frame sheets of the frames
(mesh.scene_mesh: faces stretched over depth edges among small ones) with the tries of TriangleGrid.  Times are medians of device
events around whole calls after warm-up, with their range.  Every pair of results is compared (torch.equal) and the outcome
printed; nothing is asserted.  Writes the table to --out (profiles/mesh_bvh.txt is the committed record)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from spann3r_amd import cell_grid as G
from spann3r_amd import lib as L
from spann3r_amd import mesh as M
from tools.bench_fusion import ring_frames
from tools.bench_mesh_components import pool
from tools.bench_mesh_simplify import sheets
from tools.bench_render import timed


def _row(rows, what, tm, extra=""):
    med, lo, hi, reps = tm
    rows.append("%-100s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (what, med, lo, hi, reps, extra))
    print(rows[-1], flush=True)


def _equal(a, b, keys):
    return all(torch.equal(a[k].view(torch.uint8) if a[k].dtype == torch.uint8 else a[k].view(torch.int32), b[k].view(torch.uint8)
                           if b[k].dtype == torch.uint8 else b[k].view(torch.int32)) for k in keys)


def builds(m, rows):
    nf = m["faces"].shape[0]
    grid, bvh = M.TriangleGrid(m), M.TriangleBVH(m)
    _row(rows, "mesh.TriangleGrid end to end", timed(lambda: M.TriangleGrid(m)),
         "grid %s h %.5f, %d pairs = %.2f per face, %d tries" % (grid.dims, grid.h, grid.pairs, grid.pairs / nf, grid.tries))
    _row(rows, "mesh.TriangleBVH end to end (keys, sort, %d level launches; host reads)" % bvh.levels, timed(lambda: M.TriangleBVH(m)),
         "%d usable faces, %d levels, %d nodes, LEAF %d ARITY %d, stack %d entries" %
         (bvh.usable, bvh.levels, bvh.level_offsets[-1], G.BVH_LEAF, G.BVH_ARITY, (G.BVH_ARITY - 1) * (bvh.levels - 1) + 1))
    return grid, bvh


def distance_rows(m, grid, bvh, q, tag, rows, budget=1.0):
    n = q.shape[0]
    rg = M.point_mesh_distance(q, m, grid=grid, return_stats=True)
    rb = M.point_mesh_distance(q, m, bvh=bvh, return_stats=True)
    same = _equal(rg, rb, ("dist", "closest", "face", "region"))
    tg = timed(lambda: M.point_mesh_distance(q, m, grid=grid), budget=budget)
    _row(rows, "point_mesh_distance on the built GRID, %d queries %s" % (n, tag), tg,
         "%.2f ns per query; %.1f cells visited and %.1f faces evaluated per query, %d fallbacks" %
         (1e6 * tg[0] / n, rg["stats"]["cells_visited"] / n, rg["stats"]["faces_evaluated"] / n, rg["stats"]["fallback_queries"]))
    tb = timed(lambda: M.point_mesh_distance(q, m, bvh=bvh), budget=budget)
    _row(rows, "point_mesh_distance on the built TREE, %d queries %s" % (n, tag), tb,
         "%.2f ns per query; %.1f nodes visited and %.1f faces evaluated per query; %s the grid's result; grid / tree = %.2f" %
         (1e6 * tb[0] / n, rb["stats"]["nodes_visited"] / n, rb["stats"]["faces_evaluated"] / n, "bit-equal to" if same else "DIFFERS FROM", tg[0] / tb[0]))


def case(m, s, frames, rows, samples, far_counts, shifts, big):
    verts = m["vertices"]
    rows.append("- V = %d, F = %d; near queries drawn from the mesh simplified at 2 voxels (F = %d)" % (verts.shape[0], m["faces"].shape[0], s["faces"].shape[0]))
    grid, bvh = builds(m, rows)
    extent = float((verts.amax(0) - verts.amin(0)).max())
    for n in samples:
        distance_rows(m, grid, bvh, M.sample_surface(s, n, seed=0)["points"], "near the surface", rows)
    for shift in shifts:
        for n in far_counts:
            q = (M.sample_surface(s, n, seed=0)["points"] + torch.tensor([0.0, 0.0, shift * extent], device=verts.device)).contiguous()
            distance_rows(m, grid, bvh, q, "displaced by %g scene extents (%.3f)" % (shift, shift * extent), rows, budget=0.5)
    K = np.stack([f["K"] for f in frames])
    P = np.stack([f["cam2world"] for f in frames])
    h, w = frames[0]["depth"].shape
    bh, bw = big
    Kb = np.array([[0.9 * bw, 0, (bw - 1) / 2], [0, 0.9 * bw, (bh - 1) / 2], [0, 0, 1]])
    for name, k, p, size in (("%d views of %dx%d" % (len(frames), w, h), K, P, (h, w)), ("one %dx%d view" % (bw, bh), Kb, P[:1], (bh, bw))):
        nray = len(p) * size[0] * size[1]
        rg = M.render_depth_maps(m, k, p, size, grid=grid, return_faces=True, return_stats=True)
        rb = M.render_depth_maps(m, k, p, size, bvh=bvh, return_faces=True, return_stats=True)
        same = _equal(rg, rb, ("depth", "face", "bary"))
        tg = timed(lambda: M.render_depth_maps(m, k, p, size, grid=grid))
        _row(rows, "render_depth_maps on the built GRID (sp3_mesh_ray_views), %s" % name, tg,
             "%.2f ns per ray; %.1f cells visited and %.1f faces evaluated per ray; %.1f %% of the rays hit" %
             (1e6 * tg[0] / nray, rg["stats"]["cells_visited"] / nray, rg["stats"]["faces_evaluated"] / nray, 100.0 * float((rg["depth"] > 0).float().mean())))
        tb = timed(lambda: M.render_depth_maps(m, k, p, size, bvh=bvh))
        _row(rows, "render_depth_maps on the built TREE (sp3_mesh_bvh_ray_views), %s" % name, tb,
             "%.2f ns per ray; %.1f nodes visited and %.1f faces evaluated per ray; %s the grid's maps; grid / tree = %.2f" %
             (1e6 * tb[0] / nray, rb["stats"]["nodes_visited"] / nray, rb["stats"]["faces_evaluated"] / nray, "bit-equal to" if same else "DIFFER FROM", tg[0] / tb[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--samples", type=int, nargs="+", default=[200000, 1000000])
    ap.add_argument("--far", type=int, nargs="+", default=[4096, 200000], help="query counts of the displaced rows")
    ap.add_argument("--shift", type=float, nargs="+", default=[0.05, 0.2, 1.0], help="displacements in scene extents")
    ap.add_argument("--big", type=int, nargs=2, default=[1080, 1920], metavar=("H", "W"))
    ap.add_argument("--no_sheets", action="store_true")
    args = ap.parse_args()
    frames = ring_frames(args.frames, args.size, args.size)
    rows = ["Mesh BVH next to the uniform grid on the device (%s), device %s" % (os.path.basename(L.LIB_PATH), torch.cuda.get_device_name(0)),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead, query order, allocations and read-backs of a call included)"]
    for n1 in args.dims:
        voxel = 2.4 / n1
        rows.append("--- %d frames of %dx%d fused in one call, voxel %.5f, a %d^3 virtual grid; extract_mesh(direct=True)"
                    % (len(frames), args.size, args.size, voxel, n1))
        brick = pool(n1, frames)
        m = brick.extract_mesh(direct=True)
        s = M.simplify(m, 2 * voxel, origin=brick.origin)
        case(m, s, frames, rows, args.samples, args.far if n1 == args.dims[0] else args.far[:1], args.shift, tuple(args.big))
        del brick, m, s
        torch.cuda.empty_cache()
    if not args.no_sheets:
        m = sheets(frames)
        rows.append("--- the per-frame sheets of the %d frames (mesh.scene_mesh): V = %d, F = %d" % (len(frames), m["vertices"].shape[0], m["faces"].shape[0]))
        grid, bvh = builds(m, rows)
        distance_rows(m, grid, bvh, M.sample_surface(m, 200000, seed=0)["points"], "drawn from the sheets themselves", rows)
    text = "\n".join(rows)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
