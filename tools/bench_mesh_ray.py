#!/usr/bin/env python
"""Timing record of the ray queries on a mesh (csrc/mesh_ray.hip; mesh.ray_mesh_intersect / render_depth_maps) on the pools of
tools/bench_brick_mesh.py: 50 frames of 224x224 fused in one call into a 256^3 virtual grid (0.93 M faces), then at half the voxel
size into 512^3 (3.5 M faces), extract_mesh(direct=True), both in one process.  Rows per pool: mesh.TriangleGrid, built once and
reused; sp3_mesh_ray_views (render_depth_maps on the built grid) for the 50 cameras of the pool at 224x224 and for one 1920x1080
view, with the cells visited and faces evaluated per ray and the share of rays that hit; next to them BrickTSDFVolume.raycast of the
volume the mesh came from for the same cameras, and the picture rasteriser (PointRenderer.add_triangles + image(return_depth=True),
one camera per buffer) for the large view; the 50-view render again on grids of --h_scale times the cell edge that
mesh.FACES_PER_CELL, chosen for distance queries, gives; mesh.ray_mesh_intersect for 200 000 and 1 000 000 incoherent rays (random origins in the
box, random directions), rays served sorted by the cell of their origin (the default) and unsorted (sp3_mesh_ray_query with no
order); the brute-force route on --brute rays.  Times are medians of device events around whole calls after warm-up, with their
range.  Nothing is asserted.  Writes the table to --out (profiles/mesh_ray.txt is the committed record)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from spann3r_amd import lib as L
from spann3r_amd import mesh as M
from spann3r_amd import vis
from tools.bench_fusion import ring_frames
from tools.bench_mesh_components import pool
from tools.bench_render import timed


def case(m, brick, frames, rows, ray_counts, brute_n, big, h_scales):
    def row(what, tm, extra=""):
        med, lo, hi, reps = tm
        rows.append("%-96s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (what, med, lo, hi, reps, extra))

    lib, dev = L.load(), m["vertices"].device
    verts, faces = m["vertices"].contiguous(), m["faces"].contiguous()
    nv, nf = verts.shape[0], faces.shape[0]
    grid = M.TriangleGrid(m)
    rows.append("- V = %d, F = %d; grid %s h %.5f, %d pairs = %.2f per face (FACES_PER_CELL %g)" %
                (nv, nf, grid.dims, grid.h, grid.pairs, grid.pairs / nf, M.FACES_PER_CELL))
    row("mesh.TriangleGrid end to end, built once and reused below", timed(lambda: M.TriangleGrid(m)))
    K = np.stack([f["K"] for f in frames])
    P = np.stack([f["cam2world"] for f in frames])
    h, w = frames[0]["depth"].shape
    bh, bw = big
    Kb = np.array([[0.9 * bw, 0, (bw - 1) / 2], [0, 0.9 * bw, (bh - 1) / 2], [0, 0, 1]])
    for name, k, p, size in (("%d views of %dx%d" % (len(frames), w, h), K, P, (h, w)), ("one %dx%d view" % (bw, bh), Kb, P[:1], (bh, bw))):
        nray = len(p) * size[0] * size[1]
        tm = timed(lambda: M.render_depth_maps(m, k, p, size, grid=grid))
        r = M.render_depth_maps(m, k, p, size, grid=grid, return_stats=True)
        st = r["stats"]
        row("mesh.render_depth_maps on the built grid (sp3_mesh_ray_views, 1 launch), %s" % name, tm,
            "%.2f ns per ray; %.1f cells visited and %.1f faces evaluated per ray; %.1f %% of the rays hit" %
            (1e6 * tm[0] / nray, st["cells_visited"] / nray, st["faces_evaluated"] / nray, 100.0 * float((r["depth"] > 0).float().mean())))
        tf = timed(lambda: M.render_depth_maps(m, k, p, size, grid=grid, return_faces=True))
        row("  the same with the face and bary maps", tf)
        tv = timed(lambda: brick.raycast(k, p, size, vertices=False, normals=False, colors=False))
        dv = brick.raycast(k, p, size, vertices=False, normals=False, colors=False)["depth"]
        both = (dv > 0) & (r["depth"] > 0)
        row("  BrickTSDFVolume.raycast of the volume the mesh came from (depth only), %s" % name, tv,
            "%.2f ns per ray; %.1f %% of the rays hit; median |mesh depth - volume depth| where both hit %.2e" %
            (1e6 * tv[0] / nray, 100.0 * float((dv > 0).float().mean()), float((dv - r["depth"])[both].abs().median()) if bool(both.any()) else float("nan")))
    for scale in h_scales:                                            # the cell edge the distance queries chose, against larger ones
        gs = M.TriangleGrid(m, h=grid.h * scale)
        tm = timed(lambda: M.render_depth_maps(m, K, P, (h, w), grid=gs))
        st = M.render_depth_maps(m, K, P, (h, w), grid=gs, return_stats=True)["stats"]
        nray = len(P) * h * w
        row("  mesh.render_depth_maps, %d views of %dx%d, on TriangleGrid(m, h=%g x the default's)" % (len(P), w, h, scale), tm,
            "grid %s, %.2f pairs per face; %.1f cells visited and %.1f faces evaluated per ray" %
            (gs.dims, gs.pairs / nf, st["cells_visited"] / nray, st["faces_evaluated"] / nray))
        del gs
    cam = vis.Camera(Kb, np.linalg.inv(P[0]), bw, bh)
    ren = vis.PointRenderer(camera=cam)
    colors = m["colors"]

    def raster():
        ren.clear()
        ren.add_triangles(verts, faces, colors)
        return ren.image(return_depth=True)

    tr = timed(raster)
    dr = raster()[1]
    row("  PointRenderer.add_triangles + image(return_depth=True) (fp32 edge functions, one camera per buffer), one %dx%d view" % (bw, bh), tr,
        "%.1f %% of the pixels covered" % (100.0 * float(torch.isfinite(dr).float().mean())))
    lo, hi = verts.amin(0), verts.amax(0)
    for n in ray_counts:
        gen = torch.Generator(device=dev).manual_seed(1)
        o = (lo + (hi - lo) * torch.rand((n, 3), device=dev, generator=gen)).contiguous()
        d = torch.randn((n, 3), device=dev, generator=gen).contiguous()
        order = grid.query_order(o)
        ws = torch.empty(int(lib.sp3_mesh_ray_ws_bytes(n)), dtype=torch.uint8, device=dev)
        out = dict(t=torch.empty(n, dtype=torch.float32, device=dev), face=torch.empty(n, dtype=torch.int32, device=dev),
                   bary=torch.empty((n, 3), dtype=torch.float32, device=dev), point=torch.empty((n, 3), dtype=torch.float32, device=dev),
                   side=torch.empty(n, dtype=torch.uint8, device=dev))

        def query(order_ptr):
            L.check(lib.sp3_mesh_ray_query(o.data_ptr(), d.data_ptr(), order_ptr, n, verts.data_ptr(), nv, faces.data_ptr(), nf,
                                           grid.pair_face.data_ptr(), grid.pairs, grid.cell_start.data_ptr(), C.byref(grid.g), 0.0, float("inf"), 0,
                                           ws.data_ptr(), out["t"].data_ptr(), out["face"].data_ptr(), out["bary"].data_ptr(),
                                           out["point"].data_ptr(), out["side"].data_ptr(), L.stream_ptr()), "sp3_mesh_ray_query")

        st = M.ray_mesh_intersect(o, d, m, grid=grid, return_stats=True)
        for tag, ptr in (("sorted by the cell of the origin", order.data_ptr()), ("unsorted", None)):
            tm = timed(lambda: query(ptr))
            row("sp3_mesh_ray_query alone (1 launch), %d incoherent rays, %s" % (n, tag), tm,
                "%.2f ns per ray; %.1f cells visited and %.1f faces evaluated per ray; %.1f %% hit" %
                (1e6 * tm[0] / n, st["stats"]["cells_visited"] / n, st["stats"]["faces_evaluated"] / n, 100.0 * float((st["face"] >= 0).float().mean())))
        row("mesh.ray_mesh_intersect end to end on the built grid, %d rays (query order, allocations)" % n,
            timed(lambda: M.ray_mesh_intersect(o, d, m, grid=grid)))
        del o, d, order, ws, out, st
    if brute_n:
        gen = torch.Generator(device=dev).manual_seed(2)
        o = (lo + (hi - lo) * torch.rand((brute_n, 3), device=dev, generator=gen)).contiguous()
        d = torch.randn((brute_n, 3), device=dev, generator=gen).contiguous()
        tm = timed(lambda: M.ray_mesh_intersect(o, d, m, method="brute"), budget=3.0)
        row("mesh.ray_mesh_intersect(method='brute') (2 passes + finish), %d rays x %d faces" % (brute_n, nf), tm,
            "%.2f ps per (ray, face) pair and pass" % (1e9 * tm[0] / (2.0 * brute_n * nf)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--rays", type=int, nargs="+", default=[200000, 1000000])
    ap.add_argument("--big", type=int, nargs=2, default=[1080, 1920], metavar=("H", "W"))
    ap.add_argument("--h_scale", type=float, nargs="*", default=[2.0, 4.0], help="extra rows of the 50-view render on grids of a larger cell edge")
    ap.add_argument("--brute", type=int, default=4096, metavar="N", help="rays of the brute-force row (0: none)")
    args = ap.parse_args()
    frames = ring_frames(args.frames, args.size, args.size)
    rows = ["Ray queries on a mesh on the device (%s), device %s" % (os.path.basename(L.LIB_PATH), torch.cuda.get_device_name(0)),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead, allocations and read-backs of a call included)"]
    for n1 in args.dims:
        voxel = 2.4 / n1
        rows.append("--- %d frames of %dx%d fused in one call, voxel %.5f, a %d^3 virtual grid; extract_mesh(direct=True)"
                    % (len(frames), args.size, args.size, voxel, n1))
        brick = pool(n1, frames)
        m = brick.extract_mesh(direct=True)
        case(m, brick, frames, rows, args.rays, args.brute if n1 == args.dims[0] else 0, tuple(args.big), args.h_scale)
        del brick, m
        torch.cuda.empty_cache()
    text = "\n".join(rows)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
