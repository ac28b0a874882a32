#!/usr/bin/env python
"""Timing record of the exact point-to-mesh distance (csrc/mesh_distance.hip; mesh.TriangleGrid / point_mesh_distance,
evaluate.evaluate_meshes(exact=True)) on the pools of tools/bench_brick_mesh.py: 50 frames of 224x224 fused in one call into a 256^3
virtual grid (0.93 M faces), then at half the voxel size into 512^3 (3.5 M faces), extract_mesh(direct=True).  The queries are points
drawn by area from the mesh simplified at 2 voxels, measured against the full mesh -- what evaluate_meshes asks.  Rows per pool: the
grid build end to end and its two kernels alone; sp3_mesh_dist_query alone for 200 000 and 1 000 000 queries with prepared buffers
(query order included in the preparation), with the faces evaluated per query and the fallbacks of its counters, for every
--occupancy (mesh.FACES_PER_CELL first: the record the constant was chosen from); sp3_mesh_dist_brute alone on --brute queries;
evaluate_meshes with and without exact.  Times are medians of device events around whole calls after warm-up, with their range.
Nothing is asserted.  Writes the table to --out, or appends it with --append (profiles/mesh_distance.txt is the committed record)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from spann3r_amd import evaluate as E
from spann3r_amd import lib as L
from spann3r_amd import mesh as M
from tools.bench_fusion import ring_frames
from tools.bench_mesh_components import pool
from tools.bench_render import timed


def case(m, s, rows, samples, occupancies, brute_n):
    def row(what, tm, extra=""):
        med, lo, hi, reps = tm
        rows.append("%-92s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (what, med, lo, hi, reps, extra))

    lib, dev = L.load(), m["vertices"].device
    verts, faces = m["vertices"].contiguous(), m["faces"].contiguous()
    nv, nf = verts.shape[0], faces.shape[0]
    rows.append("- V = %d, F = %d; queries drawn from the mesh simplified at 2 voxels (F = %d)" % (nv, nf, s["faces"].shape[0]))
    default = M.FACES_PER_CELL
    for occ in occupancies:
        M.FACES_PER_CELL = occ
        tag = "FACES_PER_CELL %g%s" % (occ, " (the default)" if occ == default else "")
        grid = M.TriangleGrid(m)
        row("mesh.TriangleGrid end to end (count, cumsum, fill, sort, searchsorted; host reads), %s" % tag, timed(lambda: M.TriangleGrid(m)),
            "grid %s h %.5f, %d pairs = %.2f per face, %d tries" % (grid.dims, grid.h, grid.pairs, grid.pairs / nf, grid.tries))
        if occ == default:
            counts = torch.empty(nf, dtype=torch.int64, device=dev)
            tc = timed(lambda: L.check(lib.sp3_mesh_tri_cell_count(verts.data_ptr(), nv, faces.data_ptr(), nf, C.byref(grid.g), counts.data_ptr(),
                                                                   L.stream_ptr()), "sp3_mesh_tri_cell_count"))
            row("sp3_mesh_tri_cell_count alone (1 launch)", tc, "%.2f ns per face" % (1e6 * tc[0] / nf))
            offsets = torch.cumsum(counts, 0) - counts
            cell, face = torch.empty(grid.pairs, dtype=torch.int32, device=dev), torch.empty(grid.pairs, dtype=torch.int32, device=dev)
            row("sp3_mesh_tri_cell_fill alone (1 launch)", timed(lambda: L.check(lib.sp3_mesh_tri_cell_fill(
                verts.data_ptr(), nv, faces.data_ptr(), nf, C.byref(grid.g), offsets.data_ptr(), grid.pairs, cell.data_ptr(), face.data_ptr(),
                L.stream_ptr()), "fill")))
            del counts, offsets, cell, face
        for n in samples:
            q = M.sample_surface(s, n, seed=0)["points"]
            order = grid.query_order(q)
            ws = torch.empty(int(lib.sp3_mesh_dist_query_ws_bytes(n)), dtype=torch.uint8, device=dev)
            dist, closest = torch.empty(n, dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev)
            fidx, region = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)

            def query():
                L.check(lib.sp3_mesh_dist_query(q.data_ptr(), order.data_ptr(), n, verts.data_ptr(), nv, faces.data_ptr(), nf, grid.pair_face.data_ptr(),
                                                grid.pairs, grid.cell_start.data_ptr(), C.byref(grid.g), M.DIST_RING_BUDGET, ws.data_ptr(),
                                                dist.data_ptr(), closest.data_ptr(), fidx.data_ptr(), region.data_ptr(), L.stream_ptr()),
                        "sp3_mesh_dist_query")

            tm = timed(query)
            st = M.point_mesh_distance(q, m, grid=grid, return_stats=True)["stats"]
            row("sp3_mesh_dist_query alone (grid walk + 3 fallback launches), %d queries, %s" % (n, tag), tm,
                "%.2f ns per query; %.1f faces evaluated and %.1f cells visited per query, %d fallbacks; mean dist %.6f" %
                (1e6 * tm[0] / n, st["faces_evaluated"] / n, st["cells_visited"] / n, st["fallback_queries"], float(dist.mean())))
            if occ == default:
                row("mesh.point_mesh_distance end to end on a built grid, %d queries (query order, allocations)" % n,
                    timed(lambda: M.point_mesh_distance(q, m, grid=grid)))
            del q, order, ws, dist, closest, fidx, region
        del grid
    M.FACES_PER_CELL = default
    if brute_n:
        q = M.sample_surface(s, brute_n, seed=0)["points"]
        tm = timed(lambda: M.point_mesh_distance(q, m, method="brute"), budget=3.0)
        row("mesh.point_mesh_distance(method='brute') (2 passes + finish), %d queries x %d faces" % (brute_n, nf), tm,
            "%.3f ns per (query, face) pair and pass" % (1e6 * tm[0] / (2.0 * brute_n * nf)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--samples", type=int, nargs="+", default=[200000, 1000000])
    ap.add_argument("--occupancy", type=float, nargs="+", default=[M.FACES_PER_CELL])
    ap.add_argument("--brute", type=int, default=4096, metavar="N", help="queries of the brute-force row (0: none)")
    args = ap.parse_args()
    frames = ring_frames(args.frames, args.size, args.size)
    rows = ["Exact point-to-mesh distance on the device (%s), device %s" % (os.path.basename(L.LIB_PATH), torch.cuda.get_device_name(0)),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead, allocations and read-backs of a call included)"]
    for n1 in args.dims:
        voxel = 2.4 / n1
        rows.append("--- %d frames of %dx%d fused in one call, voxel %.5f, a %d^3 virtual grid; extract_mesh(direct=True)"
                    % (len(frames), args.size, args.size, voxel, n1))
        brick = pool(n1, frames)
        m = brick.extract_mesh(direct=True)
        s = M.simplify(m, 2 * voxel, origin=brick.origin)
        case(m, s, rows, args.samples, args.occupancy, args.brute if n1 == args.dims[0] else 0)
        for exact in (False, True):
            for icp in (False, True):
                tm = timed(lambda: E.evaluate_meshes(s, m, n_samples=200000, icp=icp, exact=exact), budget=3.0)
                r = E.evaluate_meshes(s, m, n_samples=200000, icp=icp, exact=exact)
                rows.append("%-92s %10.3f ms  [%9.3f .. %9.3f] x%-3d acc %.6f comp %.6f nc1 %.4f nc2 %.4f" %
                            (("evaluate_meshes(simplified at 2 voxels, the mesh), 200000 samples each, icp=%s, exact=%s" % (icp, exact),) + tuple(tm) +
                             (r["acc"], r["comp"], r["nc1"], r["nc2"])))
        del brick, m, s
        torch.cuda.empty_cache()
    text = "\n".join(rows)
    print(text)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
