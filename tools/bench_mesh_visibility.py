#!/usr/bin/env python
"""Timing record of mesh visibility (include/spann3r_hip.h "Mesh visibility"; mesh.ray_mesh_occluded / vertex_visibility /
cull_to_views, evaluate.evaluate_meshes(cull_views=...)) on the pools of tools/bench_brick_mesh.py: 50 frames of 224x224 fused in
one call into a 256^3 virtual grid (0.93 M faces), then into 512^3 (3.5 M faces), extract_mesh(direct=True), with the 50 cameras of
the pool.  The route a user had before -- shadow rays materialised in torch, ray_mesh_intersect, a comparison -- and the new route
run in ONE process and every pair of results is compared for equality (a mismatch ends the run).  Rows per pool: vertex_visibility
through the grid and through the tree against that route (on --views of the cameras, the old route's ray building and peak memory
apart); ray_mesh_occluded against ray_mesh_intersect on incoherent rays, grid and tree, with cells / nodes and faces per ray of
both; cull_to_views end to end; evaluate_meshes with and without cull_views.  Times are medians of device events around whole calls
after warm-up, with their range.  Writes the table to --out (profiles/mesh_visibility.txt is the committed record)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from spann3r_amd import evaluate as E
from spann3r_amd import lib as L
from spann3r_amd import mesh as M
from spann3r_amd.fusion import camera_tables
from tools.bench_fusion import ring_frames
from tools.bench_mesh_components import pool
from tools.bench_render import timed


def old_rays(verts, K, P, size):
    """the parent's route, ray building: the frustum tests in torch fp64 and V x T origins and directions -> (inside bool [T, V], o, d fp32 [T V, 3])"""
    fk, w2c = camera_tables(K, P, len(P))
    W = torch.from_numpy(w2c.astype(np.float64).reshape(-1, 3, 4)).to(verts.device)
    q = verts.double()
    c = torch.einsum("tij,vj->tvi", W[:, :, :3], q) + W[:, None, :, 3]
    z = c[..., 2]
    f = torch.from_numpy(fk).to(verts.device)
    u = c[..., 0] / z * f[:, None, 0] + f[:, None, 2]
    v = c[..., 1] / z * f[:, None, 1] + f[:, None, 3]
    inside = (z > 0) & (u + 0.5 >= 0) & (u + 0.5 < size[1]) & (v + 0.5 >= 0) & (v + 0.5 < size[0])
    o = torch.from_numpy(P[:, :3, 3].astype(np.float32)).to(verts.device)[:, None, :].expand(-1, len(verts), -1)
    d = (q[None] - o.double()).float()
    return inside, o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()


def old_route(m, verts, K, P, size, bias, **acc):
    inside, o, d = old_rays(verts, K, P, size)
    hit = M.ray_mesh_intersect(o, d, m, t_max=1.0 - float(np.float32(bias)), **acc)["face"] >= 0
    return (inside & ~hit.reshape(inside.shape)).sum(0).int()


def case(m, frames, rows, ray_counts, nviews, samples):
    def row(what, tm, extra=""):
        med, lo, hi, reps = tm
        rows.append("%-100s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (what, med, lo, hi, reps, extra))

    dev = m["vertices"].device
    verts, faces = m["vertices"].contiguous(), m["faces"].contiguous()
    nv, nf = verts.shape[0], faces.shape[0]
    grid, bvh = M.TriangleGrid(m), M.TriangleBVH(m)
    rows.append("- V = %d, F = %d; grid %s, %.2f pairs per face; tree of %d levels, %d nodes" % (nv, nf, grid.dims, grid.pairs / nf, bvh.levels, bvh.level_offsets[-1]))
    K = np.stack([f["K"] for f in frames])
    P = np.stack([f["cam2world"] for f in frames])
    size = frames[0]["depth"].shape
    bias = 1e-3
    # ---- vertex_visibility against the parent's route, on the first `nviews` cameras (the old route holds V x T rays)
    k, p = K[:nviews], P[:nviews]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    want = old_route(m, verts, k, p, size, bias, grid=grid)
    peak_old = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    got = M.vertex_visibility(m, k, p, size, bias=bias, grid=grid, return_stats=True)
    peak_new = torch.cuda.max_memory_allocated() - base
    for name, acc in (("grid", dict(grid=grid)), ("tree", dict(bvh=bvh))):
        r = M.vertex_visibility(m, k, p, size, bias=bias, return_stats=True, **acc)
        if not (torch.equal(r["count"], want) and torch.equal(old_route(m, verts, k, p, size, bias, **acc), want)):
            raise SystemExit("vertex_visibility through the %s differs from the composition" % name)
        st = r["stats"]
        steps = st["cells_visited"] if name == "grid" else st["nodes_visited"]
        tn = timed(lambda: M.vertex_visibility(m, k, p, size, bias=bias, **acc))
        to = timed(lambda: old_route(m, verts, k, p, size, bias, **acc))
        row("mesh.vertex_visibility through the %s, %d views (1 launch)" % (name, nviews), tn,
            "%.2f ns per (vertex, view) pair; %.2f %s and %.2f faces per pair; %.1f %% of the pairs visible" %
            (1e6 * tn[0] / (nv * nviews), steps / (nv * nviews), "cells" if name == "grid" else "nodes", st["faces_evaluated"] / (nv * nviews),
             100.0 * float(r["count"].sum()) / (nv * nviews)))
        row("  the parent's route through the %s: rays in torch, ray_mesh_intersect, compare; EQUAL counts" % name, to, "%.1f x" % (to[0] / tn[0]))
    row("  the parent's route, building the %d shadow rays alone" % (nv * nviews), timed(lambda: old_rays(verts, k, p, size)),
        "peak device memory of the whole route %.1f MB against %.1f MB for vertex_visibility" % (peak_old / 2 ** 20, peak_new / 2 ** 20))
    if nviews < len(P):
        for name, acc in (("grid", dict(grid=grid)), ("tree", dict(bvh=bvh))):
            tn = timed(lambda: M.vertex_visibility(m, K, P, size, bias=bias, **acc))
            row("mesh.vertex_visibility through the %s, all %d views" % (name, len(P)), tn, "%.2f ns per pair" % (1e6 * tn[0] / (nv * len(P))))
        if not torch.equal(M.vertex_visibility(m, K, P, size, grid=grid)["count"], M.vertex_visibility(m, K, P, size, bvh=bvh)["count"]):
            raise SystemExit("vertex_visibility: grid and tree differ")
    # ---- ray_mesh_occluded against ray_mesh_intersect on incoherent rays
    lo, hi = verts.amin(0), verts.amax(0)
    for n in ray_counts:
        gen = torch.Generator(device=dev).manual_seed(1)
        o = (lo + (hi - lo) * torch.rand((n, 3), device=dev, generator=gen)).contiguous()
        d = torch.randn((n, 3), device=dev, generator=gen).contiguous()
        for name, acc, steps in (("grid", dict(grid=grid), "cells_visited"), ("tree", dict(bvh=bvh), "nodes_visited")):
            occ, sa = M.ray_mesh_occluded(o, d, m, return_stats=True, **acc)
            hit = M.ray_mesh_intersect(o, d, m, return_stats=True, **acc)
            if not torch.equal(occ, hit["face"] >= 0):
                raise SystemExit("ray_mesh_occluded through the %s differs from face >= 0" % name)
            ta = timed(lambda: M.ray_mesh_occluded(o, d, m, **acc))
            th = timed(lambda: M.ray_mesh_intersect(o, d, m, **acc))
            row("mesh.ray_mesh_occluded through the %s, %d incoherent rays" % (name, n), ta,
                "%.2f ns per ray; %.1f %s and %.1f faces per ray; %.1f %% occluded" %
                (1e6 * ta[0] / n, sa[steps] / n, steps.split("_")[0], sa["faces_evaluated"] / n, 100.0 * float(occ.float().mean())))
            row("  mesh.ray_mesh_intersect on the same rays (closest hit, five outputs); EQUAL to face >= 0", th,
                "%.2f x; %.1f %s and %.1f faces per ray" % (th[0] / ta[0], hit["stats"][steps] / n, steps.split("_")[0], hit["stats"]["faces_evaluated"] / n))
        del o, d
    # ---- cull_to_views and evaluate_meshes
    for name, acc in (("grid", dict()), ("tree", dict(bvh=True))):
        c = M.cull_to_views(m, K, P, size, mode="any", **acc)
        row("mesh.cull_to_views end to end (structure built inside, %d views, mode any), %s" % (len(P), name),
            timed(lambda: M.cull_to_views(m, K, P, size, **acc)),
            "%d of %d vertices seen, %d of %d faces kept" % (c["visibility"]["vertices_seen"], nv, c["visibility"]["faces_kept"], nf))
    simple = M.simplify(m, 2.0 * 2.4 / 256)
    cams = dict(intrinsics=K, cam2world=P, size=size)
    for exact in (False, True):
        t0 = timed(lambda: E.evaluate_meshes(simple, m, n_samples=samples, icp=False, exact=exact))
        t1 = timed(lambda: E.evaluate_meshes(simple, m, n_samples=samples, icp=False, exact=exact, cull_views=cams))
        r0 = E.evaluate_meshes(simple, m, n_samples=samples, icp=False, exact=exact)
        r1 = E.evaluate_meshes(simple, m, n_samples=samples, icp=False, exact=exact, cull_views=cams)
        row("evaluate_meshes(simplified at 2 voxels, the mesh), %d samples, icp=False, exact=%s" % (samples, exact), t0,
            "acc %.6f comp %.6f" % (r0["acc"], r0["comp"]))
        row("  the same with cull_views = the %d cameras" % len(P), t1,
            "acc %.6f comp %.6f; faces kept %d of %d and %d of %d" % (r1["acc"], r1["comp"], r1["pred_faces_kept"], simple["faces"].shape[0], r1["gt_faces_kept"], nf))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--rays", type=int, nargs="+", default=[200000, 1000000])
    ap.add_argument("--views", type=int, default=8, help="cameras of the rows that run the parent's route (it materialises V x T rays in fp64)")
    ap.add_argument("--samples", type=int, default=200000)
    args = ap.parse_args()
    frames = ring_frames(args.frames, args.size, args.size)
    rows = ["Mesh visibility on the device (%s), device %s" % (os.path.basename(L.LIB_PATH), torch.cuda.get_device_name(0)),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead, allocations and read-backs of a call included)"]
    for n1 in args.dims:
        voxel = 2.4 / n1
        rows.append("--- %d frames of %dx%d fused in one call, voxel %.5f, a %d^3 virtual grid; extract_mesh(direct=True)"
                    % (len(frames), args.size, args.size, voxel, n1))
        brick = pool(n1, frames)
        m = brick.extract_mesh(direct=True)
        del brick
        case(m, frames, rows, args.rays, min(args.views, len(frames)), args.samples)
        del m
        torch.cuda.empty_cache()
    text = "\n".join(rows)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
