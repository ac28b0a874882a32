#!/usr/bin/env python
"""Timing record of the mesh simplification (csrc/mesh_simplify.hip; mesh.cluster_vertices, mesh.simplify and the simplify_cell
argument of the extractors) on the pools of tools/bench_brick_mesh.py: 50 frames of 224x224 fused in one call into a 256^3 virtual
grid (0.93 M faces), then at half the voxel size into 512^3 (3.5 M faces), each simplified at cells of 2 and 4 voxels; and on the
per-frame sheets of the same frames (mesh.scene_mesh, unwelded), which it welds.  Rows per case: sp3_mesh_cluster alone
and sp3_mesh_cluster_faces alone with prepared buffers; mesh.simplify end to end; faces, vertices and GLB bytes before and after;
for scale, the host route a user had before -- positions and faces copied to the host, np.unique(axis=0) on the cell keys, np.add.at
for the sums (the vertex half of tests/mesh_simplify_ref.py), timed on this machine's CPU.  Times are medians of device events
around whole calls after warm-up, with their range (contention on the atomics varies from run to run), except the host route (wall
clock).  Nothing is asserted.  Writes the table to --out (profiles/mesh_simplify.txt is the committed record)."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from spann3r_amd import lib as L
from spann3r_amd import mesh as M
from tools.bench_fusion import ring_frames
from tools.bench_mesh_components import pool
from tools.bench_render import timed


def glb_bytes(m):
    with tempfile.TemporaryDirectory() as d:
        return M.write_glb(os.path.join(d, "m.glb"), m["vertices"], m["colors"], m["faces"], bounds=m["bounds"])


def host_route(m, cell, origin):
    """the vertex half on the host: copies, np.unique on the cell keys, np.add.at for the sums -> (seconds of the copy, of the rest, C)"""
    import mesh_simplify_ref as MS
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v, c = m["vertices"].cpu().numpy(), m["colors"].cpu().numpy().view(np.uint32).ravel()
    t1 = time.perf_counter()
    r = MS.cluster(v, cell, origin, c)
    return t1 - t0, time.perf_counter() - t1, r["n_clusters"]


def case(name, m, cell, origin, rows, host):
    def row(what, tm, extra=""):
        med, lo, hi, reps = tm
        rows.append("%-92s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (what, med, lo, hi, reps, extra))

    lib, dev = L.load(), m["vertices"].device
    verts, rgba, faces = m["vertices"].contiguous(), m["colors"].contiguous().reshape(-1).view(torch.int32), m["faces"].contiguous()
    nv, nf = verts.shape[0], faces.shape[0]
    rows.append("- %s: cell %.5f, V = %d, F = %d" % (name, cell, nv, nf))
    _, origin3 = M._grid(cell, origin, "bench")
    lv, lf = M._table_log2(nv), M._table_log2(nf)
    pos, col = torch.empty((nv, 3), dtype=torch.float32, device=dev), torch.empty(nv, dtype=torch.int32, device=dev)
    vc, info = torch.empty(nv, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.sp3_mesh_cluster_ws_bytes(nv, lv)), dtype=torch.uint8, device=dev)

    def cluster():
        L.check(lib.sp3_mesh_cluster(verts.data_ptr(), rgba.data_ptr(), nv, origin3, float(np.float32(cell)), lv, ws.data_ptr(), pos.data_ptr(),
                                     col.data_ptr(), vc.data_ptr(), info.data_ptr(), L.stream_ptr()), "sp3_mesh_cluster")

    a = timed(cluster)
    c = int(info.item())
    row("sp3_mesh_cluster alone (7 launches), prepared buffers, 2^%d slots" % lv, a,
        "%d clusters (%.1f vertices each); scratch %.1f MB; %.2f ns per vertex" % (c, nv / max(c, 1), ws.numel() / 1e6, 1e6 * a[0] / nv))
    out, finfo = torch.empty((nf, 3), dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    ws2 = torch.empty(int(lib.sp3_mesh_cluster_faces_ws_bytes(nf, lf)), dtype=torch.uint8, device=dev)

    def cluster_faces():
        L.check(lib.sp3_mesh_cluster_faces(faces.data_ptr(), nf, vc.data_ptr(), nv, 1, lf, ws2.data_ptr(), out.data_ptr(), finfo.data_ptr(),
                                           L.stream_ptr()), "sp3_mesh_cluster_faces")

    b = timed(cluster_faces)
    kept, invalid, collapsed, dup = finfo.cpu().tolist()
    row("sp3_mesh_cluster_faces alone (6 launches), dedup, prepared buffers, 2^%d slots" % lf, b,
        "%d kept, %d collapsed, %d duplicate, %d invalid; scratch %.1f MB; %.2f ns per face" % (kept, collapsed, dup, invalid, ws2.numel() / 1e6, 1e6 * b[0] / nf))
    del pos, col, vc, ws, out, ws2
    e = timed(lambda: M.simplify(m, cell, origin=origin))
    row("mesh.simplify end to end (both entry points, the read of the counts, vertex compaction)", e)
    s = M.simplify(m, cell, origin=origin)
    before, after = glb_bytes(m), glb_bytes(s) if s["faces"].shape[0] else 0
    rows.append("  faces %d -> %d (%.1f %%), vertices %d -> %d, GLB %d -> %d bytes (%.1f %%)" %
                (nf, s["faces"].shape[0], 100.0 * s["faces"].shape[0] / nf, nv, s["vertices"].shape[0], before, after, 100.0 * after / before))
    if host:
        t_copy, t_rest, c_host = host_route(m, cell, origin)
        rows.append("%-92s %10.3f ms  = copy %.3f ms + np.unique / np.add.at %.3f ms, once, wall clock, %d CPUs visible; %d clusters; %.1f x "
                    "sp3_mesh_cluster" % ("host route, vertices only: .cpu(), np.unique(axis=0) on the cell keys, np.add.at", 1e3 * (t_copy + t_rest),
                                          1e3 * t_copy, 1e3 * t_rest, os.cpu_count(), c_host, 1e3 * (t_copy + t_rest) / a[0]))


def sheets(frames):
    """the per-frame sheets of the frames: world pointmaps from depth and camera, then mesh.scene_mesh"""
    pts, cols, conf = [], [], []
    for f in frames:
        h, w = f["depth"].shape
        d = torch.from_numpy(f["depth"]).cuda().double()
        y, x = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float64), torch.arange(w, device="cuda", dtype=torch.float64), indexing="ij")
        cam = torch.stack([(x - f["cu"]) / f["fu"] * d, (y - f["cv"]) / f["fv"] * d, d], -1)
        P = torch.from_numpy(np.asarray(f["cam2world"], np.float64)).cuda()
        pts.append((cam @ P[:3, :3].T + P[:3, 3]).float())
        cols.append(torch.from_numpy(f["images"]).cuda())
        conf.append(torch.where(torch.from_numpy(f["valid"]).cuda() != 0, 5.0, 1.0).float())
    return M.scene_mesh(torch.stack(pts), torch.stack(cols), torch.stack(conf), 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0], help="cells in voxels")
    args = ap.parse_args()
    frames = ring_frames(args.frames, args.size, args.size)
    rows = ["Mesh simplification on the device (libspann3r_hip.so), device %s" % torch.cuda.get_device_name(0),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead, allocations and read-backs of a call "
            "included); the host route is one wall-clock run on this machine's CPU; the sums are not aggregated in the wave"]
    for n1 in args.dims:
        voxel = 2.4 / n1
        rows.append("--- %d frames of %dx%d fused in one call, voxel %.5f, a %d^3 virtual grid; extract_mesh(direct=True), then simplified from the volume's origin"
                    % (len(frames), args.size, args.size, voxel, n1))
        brick = pool(n1, frames)
        m = brick.extract_mesh(direct=True)
        row = timed(lambda: brick.extract_mesh(direct=True))
        rows.append("%-92s %10.3f ms  [%9.3f .. %9.3f] x%-3d" % (("extract_mesh(direct=True), for scale",) + tuple(row)))
        for k in args.cells:
            case("%g voxels" % k, m, k * voxel, brick.origin, rows, host=(k == args.cells[0]))
            rowk = timed(lambda: brick.extract_mesh(direct=True, simplify_cell=k * voxel))
            rows.append("%-92s %10.3f ms  [%9.3f .. %9.3f] x%-3d" % (("extract_mesh(direct=True, simplify_cell=%g voxels)" % k,) + tuple(rowk)))
        del brick, m
        torch.cuda.empty_cache()
    voxel = 2.4 / args.dims[0]
    rows.append("--- the per-frame sheets of the same %d frames (mesh.scene_mesh: x10 positions, unwelded), cells in voxels of the %d^3 grid"
                % (len(frames), args.dims[0]))
    scene = sheets(frames)
    for k in args.cells:
        case("sheets, %g voxels" % k, scene, k * voxel * M.SCALE, None, rows, host=(k == args.cells[0]))
    text = "\n".join(rows)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
