#!/usr/bin/env python
"""Timing record of the mesh surface sampling and normals (csrc/mesh_sample.hip; mesh.face_frames / sample_surface / vertex_normals,
evaluate.evaluate_meshes) on the pools of tools/bench_brick_mesh.py: 50 frames of 224x224 fused in one call into a 256^3 virtual
grid (0.93 M faces), then at half the voxel size into 512^3 (3.5 M faces), extract_mesh(direct=True).  Rows per pool:
sp3_mesh_face_frames alone, sp3_mesh_sample alone for 200 000 and 1 000 000 samples and sp3_mesh_vertex_normals alone, with prepared
buffers; mesh.sample_surface and evaluate.evaluate_meshes (the mesh against itself simplified at 2 voxels) end to end; for scale, the
host route a user had before -- positions, colours and faces copied to the host, numpy cross products, cumsum, searchsorted and
np.add.at (tests/mesh_sample_ref.py), timed on this machine's CPU.  Times are medians of device events around whole calls after
warm-up, with their range, except the host route (wall clock).  Nothing is asserted.  --sample-only LABEL times the sampler alone
and labels its rows: for a library variant (python -m spann3r_amd.build --variant NAME ...) selected with SP3_LIB_PATH; the
two-level search of the record was one, measured the same as the plain search and was dropped.  Writes the table to --out, or
appends it with --append (profiles/mesh_sample.txt is the committed record)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from spann3r_amd import evaluate as E
from spann3r_amd import lib as L
from spann3r_amd import mesh as M
from tools.bench_fusion import ring_frames
from tools.bench_mesh_components import pool
from tools.bench_render import timed


def host_route(m, n):
    """(seconds of the copy, of frames + n samples, of the vertex normals) on the host"""
    import mesh_sample_ref as R
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v, c, f = m["vertices"].cpu().numpy(), m["colors"].cpu().numpy().view(np.uint32).ravel(), m["faces"].cpu().numpy()
    t1 = time.perf_counter()
    fr = R.face_frames(v, f)
    R.sample(v, c, f, n, 0, frames=fr)
    t2 = time.perf_counter()
    R.vertex_normals(v, f, frames=fr)
    return t1 - t0, t2 - t1, time.perf_counter() - t2


def case(m, rows, sample_only, label, samples):
    def row(what, tm, extra=""):
        med, lo, hi, reps = tm
        rows.append("%-92s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (what, med, lo, hi, reps, extra))

    lib, dev = L.load(), m["vertices"].device
    verts, rgba, faces = m["vertices"].contiguous(), m["colors"].contiguous().reshape(-1).view(torch.int32), m["faces"].contiguous()
    nv, nf = verts.shape[0], faces.shape[0]
    rows.append("- V = %d, F = %d%s" % (nv, nf, "" if not label else "  (%s)" % label))
    fn, cum = torch.empty((nf, 3), dtype=torch.float32, device=dev), torch.empty(nf, dtype=torch.int64, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(lib.sp3_mesh_face_frames_ws_bytes(nf)), 16), dtype=torch.uint8, device=dev)

    def frames():
        L.check(lib.sp3_mesh_face_frames(verts.data_ptr(), nv, faces.data_ptr(), nf, ws.data_ptr(), fn.data_ptr(), cum.data_ptr(), info.data_ptr(),
                                         L.stream_ptr()), "sp3_mesh_face_frames")

    a = timed(frames)
    w, dmax, area = M._read_info(info)
    if not sample_only:
        row("sp3_mesh_face_frames alone (5 launches), prepared buffers", a,
            "area %.6f, dmax %.3e, W = %d; %.2f ns per face" % (area, dmax, w, 1e6 * a[0] / nf))
    for n in samples:
        pts, nrm = torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev)
        col, fidx = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)

        def sample():
            L.check(lib.sp3_mesh_sample(verts.data_ptr(), rgba.data_ptr(), nv, faces.data_ptr(), nf, cum.data_ptr(), info.data_ptr(), n, 0,
                                        pts.data_ptr(), nrm.data_ptr(), col.data_ptr(), fidx.data_ptr(), L.stream_ptr()), "sp3_mesh_sample")

        b = timed(sample)
        row("sp3_mesh_sample alone (1 launch), %d samples%s" % (n, "" if not label else ", " + label), b,
            "%.2f ns per sample; about %d dependent loads of the search each" % (1e6 * b[0] / n, int(np.ceil(np.log2(max(nf, 2))))))
        del pts, nrm, col, fidx
    if sample_only:
        return
    out = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    ws2 = torch.empty(int(lib.sp3_mesh_vertex_normals_ws_bytes(nv)), dtype=torch.uint8, device=dev)

    def vnormals():
        L.check(lib.sp3_mesh_vertex_normals(verts.data_ptr(), nv, faces.data_ptr(), nf, info.data_ptr(), ws2.data_ptr(), out.data_ptr(),
                                            L.stream_ptr()), "sp3_mesh_vertex_normals")

    c = timed(vnormals)
    row("sp3_mesh_vertex_normals alone (3 launches), prepared buffers", c,
        "%.2f ns per face; up to 9 64-bit atomic adds a face, not aggregated in the wave; scratch %.1f MB" % (1e6 * c[0] / nf, ws2.numel() / 1e6))
    del out, ws2, fn, cum, ws
    for n in samples:
        row("mesh.sample_surface end to end, %d samples (both entry points, the 16-byte read)" % n, timed(lambda: M.sample_surface(m, n)))
    row("mesh.vertex_normals end to end (both entry points, no host read)", timed(lambda: M.vertex_normals(m)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--samples", type=int, nargs="+", default=[200000, 1000000])
    ap.add_argument("--sample-only", default=None, metavar="LABEL")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    frames = ring_frames(args.frames, args.size, args.size)
    rows = ["Mesh surface sampling and normals on the device (%s), device %s" % (os.path.basename(L.LIB_PATH), torch.cuda.get_device_name(0)),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead, allocations and read-backs of a call "
            "included); the host route is one wall-clock run on this machine's CPU"]
    for n1 in args.dims:
        voxel = 2.4 / n1
        rows.append("--- %d frames of %dx%d fused in one call, voxel %.5f, a %d^3 virtual grid; extract_mesh(direct=True)"
                    % (len(frames), args.size, args.size, voxel, n1))
        brick = pool(n1, frames)
        m = brick.extract_mesh(direct=True)
        case(m, rows, args.sample_only is not None, args.sample_only, args.samples)
        if args.sample_only is None:
            s = M.simplify(m, 2 * voxel, origin=brick.origin)
            for icp in (False, True):
                tm = timed(lambda: E.evaluate_meshes(s, m, n_samples=200000, icp=icp), budget=3.0)
                r = E.evaluate_meshes(s, m, n_samples=200000, icp=icp)
                rows.append("%-92s %10.3f ms  [%9.3f .. %9.3f] x%-3d acc %.6f comp %.6f nc1 %.4f nc2 %.4f; areas %.5f / %.5f" %
                            (("evaluate_meshes(simplified at 2 voxels, the mesh), 200000 samples each, icp=%s" % icp,) + tuple(tm) +
                             (r["acc"], r["comp"], r["nc1"], r["nc2"], r["pred_area"], r["gt_area"])))
            tv = timed(lambda: E.evaluate_reconstruction(s["vertices"], m["vertices"]), budget=3.0)
            rv = E.evaluate_reconstruction(s["vertices"], m["vertices"])
            rows.append("%-92s %10.3f ms  [%9.3f .. %9.3f] x%-3d acc %.6f comp %.6f nc1 %.4f nc2 %.4f" %
                        (("evaluate_reconstruction on the two vertex sets (%d / %d), for scale" % (s["vertices"].shape[0], m["vertices"].shape[0]),)
                         + tuple(tv) + (rv["acc"], rv["comp"], rv["nc1"], rv["nc2"])))
            if not args.no_host:
                t_copy, t_sample, t_vn = host_route(m, args.samples[0])
                rows.append("%-92s %10.3f ms  = copy %.3f ms + frames, cumsum and %d samples by searchsorted %.3f ms + np.add.at vertex normals %.3f ms, "
                            "once, wall clock, %d CPUs visible" % ("host route: .cpu(), numpy cross products, cumsum, searchsorted, np.add.at",
                                                                   1e3 * (t_copy + t_sample + t_vn), 1e3 * t_copy, args.samples[0], 1e3 * t_sample,
                                                                   1e3 * t_vn, os.cpu_count()))
        del brick, m
        torch.cuda.empty_cache()
    text = "\n".join(rows)
    print(text)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
