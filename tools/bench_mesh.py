#!/usr/bin/env python
"""Timing record of the mesh export and the surface renderer (spann3r_amd/mesh.py, csrc/mesh.hip): 50 frames of 224x224 and 10 frames
of 512x512, seeded pointmaps (tools/bench_render.py's scene), confidences of which about 80 % pass the threshold.  Per case:
the face build and the vertex compaction on the device (device events around the library calls, buffers allocated outside), the
device-to-host copy of the compacted arrays and the file write (host clock), the numpy path of tests/mesh_ref.py on this machine's
CPU as the baseline, and per-frame raster time of surface=True against the point splat at 1920x1080 with the share of triangles
culled by max_bbox_px.  Nothing is asserted.  Writes the table to --out (profiles/mesh_export.txt is the committed record)."""
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
from spann3r_amd import vis
from tools.bench_render import scene, timed

THRESH = 2e-3


def host_ms(fn, reps=3):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts), max(ts), reps


def case(t, h, w, rows, cpu):
    pts_h, cols_h = scene(t, h, w)
    rng = np.random.default_rng(1)
    conf_h = (1 + rng.random((t, h, w)) * 0.01).astype(np.float32)
    pts, cols, conf = (torch.from_numpy(x).cuda() for x in (pts_h, cols_h, conf_h))
    n = t * h * w
    lib, st = L.load(), L.stream_ptr()

    def row(name, tm, work=None, unit=""):
        med, lo, hi, reps = tm
        rate = "" if work is None else "%10.3e %s" % (work / (med * 1e-3), unit)
        rows.append("%-66s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (name, med, lo, hi, reps, rate))

    rows.append("--- %d frames of %dx%d (%.2f M pixels), (conf - 1) / conf > %g keeps %.1f %%"
                % (t, h, w, n / 1e6, THRESH, 100 * float(((conf - 1) / conf > THRESH).float().mean())))
    cap = 4 * t * (h - 1) * (w - 1)
    faces = torch.empty((cap, 3), dtype=torch.int32, device="cuda")
    colour = torch.empty(cap, dtype=torch.int32, device="cuda")
    counts = torch.zeros(1 + 4 * t, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.sp3_mesh_faces_ws_bytes(t, h, w), dtype=torch.uint8, device="cuda")

    def build(both):
        L.check(lib.sp3_mesh_faces(0, conf.data_ptr(), THRESH, pts.data_ptr(), t, h, w, both, ws.data_ptr(), faces.data_ptr(), colour.data_ptr(),
                                   counts.data_ptr(), st), "sp3_mesh_faces")
    tm_both = timed(lambda: build(1))
    f_both = int(counts[0].item())
    row("sp3_mesh_faces, both windings (the reference's list): %d faces" % f_both, tm_both, f_both, "faces/s")
    tm_fwd = timed(lambda: build(0))
    f_fwd = int(counts[0].item())
    row("sp3_mesh_faces, forward windings (what the export uses): %d faces" % f_fwd, tm_fwd, f_fwd, "faces/s")
    rgba = torch.empty(n, dtype=torch.int32, device="cuda")
    L.check(lib.sp3_pack_rgba8(cols.data_ptr(), n, rgba.data_ptr(), st), "sp3_pack_rgba8")
    pos, out_rgba = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    info = torch.zeros(8, dtype=torch.float32, device="cuda")
    ws2 = torch.empty(lib.sp3_mesh_vertices_ws_bytes(n), dtype=torch.uint8, device="cuda")
    keep_faces = faces[:f_fwd].clone()
    work = torch.empty_like(keep_faces)
    xf = (M.C.c_float * 16)(*M.TRANSFORM.reshape(16))

    def compact():
        work.copy_(keep_faces)                                     # (the call rewrites the faces in place)
        L.check(lib.sp3_mesh_compact_vertices(pts.data_ptr(), rgba.data_ptr(), n, work.data_ptr(), f_fwd, 0, 0, 0.0, M.SCALE, xf, ws2.data_ptr(),
                                              pos.data_ptr(), out_rgba.data_ptr(), info.data_ptr(), info.data_ptr() + 8, st), "sp3_mesh_compact_vertices")
    tm_c = timed(compact)
    tm_copy = timed(lambda: work.copy_(keep_faces))
    nv = int(info.cpu().numpy()[:1].view(np.int32)[0])
    row("sp3_mesh_compact_vertices (+ a copy of the faces): %d of %d vertices" % (nv, n), tm_c, nv, "vertices/s")
    row("  of which the copy of the faces", tm_copy)
    row("scene_mesh, the whole device path with its two host reads", timed(lambda: M.scene_mesh(pts, cols, conf, THRESH)))
    scene_d = M.scene_mesh(pts, cols, conf, THRESH)
    nbytes = sum(scene_d[k].numel() * scene_d[k].element_size() for k in ("vertices", "colors", "faces"))
    row("device-to-host copy of vertices, colours, faces (%.1f MB)" % (nbytes / 1e6),
        host_ms(lambda: [scene_d[k].cpu() for k in ("vertices", "colors", "faces")]), nbytes, "bytes/s")
    host = {k: scene_d[k].cpu().numpy() for k in ("vertices", "colors", "faces")}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "scene.glb")
        row("write_glb from host arrays (host clock, temporary directory)", host_ms(lambda: M.write_glb(path, host["vertices"], host["colors"], host["faces"],
                                                                                                        bounds=scene_d["bounds"])), nbytes, "bytes/s")
    if cpu:
        import mesh_ref as MR
        t0 = time.perf_counter()
        ok = MR.conf_valid(conf_h, THRESH) & np.isfinite(pts_h).all(-1)
        ref_faces, _, ref_counts = MR.faces_ref(ok)
        t1 = time.perf_counter()
        fwd = MR.faces_ref(ok, both_windings=False)[0]
        t2 = time.perf_counter()
        rpos, kept, rfaces, _ = MR.compact_ref(pts_h, fwd, scale=M.SCALE, transform=M.TRANSFORM)
        t3 = time.perf_counter()
        rows.append("numpy path (tests/mesh_ref.py), host clock, one run, numpy's own single thread (OMP_NUM_THREADS=%s, torch threads %d):"
                    % (os.environ.get("OMP_NUM_THREADS", "unset"), torch.get_num_threads()))
        rows.append("  mask + face list, both windings as the reference builds it: %10.1f ms (%d faces) -> %.0f x the device's %.3f ms"
                    % ((t1 - t0) * 1e3, len(ref_faces), (t1 - t0) * 1e3 / tm_both[0], tm_both[0]))
        rows.append("  face list, forward windings: %10.1f ms -> %.0f x the device's %.3f ms" % ((t2 - t1) * 1e3, (t2 - t1) * 1e3 / tm_fwd[0], tm_fwd[0]))
        rows.append("  vertex compaction + transform + remap: %10.1f ms -> %.0f x the device's %.3f ms"
                    % ((t3 - t2) * 1e3, (t3 - t2) * 1e3 / max(tm_c[0] - tm_copy[0], 1e-6), tm_c[0] - tm_copy[0]))
        rows.append("  device equals numpy: faces %s, vertices %s" % (len(ref_faces) == f_both and np.array_equal(host["faces"], rfaces),
                                                                      np.array_equal(host["vertices"], rpos)))
    # raster: every frame into a 1920x1080 buffer, growing, as points and as surface
    cam = vis.fit_camera(pts)
    for surface in (False, True):
        r = vis.PointRenderer(camera=cam, conf_thresh=THRESH)

        def draw():
            r.clear()
            for i in range(t):
                (r.add_mesh if surface else r.add)(pts[i], cols[i], conf[i])
        tm = timed(draw)
        med, lo, hi, reps = tm
        row("raster, %s: clear + %d frames into %dx%d" % ("surface (add_mesh)" if surface else "points (add)", t, cam.width, cam.height), tm)
        rows.append("  per frame %.3f ms; pixels drawn at the end: %d of %d" % (med / t, int((r.image(False, True)[1] >= 0).sum()), cam.width * cam.height))
        if surface:
            r2 = vis.PointRenderer(camera=cam, conf_thresh=THRESH)
            for i in range(t):
                r2.add_mesh(pts[i], cols[i], conf[i])
            given, culled = (int(x) for x in r2.mesh_stats.cpu())
            rows.append("  triangles given %d, culled by max_bbox_px = 4096: %d (%.4f %%)" % (given, culled, 100.0 * culled / max(given, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="a quick look: 3 frames of 64x80 only")
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy baseline")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh: needs the GPU (nothing here is measured on a CPU)")
    rows = []
    head = ["mesh export and surface raster (%s), device %s" % (os.path.basename(L.LIB_PATH), torch.cuda.get_device_name(0)),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead included) unless a row says host clock", ""]
    if a.small:
        case(3, 64, 80, rows, not a.no_cpu)
    else:
        case(50, 224, 224, rows, not a.no_cpu)
        case(10, 512, 512, rows, not a.no_cpu)
    text = "\n".join(head + rows) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
