#!/usr/bin/env python
"""Timing record of the mesh components (csrc/mesh_components.hip; mesh.components, mesh.filter_components and the
min_component_faces argument of the extractors) on the pools of tools/bench_brick_mesh.py: 50 frames of 224x224 fused in one call
into a 256^3 virtual grid (0.93 M faces), then at half the voxel size into 512^3 (3.5 M faces).  Rows per size: sp3_mesh_components
alone and sp3_mesh_select_faces alone with prepared buffers; extract_mesh(direct=True) end to end without and with
min_component_faces; for scale, the host route a user had before -- the faces copied to the host, then
scipy.sparse.csgraph.connected_components where scipy imports (otherwise the numpy restatement of tests/mesh_components_ref.py on a
stated part of the faces), timed on this machine's CPU -- and, with --parent_tree PATH, extract_mesh(direct=True) of the checkout
at PATH (the parent commit, built) on the same pool, in a child process of its own on the same device.  Times are medians of device
events around whole calls after warm-up, except the host route (wall clock).  Nothing is asserted.  Writes the table to --out
(profiles/mesh_components.txt is the committed record)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:                                  # (the child of --parent_tree: import that checkout instead)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from spann3r_amd import fusion as F
from spann3r_amd import lib as L
from tools.bench_fusion import ring_frames
from tools.bench_render import timed


def pool(n1, frames):
    brick = F.BrickTSDFVolume((-1.2, -1.2, -0.3), 2.4 / n1, (n1, n1, n1), capacity=1 << 15)
    brick.integrate(depth=[torch.from_numpy(f["depth"]).cuda() for f in frames], intrinsics=[f["K"] for f in frames],
                    cam2world=[f["cam2world"] for f in frames], valid=[torch.from_numpy(f["valid"]).cuda() for f in frames],
                    images=[torch.from_numpy(f["images"]).cuda() for f in frames])
    return brick


def host_route(faces, nv):
    """(what ran, seconds of the copy, seconds of the labelling, components found).  The imports and one small warm call of the
    library happen before the clock starts."""
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components
        connected_components(sp.coo_matrix((np.ones(2, np.int8), ([0, 1], [1, 2])), shape=(4, 4)).tocsr(), directed=False)
    except ImportError:
        sp = None
        import mesh_components_ref as MC
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f = faces.cpu().numpy()
    t1 = time.perf_counter()
    if sp is None:
        part = f[:len(f) // 8]
        c = MC.components(part, nv)["n_components"]
        return "numpy restatement on the first eighth of the faces (%d)" % len(part), t1 - t0, time.perf_counter() - t1, c
    u, v = np.concatenate([f[:, 0], f[:, 0]]), np.concatenate([f[:, 1], f[:, 2]])
    adj = sp.coo_matrix((np.ones(len(u), np.int8), (u, v)), shape=(nv, nv)).tocsr()
    c, labels = connected_components(adj, directed=False)
    c -= nv - len(np.unique(f))                           # (vertices no face names are classes of their own there)
    return "scipy %s csgraph.connected_components (csr build included)" % __import__("scipy").__version__, t1 - t0, time.perf_counter() - t1, c


def case(n1, frames, hw, rows, min_faces, parent_tree):
    from spann3r_amd import mesh as M
    voxel = 2.4 / n1
    rows.append("--- %d frames of %dx%d fused in one call, voxel %.5f, a %d^3 virtual grid; colours on, trunc = band = 3 voxels, min_weight 1"
                % (len(frames), hw, hw, voxel, n1))

    def row(name, tm, extra=""):
        med, lo, hi, reps = tm
        rows.append("%-92s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (name, med, lo, hi, reps, extra))

    brick = pool(n1, frames)
    v, _, f, counts = brick.extract_raw()
    nv, nf = counts.cpu().tolist()
    if nv > v.shape[0] or nf > f.shape[0]:
        v, _, f, counts = brick.extract_raw(1.0, nv, nf)
    faces = f[:nf].contiguous()
    comp = M.components(faces, nv)
    cf = np.sort(comp["component_faces"].cpu().numpy())[::-1]
    rows.append("  %d bricks; V = %d, F = %d; %d components, the largest of %s faces, %d of fewer than %d faces (%d faces in those), %d vertices "
                "no face names" % (brick.n_bricks, nv, nf, comp["n_components"], ", ".join(str(x) for x in cf[:3]), int((cf < min_faces).sum()), min_faces,
                                   int(cf[cf < min_faces].sum()), int((comp["vertex_component"] < 0).sum())))

    # ---- the entry points alone, prepared buffers
    lib, dev, c = L.load(), faces.device, comp["n_components"]
    vc, fc = torch.empty(nv, dtype=torch.int32, device=dev), torch.empty(nf, dtype=torch.int32, device=dev)
    ncf, ncv = torch.empty(max(c, 1), dtype=torch.int32, device=dev), torch.empty(max(c, 1), dtype=torch.int32, device=dev)
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.sp3_mesh_components_ws_bytes(nv)), dtype=torch.uint8, device=dev)

    def entry():
        L.check(lib.sp3_mesh_components(faces.data_ptr(), nf, nv, ws.data_ptr(), c, vc.data_ptr(), fc.data_ptr(), ncf.data_ptr(), ncv.data_ptr(),
                                        info.data_ptr(), L.stream_ptr()), "sp3_mesh_components")

    a = timed(entry)
    row("sp3_mesh_components alone (8 launches), prepared buffers", a, "scratch %.1f MB; %.2f ns per face" % (ws.numel() / 1e6, 1e6 * a[0] / nf))
    keep = torch.from_numpy((comp["component_faces"].cpu().numpy() >= min_faces).astype(np.uint8)).to(dev)
    out, count = torch.empty((nf, 3), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ws2 = torch.empty(int(lib.sp3_mesh_select_faces_ws_bytes(nf)), dtype=torch.uint8, device=dev)

    def select():
        L.check(lib.sp3_mesh_select_faces(faces.data_ptr(), fc.data_ptr(), nf, keep.data_ptr(), c, ws2.data_ptr(), out.data_ptr(), count.data_ptr(),
                                          L.stream_ptr()), "sp3_mesh_select_faces")

    b = timed(select)
    row("sp3_mesh_select_faces alone (3 launches), components of >= %d faces kept" % min_faces, b, "%d of %d faces kept" % (int(count.item()), nf))
    del vc, ncf, ncv, ws, out, ws2

    # ---- end to end
    d = timed(lambda: brick.extract_mesh(direct=True))
    e = timed(lambda: brick.extract_mesh(direct=True, min_component_faces=min_faces))
    row("extract_mesh(direct=True), this commit", d)
    row("extract_mesh(direct=True, min_component_faces=%d): components, ranking read-back, selection" % min_faces, e, "%.2f x without; + %.3f ms" % (e[0] / d[0], e[0] - d[0]))
    m = brick.extract_mesh(direct=True, min_component_faces=min_faces)
    rows.append("  filtered mesh: %d faces, %d vertices, components %s" % (m["faces"].shape[0], m["vertices"].shape[0], m["components"]))
    if parent_tree:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", parent_tree, "--extract_only", "--dims", str(n1), "--frames",
                                str(len(frames)), "--size", str(hw)], capture_output=True, text=True, timeout=600)
        line = [x for x in child.stdout.splitlines() if x.startswith("{")]
        if child.returncode == 0 and line:
            r = json.loads(line[-1])
            row("extract_mesh(direct=True), the parent commit's checkout on the same pool (its own process)", tuple(r["timed"]),
                "%d faces; this commit / parent = %.3f" % (r["faces"], d[0] / r["timed"][0]))
        else:
            rows.append("  the parent's checkout did not run: %s" % (child.stderr.strip().splitlines() or ["?"])[-1])

    # ---- for scale: the host route
    what, t_copy, t_label, c_host = host_route(faces, nv)
    rows.append("%-92s %10.3f ms  = copy %.3f ms + labelling %.3f ms, once, wall clock, %d CPUs visible; %d components; %.1f x sp3_mesh_components"
                % ("host route: faces.cpu(), then " + what, 1e3 * (t_copy + t_label), 1e3 * t_copy, 1e3 * t_label, os.cpu_count(), c_host,
                   1e3 * (t_copy + t_label) / a[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--min_faces", type=int, default=100)
    ap.add_argument("--parent_tree", default=None, help="a built checkout of the parent commit: its extract_mesh(direct=True) is timed too")
    ap.add_argument("--tree", default=None, help="import the package from this checkout (used by --parent_tree's child)")
    ap.add_argument("--extract_only", action="store_true", help="time extract_mesh(direct=True) alone and print one JSON line")
    args = ap.parse_args()
    frames = ring_frames(args.frames, args.size, args.size)
    if args.extract_only:
        brick = pool(args.dims[0], frames)
        tm = timed(lambda: brick.extract_mesh(direct=True))
        print(json.dumps(dict(timed=tm, faces=brick.extract_mesh(direct=True)["faces"].shape[0], tree=ROOT)))
        return
    rows = ["Mesh components on the device (libspann3r_hip.so), device %s" % torch.cuda.get_device_name(0),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead, allocations and read-backs of a call "
            "included); the host route is one wall-clock run on this machine's CPU"]
    for n1 in args.dims:
        case(n1, frames, args.size, rows, args.min_faces, args.parent_tree)
        torch.cuda.empty_cache()
    text = "\n".join(rows)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
