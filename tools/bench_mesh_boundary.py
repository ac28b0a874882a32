#!/usr/bin/env python
"""Timing record of the mesh boundary loops and the hole filling (csrc/mesh_boundary.hip; mesh.BoundaryLoops, mesh.fill_holes, the
fill_holes argument of the extractors) on the brick pools of tools/bench_brick_mesh.py: 50 frames of 224x224 fused into a 256^3
virtual grid, then at half the voxel size into 512^3, meshed with extract_mesh(direct=True).  Rows per size: MeshTopology for scale;
BoundaryLoops on a prebuilt topology end to end, with B, the loops and the rounds beside it; each entry point of it alone on
prepared buffers; fill_holes on prebuilt loops and end to end from the bare mesh; extract_mesh(direct=True) with and without
fill_holes.  Next to them the same work on this machine's CPU, both from the host copy of the edge table: the numpy restatement
(tests/mesh_boundary_ref.py) and a plain Python walk along a dict from vertex to the element leaving it.  Nothing is asserted
except that the three agree.  Writes the table to --out (profiles/mesh_boundary.txt is the committed record)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from spann3r_amd import fusion as F
from spann3r_amd import lib as L
from spann3r_amd import mesh as M
from tools.bench_fusion import ring_frames
from tools.bench_render import timed

FILL = 16


def wall(fn, reps):
    """ms per call on the host clock, as (median, min, max, reps)"""
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return (float(np.median(ts)), min(ts), max(ts), reps), out


def host_walk(src, dst):
    """the loops by walking, from the elements' ends: -> the loops as lists of elements from their heads, in ascending head"""
    leaving, entering = {}, {}
    for j, (s, d) in enumerate(zip(src.tolist(), dst.tolist())):
        leaving.setdefault(s, []).append(j)
        entering.setdefault(d, []).append(j)
    nxt = [leaving[d][0] if len(leaving.get(d, ())) == 1 and len(entering[d]) == 1 else -1 for d in dst.tolist()]
    loops, state = [], [0] * len(nxt)                       # 0 new, 1 on the path being walked, 2 done
    for j in range(len(nxt)):
        if state[j]:
            continue
        path, k = [], j
        while k != -1 and state[k] == 0:
            state[k] = 1
            path.append(k)
            k = nxt[k]
        if k == j:
            loops.append(path)
        for i in path:
            state[i] = 2
    return loops


def case(n1, frames, hw, rows, host_reps):
    import mesh_boundary_ref as B
    t = len(frames)
    voxel = 2.4 / n1
    rows.append("--- %d frames of %dx%d fused in one call, voxel %.5f, a %d^3 virtual grid; extract_mesh(direct=True)" % (t, hw, hw, voxel, n1))

    def row(name, tm, extra=""):
        med, lo, hi, reps = tm
        rows.append("%-100s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (name, med, lo, hi, reps, extra))

    brick = F.BrickTSDFVolume((-1.2, -1.2, -0.3), voxel, (n1, n1, n1), capacity=1 << 15)
    brick.integrate(depth=[torch.from_numpy(f["depth"]).cuda() for f in frames], intrinsics=[f["K"] for f in frames],
                    cam2world=[f["cam2world"] for f in frames], valid=[torch.from_numpy(f["valid"]).cuda() for f in frames],
                    images=[torch.from_numpy(f["images"]).cuda() for f in frames])
    m = brick.extract_mesh(direct=True)
    v, f = m["vertices"], m["faces"]
    nv, nf, dev, lib = v.shape[0], f.shape[0], v.device, L.load()
    topo = M.topology(m)
    loops = M.boundary_loops(m, topo)
    b, e, r = loops.n_boundary, topo.n_edges, loops.report
    lengths = torch.diff(loops.loop_first).cpu().numpy()
    rows.append("  V = %d, F = %d, E = %d; B = %d boundary elements (%.2f %% of 3 F) in %d loops (the longest %d), %d on open chains, %d irregular "
                "vertices; %d rounds" % (nv, nf, e, b, 100.0 * b / (3 * nf), r["loops"], r["longest"], r["open"], r["irregular_vertices"], loops.rounds))
    rows.append("  loops by length: " + ", ".join("%d x %d" % (int(c), int(n)) for n, c in zip(*np.unique(lengths, return_counts=True)) if n <= 32) +
                "; %d longer than 32" % int((lengths > 32).sum()))

    a = timed(lambda: M.topology(m))
    row("MeshTopology(m) end to end, for scale", a)
    bl = timed(lambda: M.boundary_loops(m, topo))
    row("BoundaryLoops(m, topology=prebuilt) end to end (%d launches, allocations, the face comparison and the one 64-byte read)" %
        (6 + 1 + 1 + loops.rounds + 7), bl, "%.2f x MeshTopology" % (bl[0] / a[0]))
    row("BoundaryLoops(m): the topology built first", timed(lambda: M.boundary_loops(m)))

    # ---- its parts on prepared buffers
    i32 = dict(dtype=torch.int32, device=dev)
    edge, half, src, dst, nxt, loop, rank = (torch.empty(b, **i32) for _ in range(7))
    vout, vin, vleave = (torch.empty(nv, **i32) for _ in range(3))
    info, state = torch.zeros(16, **i32), torch.empty((b, 4), **i32)
    first, members = torch.empty(b + 1, **i32), torch.empty(b, **i32)
    ws_e = torch.empty(int(lib.sp3_mesh_boundary_elements_ws_bytes(e)), dtype=torch.uint8, device=dev)
    ws_r = torch.empty(int(lib.sp3_mesh_boundary_rank_ws_bytes(b)), dtype=torch.uint8, device=dev)
    ws_l = torch.empty(int(lib.sp3_mesh_boundary_loops_ws_bytes(b)), dtype=torch.uint8, device=dev)

    def elements():
        L.check(lib.sp3_mesh_boundary_elements(f.data_ptr(), nf, nv, topo.edge_class.data_ptr(), topo.edge_first.data_ptr(), topo.half_edges.data_ptr(),
                                               e, b, ws_e.data_ptr(), edge.data_ptr(), half.data_ptr(), src.data_ptr(), dst.data_ptr(), vout.data_ptr(),
                                               vin.data_ptr(), vleave.data_ptr(), L.stream_ptr()), "sp3_mesh_boundary_elements")

    def link():
        info.zero_()
        L.check(lib.sp3_mesh_boundary_link(dst.data_ptr(), b, vout.data_ptr(), vin.data_ptr(), vleave.data_ptr(), nv, nxt.data_ptr(), info.data_ptr(),
                                           L.stream_ptr()), "sp3_mesh_boundary_link")

    def ranks():
        L.check(lib.sp3_mesh_boundary_rank(nxt.data_ptr(), b, ws_r.data_ptr(), state.data_ptr(), L.stream_ptr()), "sp3_mesh_boundary_rank")

    def csr():
        info.zero_()
        L.check(lib.sp3_mesh_boundary_loops(nxt.data_ptr(), state.data_ptr(), b, ws_l.data_ptr(), loop.data_ptr(), rank.data_ptr(), first.data_ptr(),
                                            members.data_ptr(), info.data_ptr(), L.stream_ptr()), "sp3_mesh_boundary_loops")

    row("  sp3_mesh_boundary_elements (6 launches over %d edges and %d vertices)" % (e, nv), timed(elements))
    row("  sp3_mesh_boundary_link (1 launch; the info fill beside it)", timed(link))
    rk = timed(ranks)
    row("  sp3_mesh_boundary_rank (1 + %d launches over %d elements)" % (loops.rounds, b), rk, "%.4f ms per round" % (rk[0] / (1 + loops.rounds)))
    row("  sp3_mesh_boundary_loops (7 launches; the info fill beside it)", timed(csr))
    del edge, half, src, dst, nxt, loop, rank, vout, vin, vleave, state, first, members, ws_e, ws_r, ws_l

    # ---- the fill
    filled = M.fill_holes(m, FILL, loops=loops)
    s = filled["fill"]
    rows.append("  fill_holes(max_edges = %d): %d of %d loops filled, %d vertices and %d faces added; boundary edges %d -> %d" %
                (FILL, s["filled"], s["loops"], s["vertices_added"], s["faces_added"], b, M.topology(filled).report["boundary"]))
    f1 = timed(lambda: M.fill_holes(m, FILL, loops=loops))
    f2 = timed(lambda: M.fill_holes(m, FILL, topology=topo))
    f3 = timed(lambda: M.fill_holes(m, FILL))
    row("fill_holes(m, %d, loops=prebuilt): 4 + 2 launches, the copies of the mesh, the face comparison and the one read" % FILL, f1)
    row("fill_holes(m, %d, topology=prebuilt): the loops built first" % FILL, f2, "%.2f x MeshTopology" % (f2[0] / a[0]))
    row("fill_holes(m, %d) end to end: the topology and the loops built first" % FILL, f3)
    x0 = timed(lambda: brick.extract_mesh(direct=True))
    x1 = timed(lambda: brick.extract_mesh(direct=True, fill_holes=FILL))
    row("extract_mesh(direct=True)", x0)
    row("extract_mesh(direct=True, fill_holes=%d)" % FILL, x1, "%.2f x" % (x1[0] / x0[0]))

    # ---- the same work on the CPU, from the host copy of the edge table
    fh = f.cpu().numpy()
    host_topo = {k: getattr(topo, k).cpu().numpy() for k in ("edge_class", "edge_first", "half_edges")}
    h1, ref = wall(lambda: B.boundary_loops(fh, nv, topo=host_topo), host_reps)
    row("host: the numpy restatement of the loops (tests/mesh_boundary_ref.py), the edge table given", h1, "%.0f x BoundaryLoops" % (h1[0] / bl[0]))
    h2, walked = wall(lambda: host_walk(ref["src"], ref["dst"]), host_reps)
    row("host: the Python walk, the elements given", h2, "%.0f x BoundaryLoops" % (h2[0] / bl[0]))
    vh, ch = v.cpu().numpy(), m["colors"].cpu().numpy()
    h3, hf = wall(lambda: B.fill_holes(vh, ch, fh, FILL, loops=ref), host_reps)
    row("host: the numpy restatement of the fill, the loops given", h3, "%.0f x fill_holes(loops=prebuilt)" % (h3[0] / f1[0]))
    same = all(np.array_equal(getattr(loops, k).cpu().numpy(), ref[k]) for k in B.TABLES) and loops.report == ref["report"]
    same_walk = [j for p in walked for j in p] == ref["loop_members"].tolist()
    same_fill = np.array_equal(filled["vertices"].cpu().numpy().view(np.uint32), hf[0].view(np.uint32)) and \
        np.array_equal(filled["faces"].cpu().numpy(), hf[2]) and np.array_equal(filled["colors"].cpu().numpy(), hf[1])
    rows.append("  device == restatement: tables and report %s, filled mesh bit for bit %s; walk == restatement: %s" % (same, same_fill, same_walk))
    assert same and same_walk and same_fill


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--host_reps", type=int, default=2)
    args = ap.parse_args()
    rows = ["Mesh boundary loops and hole filling on the device (libspann3r_hip.so), device %s; the host rows: OMP_NUM_THREADS = %s"
            % (torch.cuda.get_device_name(0), os.environ.get("OMP_NUM_THREADS", "unset")),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead, allocations and read-backs of a call "
            "included); host rows on the wall clock"]
    frames = ring_frames(args.frames, args.size, args.size)
    for n1 in args.dims:
        case(n1, frames, args.size, rows, args.host_reps)
        torch.cuda.empty_cache()
    text = "\n".join(rows)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
