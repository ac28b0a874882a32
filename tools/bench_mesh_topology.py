#!/usr/bin/env python
"""Timing record of the mesh topology and the Taubin filter (csrc/mesh_topology.hip; mesh.MeshTopology, mesh.smooth, the smooth_iters
argument of the extractors) on the brick pools of tools/bench_brick_mesh.py: 50 frames of 224x224 fused into a 256^3 virtual grid,
then at half the voxel size into 512^3, meshed with extract_mesh(direct=True).  Rows per size: MeshTopology end to end; each entry
point and each sort of it alone on prepared buffers (sp3_mesh_edge_table is eight launches, timed as one call); one smoothing pass;
smooth at 10 iterations with and without a prebuilt topology; extract_mesh(direct=True) with and without smooth_iters=10.  Next to
them the host route a user has today, on this machine's CPU: faces.cpu(), the np.unique report of tests/fusion_ref.manifold_report,
a scipy.sparse adjacency matrix and matrix-vector products for the same 10 rounds of the filter (float64 on the host; its positions
are compared with the device's as a largest difference, they are not expected to be equal in bits).  Nothing is asserted.  Writes
the table to --out (profiles/mesh_topology.txt is the committed record)."""
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


def wall(fn, reps):
    """ms per call on the host clock, as (median, min, max, reps)"""
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return (float(np.median(ts)), min(ts), max(ts), reps), out


def host_smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53):
    """the filter through scipy.sparse: a binary adjacency matrix of the distinct neighbours, row-normalised, boundary vertices fixed"""
    import scipy.sparse as sp
    v, f = vertices.cpu().numpy().astype(np.float64), faces.cpu().numpy().astype(np.int64)
    n = len(v)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und, cnt = np.unique(np.sort(e, axis=1), axis=0, return_counts=True)
    a = sp.coo_matrix((np.ones(2 * len(und)), (np.concatenate([und[:, 0], und[:, 1]]), np.concatenate([und[:, 1], und[:, 0]]))), shape=(n, n)).tocsr()
    k = np.asarray(a.sum(1)).ravel()
    move = k > 0
    move[und[cnt == 1].reshape(-1)] = False
    w = sp.diags(np.where(k > 0, 1.0 / np.maximum(k, 1), 0.0)) @ a
    for _ in range(iterations):
        for c in (lam, mu):
            d = w @ v - v
            v = v + c * np.where(move[:, None], d, 0.0)
    return torch.from_numpy(v.astype(np.float32)).to(vertices.device)


def case(n1, frames, hw, rows, host_reps):
    import fusion_ref as FR
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
    r = topo.report
    rows.append("  V = %d, F = %d; E = %d (%d boundary, %d interior, %d inconsistent, %d non-manifold), %d unusable faces, Euler characteristic %d, "
                "%d boundary vertices" % (nv, nf, r["edges"], r["boundary"], r["interior"], r["inconsistent"], r["nonmanifold"], r["faces_unusable"],
                                         r["euler"], topo.boundary_vertices))

    # ---- the topology: end to end, then its parts on prepared buffers
    a = timed(lambda: M.topology(m))
    row("MeshTopology(m) end to end (2 sorts, 10 launches, allocations and the one 64-byte read included)", a)
    n, e = 3 * nf, topo.n_edges
    i32 = dict(dtype=torch.int32, device=dev)
    keys, info = torch.empty(n, dtype=torch.int64, device=dev), torch.zeros(16, **i32)

    def edge_keys():
        L.check(lib.sp3_mesh_edge_keys(f.data_ptr(), nf, nv, keys.data_ptr(), info.data_ptr(), L.stream_ptr()), "sp3_mesh_edge_keys")

    row("  sp3_mesh_edge_keys (1 launch, %d faces)" % nf, timed(edge_keys))
    row("  torch.sort(stable=True) of the %d int64 edge keys" % n, timed(lambda: torch.sort(keys, stable=True)))
    skeys, order = torch.sort(keys, stable=True)
    edges, first = torch.empty((n, 2), **i32), torch.empty(n + 1, **i32)
    uses, fwd, half = torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(n, **i32)
    cls, vb = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(nv, dtype=torch.uint8, device=dev)
    ws = torch.empty(int(lib.sp3_mesh_edge_table_ws_bytes(n, nv)), dtype=torch.uint8, device=dev)

    def edge_table():
        info.zero_()
        L.check(lib.sp3_mesh_edge_table(skeys.data_ptr(), order.data_ptr(), n, nv, ws.data_ptr(), edges.data_ptr(), first.data_ptr(), uses.data_ptr(),
                                        fwd.data_ptr(), cls.data_ptr(), half.data_ptr(), vb.data_ptr(), info.data_ptr(), L.stream_ptr()),
                "sp3_mesh_edge_table")

    row("  sp3_mesh_edge_table (8 launches: flags, head count, scan, scatter, classes, half-edge merge, vertex count)", timed(edge_table))
    dkeys = torch.empty(2 * e, dtype=torch.int64, device=dev)

    def adj_keys():
        L.check(lib.sp3_mesh_adjacency_keys(topo.edges.data_ptr(), e, dkeys.data_ptr(), L.stream_ptr()), "sp3_mesh_adjacency_keys")

    row("  sp3_mesh_adjacency_keys (1 launch, %d edges)" % e, timed(adj_keys))
    row("  torch.sort of the %d int64 directed keys" % (2 * e), timed(lambda: torch.sort(dkeys, stable=True)))
    sdk = torch.sort(dkeys, stable=True)[0]
    off, nb = torch.empty(nv + 1, **i32), torch.empty(2 * e, **i32)

    def adj_rows():
        L.check(lib.sp3_mesh_adjacency_rows(sdk.data_ptr(), 2 * e, nv, off.data_ptr(), nb.data_ptr(), L.stream_ptr()), "sp3_mesh_adjacency_rows")

    row("  sp3_mesh_adjacency_rows (1 launch: neighbours and row starts)", timed(adj_rows))
    del keys, skeys, order, edges, first, uses, fwd, half, cls, vb, ws, dkeys, sdk, off, nb

    # ---- the filter
    out = torch.empty_like(v)
    p = timed(lambda: topo.smooth_pass(v, 0.5, topo.vertex_boundary, out=out))
    gathered = (2 * e * 16 + nv * (12 + 12 + 8 + 1)) / 1e6                      # per neighbour 12 bytes of position and 4 of index
    row("sp3_mesh_smooth_pass, one pass (mean valence %.2f)" % (2 * e / max(nv, 1)), p,
        "%.1f MB asked for by the lanes, %.0f GB/s of that (gathers repeat lines and the repeats run cache-warm: not HBM traffic)"
        % (gathered, gathered / p[0]))
    s1 = timed(lambda: M.smooth(m, 10, topology=topo))
    s2 = timed(lambda: M.smooth(m, 10))
    row("smooth(m, 10, topology=prebuilt): 20 passes, the face comparison and the bounds read included", s1)
    row("smooth(m, 10): the topology built first", s2)
    x0 = timed(lambda: brick.extract_mesh(direct=True))
    x1 = timed(lambda: brick.extract_mesh(direct=True, smooth_iters=10))
    row("extract_mesh(direct=True)", x0)
    row("extract_mesh(direct=True, smooth_iters=10)", x1, "%.2f x" % (x1[0] / x0[0]))

    # ---- the host route of today
    h0, fh = wall(lambda: f.cpu().numpy(), host_reps)
    row("host: faces.cpu()", h0)
    h1, rep = wall(lambda: FR.manifold_report(fh), host_reps)
    row("host: the np.unique report (tests/fusion_ref.manifold_report) on the CPU", h1, "%.0f x MeshTopology" % (h1[0] / a[0]))
    h2, hs = wall(lambda: host_smooth(v, f), host_reps)
    row("host: scipy.sparse adjacency + 20 matrix-vector products, positions copied out and back", h2, "%.0f x smooth(m, 10)" % (h2[0] / s2[0]))
    dv = M.smooth(m, 10)["vertices"]
    rows.append("  the host report: closed %s, euler %d, %d boundary edges, bad %d; largest |device - host| position after 10 rounds: %.3g (voxel %.5f)"
                % (rep["closed"], rep["euler"], len(rep["boundary"]), rep["bad"], float((dv - hs).abs().max()), voxel))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--host_reps", type=int, default=2)
    args = ap.parse_args()
    rows = ["Mesh topology and Taubin smoothing on the device (libspann3r_hip.so), device %s; the host rows: OMP_NUM_THREADS = %s"
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
