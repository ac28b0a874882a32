#!/usr/bin/env python
"""Timing record of marching tetrahedra on the brick pool (csrc/brick_mesh.hip, BrickTSDFVolume.extract_mesh(direct=True)) next to
the route through the dense kernel (to_dense() + sp3_tsdf_extract, BrickTSDFVolume.extract_mesh()) on the scene of
tools/bench_fusion.py / tools/bench_bricks.py: 50 frames of 224x224 fused in one call into a 256^3 virtual grid, then at half the
voxel size into 512^3.  Both routes run in this one process on one device, on the same pool.  Rows per size: the entry point alone
with prepared output buffers; the dense yardstick alone (to_dense of the allocated bricks' bounding box, which allocates the dense
volume, then sp3_tsdf_extract with prepared capacities); the two extract_mesh routes end to end (read-back of the counts and vertex
compaction included); the peak of torch.cuda.max_memory_allocated over each route, above what was held before it.  The two meshes
are compared as sets of face rows on the way (also against the dense kernel on the whole grid, whose origin is the virtual grid's).  Nothing is asserted.  Writes the table to --out (profiles/brick_mesh.txt is the
committed record)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from spann3r_amd import fusion as F
from spann3r_amd import lib as L
from tools.bench_fusion import ring_frames
from tools.bench_render import timed


def peak_mb(fn):
    """MB that fn holds at its peak above what is allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 1e6


def face_rows(m):
    v = m["vertices"].contiguous().view(torch.int32)[m["faces"].long()].reshape(-1, 9)
    c = m["colors"].contiguous().view(torch.int32).reshape(-1)[m["faces"].long()]
    return torch.cat([v, c], 1)


def same_faces(a, b):
    """the two meshes as multisets of (9 position words, 3 rgba words) rows"""
    if a["faces"].shape != b["faces"].shape:
        return False
    ra, rb = face_rows(a).cpu().numpy(), face_rows(b).cpu().numpy()
    return bool(np.array_equal(ra[np.lexsort(ra.T[::-1])], rb[np.lexsort(rb.T[::-1])]))


def case(n1, frames, hw, rows):
    t = len(frames)
    voxel = 2.4 / n1
    origin = (-1.2, -1.2, -0.3)
    rows.append("--- %d frames of %dx%d fused in one call, voxel %.5f, a %d^3 virtual grid; colours on, trunc = band = 3 voxels, min_weight 1"
                % (t, hw, hw, voxel, n1))

    def row(name, tm, extra=""):
        med, lo, hi, reps = tm
        rows.append("%-92s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (name, med, lo, hi, reps, extra))

    brick = F.BrickTSDFVolume(origin, voxel, (n1, n1, n1), capacity=1 << 15)
    brick.integrate(depth=[torch.from_numpy(f["depth"]).cuda() for f in frames], intrinsics=[f["K"] for f in frames],
                    cam2world=[f["cam2world"] for f in frames], valid=[torch.from_numpy(f["valid"]).cuda() for f in frames],
                    images=[torch.from_numpy(f["images"]).cuda() for f in frames])
    lo, size = brick.brick_box()
    nv, nf = brick.extract_raw()[3].cpu().tolist()
    rows.append("  %d bricks of %d (%.1f %%) = %.2f M allocated voxels; their bounding box %s = %.1f M voxels; V = %d, F = %d"
                % (brick.n_bricks, brick.table.numel(), 100.0 * brick.n_bricks / brick.table.numel(), brick.n_bricks * 512 / 1e6,
                   "x".join(str(s) for s in size), size[0] * size[1] * size[2] / 1e6, nv, nf))

    # ---- the entry point alone, prepared buffers
    lib, dev = L.load(), brick.device
    ver = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    col = torch.empty(nv, dtype=torch.int32, device=dev)
    fac = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.sp3_tsdf_brick_extract_ws_bytes(brick.n_bricks)), dtype=torch.uint8, device=dev)
    nx, ny, nz = brick.dims

    def entry():
        L.check(lib.sp3_tsdf_brick_extract(nx, ny, nz, brick._origin_c, brick.voxel_size, brick.table.data_ptr(), brick.slot_brick.data_ptr(),
                                           brick.n_bricks, brick.tsdf.data_ptr(), brick.weight.data_ptr(), L.ptr(brick.rgb), 1.0, ws.data_ptr(), nv, nf,
                                           ver.data_ptr(), col.data_ptr(), fac.data_ptr(), cnt.data_ptr(), L.stream_ptr()), "sp3_tsdf_brick_extract")

    a = timed(entry)
    row("bricks: sp3_tsdf_brick_extract alone (5 launches), prepared buffers", a, "scratch %.1f MB" % (ws.numel() / 1e6))
    del ver, col, fac, ws

    # ---- the yardstick: the route that existed before, in the same process
    def dense_raw():
        d = brick.to_dense(dims_limit=n1)
        return d.extract_raw(1.0, nv, nf)

    b = timed(dense_raw)
    row("dense route: to_dense(bounding box) + sp3_tsdf_extract (6 launches), capacities known", b, "%.2f x the brick entry" % (b[0] / a[0]))
    dense = brick.to_dense(dims_limit=n1)
    c = timed(lambda: dense.extract_raw(1.0, nv, nf))
    row("dense route: sp3_tsdf_extract alone on the densified box", c, "%.2f x the brick entry" % (c[0] / a[0]))
    del dense

    # ---- end to end
    d = timed(lambda: brick.extract_mesh(direct=True))
    e = timed(lambda: brick.extract_mesh(dims_limit=n1))
    row("bricks: extract_mesh(direct=True), read-back and vertex compaction included", d)
    row("dense route: extract_mesh(), the same included", e, "%.2f x direct" % (e[0] / d[0]))
    ma, mb = brick.extract_mesh(direct=True), brick.extract_mesh(dims_limit=n1)
    mc = brick.to_dense(((0, 0, 0), brick.dims), dims_limit=n1).extract_mesh()      # the whole grid: its origin is the virtual grid's
    rows.append("  the two meshes: %d and %d faces, %d and %d vertices; the same face rows (positions and colours, bit for bit) as the dense "
                "kernel on the bounding box (positions from the box's origin): %s, on the whole grid: %s"
                % (ma["faces"].shape[0], mb["faces"].shape[0], ma["vertices"].shape[0], mb["vertices"].shape[0], same_faces(ma, mb), same_faces(ma, mc)))
    del ma, mb, mc
    brick._mesh_ws = None
    held = brick.memory_bytes
    pa, pb = peak_mb(lambda: brick.extract_mesh(direct=True)), peak_mb(lambda: brick.extract_mesh(dims_limit=n1))
    rows.append("  peak device memory above the pool (%.1f MB held): direct %.1f MB (scratch kept on the volume included); dense route %.1f MB"
                % (held / 1e6, pa, pb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    args = ap.parse_args()
    rows = ["Marching tetrahedra on the brick pool against the route through the dense kernel (libspann3r_hip.so), device %s" % torch.cuda.get_device_name(0),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead, allocations and read-backs of a call "
            "included); both routes in one process on the same pool"]
    frames = ring_frames(args.frames, args.size, args.size)
    for n1 in args.dims:
        case(n1, frames, args.size, rows)
        torch.cuda.empty_cache()
    text = "\n".join(rows)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
