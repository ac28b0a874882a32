#!/usr/bin/env python
"""Timing record of the brick TSDF volume (spann3r_amd/fusion.py BrickTSDFVolume, csrc/bricks.hip) next to the dense volume on the
scene of tools/bench_fusion.py / tools/bench_raycast.py: 50 frames of 224x224 -- a sphere on a plane seen from a ring of cameras --
at the voxel size that gives the dense bench its 256^3, then at half that (a 512^3 virtual grid; the dense volume is then 2.7 GB).
Both paths run in this one process on one device.  Rows per size: mark + alloc + integrate against the dense integrate, as one call
and as 50 calls (each repeat starts from reset(); the brick path's read-back of two int32 per call is inside); the 50 views ray-cast
in one launch and one 1920x1080 view, prepared tables; tracked fusion end to end through fuse_pointmaps(track=True) (host clock
around the whole call ending in a synchronise); the bytes held.  The ray-cast maps of the two paths are compared bit for bit on the
way (the brick volume against its own to_dense).  Nothing is asserted.  Writes the table to --out (profiles/bricks.txt is the
committed record)."""
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
from tools.bench_fusion import ring_frames
from tools.bench_raycast import world_points
from tools.bench_render import timed


def dense_bytes(vol):
    return sum(t.numel() * t.element_size() for t in (vol.tsdf, vol.weight, vol.rgb) if t is not None)


def host_ms(fn, reps=3):
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = ts[1:]
    return (float(np.median(ts)), min(ts), max(ts), reps), out


def case(n1, frames, hw, rows, tracked=True):
    t = len(frames)
    voxel = 2.4 / n1
    origin = (-1.2, -1.2, -0.3)
    rows.append("--- %d frames of %dx%d, voxel %.5f: dense %d^3 voxels (%.1f M) against bricks in a %d^3 virtual grid; colours on, "
                "trunc = band = 3 voxels, step 1 voxel" % (t, hw, hw, voxel, n1, n1 ** 3 / 1e6, n1))

    def row(name, tm, extra=""):
        med, lo, hi, reps = tm
        rows.append("%-86s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (name, med, lo, hi, reps, extra))

    depth = [torch.from_numpy(f["depth"]).cuda() for f in frames]
    valid = [torch.from_numpy(f["valid"]).cuda() for f in frames]
    images = [torch.from_numpy(f["images"]).cuda() for f in frames]
    Ks, Ps = [f["K"] for f in frames], [f["cam2world"] for f in frames]
    dense = F.TSDFVolume(origin, voxel, (n1, n1, n1))
    brick = F.BrickTSDFVolume(origin, voxel, (n1, n1, n1), capacity=1 << 15)
    all_kw = dict(depth=depth, intrinsics=Ks, cam2world=Ps, valid=valid, images=images)

    # ---- integration
    def one(vol):
        vol.reset()
        vol.integrate(**all_kw)

    def many(vol):
        vol.reset()
        for i in range(t):
            vol.integrate(depth=depth[i:i + 1], intrinsics=Ks[i], cam2world=Ps[i][None], valid=valid[i:i + 1], images=images[i:i + 1])

    a, b = timed(lambda: one(dense)), timed(lambda: one(brick))
    row("dense: reset + integrate, %d frames in ONE call" % t, a)
    row("bricks: reset + mark + alloc + integrate, %d frames in ONE call" % t, b,
        "%.2f x dense; %d bricks of %d (%.1f %%), pool grown %d times" % (b[0] / a[0], brick.n_bricks, brick.table.numel(),
                                                                           100.0 * brick.n_bricks / brick.table.numel(), brick.grown))
    a, b = timed(lambda: many(dense)), timed(lambda: many(brick))
    row("dense: reset + %d integrate calls of one frame" % t, a)
    row("bricks: reset + %d (mark + alloc + integrate) calls of one frame" % t, b, "%.2f x dense; %d bricks" % (b[0] / a[0], brick.n_bricks))
    one(dense)
    one(brick)
    rows.append("  bytes held: dense %.1f MB; bricks %.1f MB (%d slots of capacity %d in use, table and flags %.1f MB)"
                % (dense_bytes(dense) / 1e6, brick.memory_bytes / 1e6, brick.n_bricks, brick.capacity,
                   (brick.table.numel() * 5) / 1e6))

    # ---- ray-casting: the one-call volumes; the brick volume against its own densified copy for the bits
    same_dense = brick.to_dense(((0, 0, 0), brick.dims), dims_limit=n1)
    W, H = 1920, 1080
    Kb = np.array([[0.9 * W, 0, (W - 1) / 2], [0, 0.9 * W, (H - 1) / 2], [0, 0, 1]])
    for name, K, P, size in (("%d views of %dx%d in ONE launch" % (t, hw, hw), Ks, Ps, (hw, hw)), ("one %dx%d view" % (W, H), Kb, Ps[0], (H, W))):
        td, tb, ts = dense.view_table(K, P, size), brick.view_table(K, P, size), same_dense.view_table(K, P, size)
        a, b = timed(lambda: dense.raycast_table(td)), timed(lambda: brick.raycast_table(tb))
        same_dense.raycast_table(ts)
        bits = all(torch.equal(tb[3][k].contiguous().view(torch.uint8), ts[3][k].contiguous().view(torch.uint8)) for k in tb[3])
        hits = (float((td[3]["depth"] > 0).float().mean()), float((tb[3]["depth"] > 0).float().mean()))
        row("dense: sp3_tsdf_raycast, %s, prepared table" % name, a, "%.1f %% of the rays hit" % (100 * hits[0]))
        row("bricks: sp3_tsdf_brick_raycast, %s, prepared table" % name, b,
            "%.2f x dense; %.1f %% hit; same bits as the dense ray-caster on to_dense(): %s" % (b[0] / a[0], 100 * hits[1], bits))
    del same_dense

    # ---- tracked fusion end to end
    if tracked:
        pts = torch.from_numpy(np.stack([world_points(f, hw) for f in frames])).cuda()
        lo, hi = torch.tensor(dense.origin).cuda(), torch.tensor(dense.origin + voxel * (n1 - 1)).cuda()
        val = torch.stack(valid).bool() & ((pts >= lo) & (pts <= hi)).all(-1)
        img = torch.stack(images)
        K0, P = np.stack(Ks), np.stack(Ps)
        kw = dict(voxel_size=voxel, dims_max=2 * n1, track=True, return_volume=True)
        del dense, brick
        torch.cuda.empty_cache()
        a, out_d = host_ms(lambda: F.fuse_pointmaps(pts, K0, P, val, img, **kw))
        row("dense: fuse_pointmaps(track=True), %d frames, mesh included (host clock)" % t, a,
            "volume %s, %d faces" % (out_d[1].dims, out_d[0]["faces"].shape[0]))
        del out_d
        torch.cuda.empty_cache()
        b, out_b = host_ms(lambda: F.fuse_pointmaps(pts, K0, P, val, img, bricks=True, **kw))
        row("bricks: fuse_pointmaps(track=True, bricks=True), %d frames, mesh through to_dense included (host clock)" % t, b,
            "%.2f x dense; grid %s, %d bricks, %d faces" % (b[0] / a[0], out_b[1].dims, out_b[1].n_bricks, out_b[0]["faces"].shape[0]))
        ext = (lo.cpu().numpy() - 1.0, hi.cpu().numpy() + 1.0)
        c, out_c = host_ms(lambda: F.fuse_pointmaps(pts, K0, P, val, img, bricks=True, extent=ext, **kw))
        row("bricks: the same inside an extent one unit wider on every side (the points are not consulted)", c,
            "%.2f x dense; grid %s, %d bricks, %.1f MB" % (c[0] / a[0], out_c[1].dims, out_c[1].n_bricks, out_c[1].memory_bytes / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512])
    args = ap.parse_args()
    rows = ["Brick TSDF volume against the dense volume (libspann3r_hip.so), device %s" % torch.cuda.get_device_name(0),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead and the brick path's read-backs included) "
            "unless a row says host clock; both paths in one process"]
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
