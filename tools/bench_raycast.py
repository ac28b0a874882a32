#!/usr/bin/env python
"""Timing record of the volume ray-caster and of tracked fusion (spann3r_amd/fusion.py, csrc/raycast.hip) on the scene of
tools/bench_fusion.py: 50 frames of 224x224 -- a sphere on a plane seen from a ring of cameras -- fused into a 256^3 volume with
colours.  Rows: the 50 views ray-cast in ONE launch and as 50 launches, one 1920x1080 view, and next to both the only other route
to the same pictures: extract_mesh plus PointRenderer.add_triangles (device events around the calls, warmed up, repeated; the rows
marked `prepared` launch a descriptor table built outside, the others go through TSDFVolume.raycast and pay for the table and the
output buffers).  Then tracked fusion of the 50 frames through fuse_pointmaps(track=True), host clock around the whole call ending
in a synchronise, split by track_frame's own timers into ray-cast, accumulate (launch plus the read of 29 doubles), host solve and
the rest (integrate, transform, extraction), next to the untracked one-call fusion.  Nothing is asserted.  Writes the table to --out
(profiles/raycast.txt is the committed record)."""
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
from spann3r_amd import vis
from tools.bench_fusion import ring_frames
from tools.bench_render import timed


def world_points(f, hw):
    """the world pointmap fp32 [hw, hw, 3] of a ring frame's depth"""
    ys, xs = np.mgrid[0:hw, 0:hw]
    rays = np.stack([(xs - f["cu"]) / f["fu"], (ys - f["cv"]) / f["fv"], np.ones((hw, hw))], -1) @ f["cam2world"][:3, :3].T
    return (f["cam2world"][:3, 3] + rays * f["depth"].astype(np.float64)[..., None]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dims", type=int, default=256)
    args = ap.parse_args()
    t, hw, n1 = args.frames, args.size, args.dims
    rows = ["TSDF ray-casting and tracked fusion (libspann3r_hip.so), device %s" % torch.cuda.get_device_name(0),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead included) unless a row says host clock",
            "--- %d frames of %dx%d fused into %d^3 voxels (%.1f M), colours on, trunc 3 voxels, step 1 voxel" % (t, hw, hw, n1, n1 ** 3 / 1e6)]

    def row(name, tm, extra=""):
        med, lo, hi, reps = tm
        rows.append("%-84s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (name, med, lo, hi, reps, extra))

    frames = ring_frames(t, hw, hw)
    voxel = 2.4 / n1
    vol = F.TSDFVolume((-1.2, -1.2, -0.3), voxel, (n1, n1, n1))
    depth = [torch.from_numpy(f["depth"]).cuda() for f in frames]
    valid = [torch.from_numpy(f["valid"]).cuda() for f in frames]
    images = [torch.from_numpy(f["images"]).cuda() for f in frames]
    Ks, Ps = [f["K"] for f in frames], [f["cam2world"] for f in frames]
    vol.integrate(depth=depth, intrinsics=Ks, cam2world=Ps, valid=valid, images=images)

    # ---- the 50 views
    whole = vol.view_table(Ks, Ps, (hw, hw))
    singles = [vol.view_table(Ks[i], Ps[i], (hw, hw)) for i in range(t)]
    tm = timed(lambda: vol.raycast_table(whole))
    hit = float((whole[3]["depth"] > 0).float().mean())
    row("sp3_tsdf_raycast, %d views in ONE launch, prepared table (depth, vertex, normal, rgba)" % t, tm,
        "%.3e rays/s; %.1f %% of the rays hit" % (t * hw * hw / (tm[0] * 1e-3), 100 * hit))
    tm2 = timed(lambda: [vol.raycast_table(s) for s in singles])
    row("sp3_tsdf_raycast, %d one-view launches, prepared tables" % t, tm2, "%.2f x the one launch" % (tm2[0] / tm[0]))
    same = all(torch.equal(torch.cat([s[3][k] for s in singles]), whole[3][k]) for k in whole[3])
    rows.append("  one launch and %d launches give the same bits: %s" % (t, same))
    tm3 = timed(lambda: vol.raycast(Ks, Ps, (hw, hw)))
    row("TSDFVolume.raycast, %d views (table, its upload and the output buffers included)" % t, tm3)
    tm3d = timed(lambda: vol.raycast_table(vol.view_table(Ks, Ps, (hw, hw), vertices=False, normals=False, colors=False)))
    row("TSDFVolume.raycast, %d views, depth only" % t, tm3d)

    # ---- the other route: the mesh, rasterised
    tm4 = timed(lambda: vol.extract_mesh())
    row("extract_mesh (the other route's first half, once per volume)", tm4)
    mesh = vol.extract_mesh()
    cams = [vis.Camera(Ks[i], np.linalg.inv(Ps[i]), hw, hw) for i in range(t)]

    def raster_all():
        for c in cams:
            r = vis.PointRenderer(camera=c)
            r.add_triangles(mesh["vertices"], mesh["faces"], mesh["colors"])
            r.image(return_depth=True)

    tm5 = timed(raster_all)
    row("PointRenderer.add_triangles + image(return_depth), %d views of the %d-face mesh" % (t, mesh["faces"].shape[0]), tm5,
        "mesh route %.3f ms against %.3f ms ray-cast: %.2f x" % (tm4[0] + tm5[0], tm3[0], (tm4[0] + tm5[0]) / tm3[0]))

    # ---- one large view
    W, H = 1920, 1080
    Kb = np.array([[0.9 * W, 0, (W - 1) / 2], [0, 0.9 * W, (H - 1) / 2], [0, 0, 1]])
    big = vol.view_table(Kb, Ps[0], (H, W))
    tm6 = timed(lambda: vol.raycast_table(big))
    row("sp3_tsdf_raycast, one %dx%d view, prepared table" % (W, H), tm6,
        "%.3e rays/s; %.1f %% hit" % (W * H / (tm6[0] * 1e-3), 100 * float((big[3]["depth"] > 0).float().mean())))
    cam_b = vis.Camera(Kb, np.linalg.inv(Ps[0]), W, H)

    def raster_big():
        r = vis.PointRenderer(camera=cam_b)
        r.add_triangles(mesh["vertices"], mesh["faces"], mesh["colors"])
        r.image(return_depth=True)

    tm7 = timed(raster_big)
    row("PointRenderer.add_triangles + image(return_depth), the same view of the mesh", tm7,
        "mesh route %.3f ms against %.3f ms: %.2f x" % (tm4[0] + tm7[0], tm6[0], (tm4[0] + tm7[0]) / tm6[0]))

    # ---- tracked fusion
    pts = torch.from_numpy(np.stack([world_points(f, hw) for f in frames])).cuda()
    lo, hi = torch.tensor(vol.origin).cuda(), torch.tensor(vol.origin + voxel * (n1 - 1)).cuda()
    val = torch.stack(valid).bool() & ((pts >= lo) & (pts <= hi)).all(-1)          # the points inside the box of the volume above
    img = torch.stack(images)
    K0, P = np.stack(Ks), np.stack(Ps)
    kw = dict(voxel_size=voxel, dims_max=2 * n1)

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

    tm8, plain = host_ms(lambda: F.fuse_pointmaps(pts, K0, P, val, img, return_volume=True, **kw))
    row("fuse_pointmaps, untracked: one integrate launch, extract_mesh (host clock)", tm8, "volume %s" % (plain[1].dims,))
    timers = {}
    tm9, tracked = host_ms(lambda: F.fuse_pointmaps(pts, K0, P, val, img, return_volume=True, track=True, return_poses=True,
                                                   track_args=dict(timings=timers), **kw))
    mesh_t, vol_t = tracked
    calls = 4                                                                    # host_ms ran it reps + 1 times
    part = {k: timers.get(k, 0.0) * 1e3 / calls for k in ("raycast", "accumulate", "solve")}
    trips = timers.get("round_trips", 0) / calls
    row("fuse_pointmaps, track=True: %d frames registered, then integrated one by one (host clock)" % (t - 1), tm9,
        "%.1f x untracked; %d ray-casts, %d integrate launches" % (tm9[0] / tm8[0], vol_t.raycasts, vol_t.launches))
    rest = tm9[0] - sum(part.values())
    rows.append("  of which, host clock per call: ray-cast %.2f ms, accumulate + read-back of 29 doubles %.2f ms, host solve %.2f ms, "
                "integrate / transform / extract and the rest %.2f ms; %.1f host round trips per frame"
                % (part["raycast"], part["accumulate"], part["solve"], rest, trips / (t - 1)))
    ang = [np.degrees(np.arccos(np.clip((np.trace(T[:3, :3]) - 1) / 2, -1, 1))) for T in mesh_t["corrections"][1:]]
    rows.append("  %d of %d frames tracked; exact poses in, so the corrections are the tracker's own bias: largest %.4f degrees, %.3f voxels"
                % (sum(mesh_t["tracked"][1:]), t - 1, max(ang), max(np.linalg.norm(T[:3, 3]) for T in mesh_t["corrections"][1:]) / voxel))
    text = "\n".join(rows)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
