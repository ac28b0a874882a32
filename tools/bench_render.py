#!/usr/bin/env python
"""Timing record of the headless renderer (spann3r_amd/vis.py, csrc/render.hip): render_frames on the device only, no PNG writing.
Cases: 50 frames of 512x512 points into 1920x1080, growing and dynamic, and 10 frames of 224x224.  Device events around warmed-up
repeats that fill about a second per row; nothing is asserted.  Splat (colour packing + atomic z-test) and resolve are also timed on
their own; "key bytes" are 8 bytes per pixel a drawn point covers, i.e. what the splat offers to the z-buffer (with the load-first
pre-test only part of them reach an atomic; the library built with -DSP3_RENDER_PRETEST=0 sends all of them: run this tool once per
library, SP3_LIB_PATH selects it).  The CPU yardstick is the numpy restatement tests/render_ref.py on the same input (host clock).
Writes the table to --out (profiles/render_points.txt is the committed record; --append adds to it) and prints it."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from spann3r_amd import lib as L
from spann3r_amd import vis


def scene(t, h, w, seed=0):
    """t pointmaps [t, h, w, 3] of a wavy wall about 3 units away, seen by a camera that slides sideways by a fiftieth of its view per
    frame (consecutive frames overlap, as in a scan), with depth noise; colours from position"""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.linspace(-0.6, 0.6, h), np.linspace(-0.8, 0.8, w), indexing="ij")
    pts, cols = [], []
    for i in range(t):
        x = u * 3.0 + 0.1 * i
        y = v * 3.0 + 0.2 * math.sin(0.3 * i)
        z = 3.0 + 0.4 * np.sin(1.3 * x) * np.cos(1.7 * y) + rng.normal(0, 0.01, x.shape)
        pts.append(np.stack((x, y, z), -1))
        cols.append(np.stack((0.5 + 0.5 * np.sin(x), 0.5 + 0.5 * np.cos(2 * y), np.full_like(x, i / max(t - 1, 1))), -1))
    return np.stack(pts).astype(np.float32), np.stack(cols).astype(np.float32)


def timed(fn, budget=1.0, min_reps=3, max_reps=200):
    """ms per call over warmed-up repeats (device events), as (median, min, max, reps)"""
    fn()
    torch.cuda.synchronize()
    ts = []
    t_end = time.perf_counter() + budget
    while len(ts) < min_reps or (time.perf_counter() < t_end and len(ts) < max_reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), min(ts), max(ts), len(ts)


def case(t, h, w, rows, notes, cpu_frames):
    pts_h, cols_h = scene(t, h, w)
    pts, cols = torch.from_numpy(pts_h).cuda(), torch.from_numpy(cols_h).cuda()
    cam = vis.fit_camera(pts)
    n = h * w

    def row(name, tm, work=None, unit=""):
        med, lo, hi, reps = tm
        rate = "" if work is None else "%10.3e %s" % (work / (med * 1e-3), unit)
        rows.append("%-58s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (name, med, lo, hi, reps, rate))

    rows.append("--- %d frames of %dx%d points (%.2f M points) into %dx%d" % (t, h, w, t * n / 1e6, cam.width, cam.height))
    # covered pixels, from the picture's own rule on the host: points that land inside the image (point_size 1)
    import render_ref as RR
    rc = RR.Cam(cam.extrinsic[:3, :3], cam.extrinsic[:3, 3], cam.intrinsic[0, 0], cam.intrinsic[1, 1], cam.intrinsic[0, 2], cam.intrinsic[1, 2],
                cam.width, cam.height)
    uu, vv, _, ok = RR.project(pts_h.reshape(-1, 3), rc)
    inside = int((ok & (np.floor(uu + 0.5) >= 0) & (np.floor(uu + 0.5) < cam.width) & (np.floor(vv + 0.5) >= 0) & (np.floor(vv + 0.5) < cam.height)).sum())
    for dynamic in (False, True):
        tag = "dynamic" if dynamic else "growing"
        row("render_frames, %s (%d pictures)" % (tag, t), timed(lambda: vis.render_frames(pts, cols, cam, None, dynamic=dynamic)), t, "pictures/s")
        r = vis.PointRenderer(camera=cam, dynamic=dynamic)

        def splat_all():
            if not dynamic:
                r.clear()
            for i in range(t):
                r.add(pts[i], cols[i])
        row("  %s: clear + pack + splat of all %d frames" % (tag, t), timed(splat_all), inside * 8.0, "key bytes/s offered to the z-buffer")
    r = vis.PointRenderer(camera=cam)
    for i in range(t):
        r.add(pts[i], cols[i])
    lib, st = L.load(), L.stream_ptr()
    i_last = t - 1

    def splat_only():
        L.check(lib.sp3_render_splat(pts[i_last].data_ptr(), 0, 0.0, n, i_last * n, vis.C.byref(r.cam), r.keys.data_ptr(), st), "sp3_render_splat")
    row("  sp3_render_splat, one frame into the full buffer (re-drawn)", timed(splat_only), n, "points/s")
    fresh = vis.PointRenderer(camera=cam, dynamic=True)

    def clear_splat():
        fresh.clear()
        L.check(lib.sp3_render_splat(pts[0].data_ptr(), 0, 0.0, n, 0, vis.C.byref(fresh.cam), fresh.keys.data_ptr(), st), "sp3_render_splat")
    row("  sp3_render_clear + sp3_render_splat, one frame, empty buffer", timed(clear_splat), n, "points/s")
    # the whole cloud in ONE launch: the splat at a size where launches do not bound it.  Into an empty buffer every key of the
    # no-pre-test build goes through an atomic, so its "key bytes" are exactly the bytes through atomics.
    flat = pts.reshape(-1, 3)

    def clear_splat_cloud():
        fresh.clear()
        L.check(lib.sp3_render_splat(flat.data_ptr(), 0, 0.0, t * n, 0, vis.C.byref(fresh.cam), fresh.keys.data_ptr(), st), "sp3_render_splat")

    def resplat_cloud():
        L.check(lib.sp3_render_splat(flat.data_ptr(), 0, 0.0, t * n, 0, vis.C.byref(r.cam), r.keys.data_ptr(), st), "sp3_render_splat")
    t_clear = timed(fresh.clear)
    t_cs = timed(clear_splat_cloud)
    row("  clear + splat of the whole cloud in ONE launch, empty buffer", t_cs, inside * 8.0, "key bytes/s (clear included)")
    rows.append("%-58s %10.3f ms  %10.3e key bytes/s, %10.3e points/s (median minus the clear's median)"
                % ("    of which the splat", t_cs[0] - t_clear[0], inside * 8.0 / ((t_cs[0] - t_clear[0]) * 1e-3), t * n / ((t_cs[0] - t_clear[0]) * 1e-3)))
    row("  splat of the whole cloud in ONE launch, full buffer (re-drawn)", timed(resplat_cloud), inside * 8.0, "key bytes/s offered")
    row("  sp3_render_clear alone", timed(fresh.clear), fresh.keys.numel() * 8.0, "bytes/s")
    px = cam.width * cam.height
    row("  sp3_render_resolve (rgb only), full buffer", timed(r.image), px * (8 + 3.0), "bytes/s (keys in, rgb out; colour gathers not counted)")
    row("  sp3_render_resolve (rgb + depth + index)", timed(lambda: r.image(True, True)), px * (8 + 3 + 8.0), "bytes/s")
    rows.append("  points inside the image: %d of %d (%.1f %%); pixels drawn at the end: %d of %d"
                % (inside, t * n, 100.0 * inside / (t * n), int((r.image(False, True)[1] >= 0).sum()), px))
    # CPU yardstick: the numpy restatement, one picture of the first `cpu_frames` frames (host clock, one run)
    t0 = time.perf_counter()
    index, _ = RR.render(pts_h[:cpu_frames].reshape(-1, 3), rc)
    RR.resolve(index, cols_h[:cpu_frames].reshape(-1, 3))
    dt = (time.perf_counter() - t0) * 1e3
    rows.append("  numpy restatement (tests/render_ref.py), ONE picture of %d frames (%.2f M points), host clock: %10.1f ms"
                % (cpu_frames, cpu_frames * n / 1e6, dt))
    if cpu_frames == t:
        rc_i = r.image(False, True)[1].cpu().numpy()
        notes.append("%dx%dx%d: device index picture equals the restatement's on %.4f %% of the pixels (unsafe input: points near pixel "
                     "boundaries may differ)" % (t, h, w, 100.0 * float((rc_i == index).mean())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--label", default="product library")
    ap.add_argument("--small", action="store_true", help="a quick look: 5 frames of 128x128 only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render: needs the GPU (nothing here is measured on a CPU)")
    rows, notes = [], []
    head = ["headless renderer, %s (%s), device %s" % (a.label, os.path.basename(L.LIB_PATH), torch.cuda.get_device_name(0)),
            "times: median [min .. max] x repeats, device events around whole calls (launch overhead included); rates = work / median", ""]
    if a.small:
        case(5, 128, 128, rows, notes, 5)
    else:
        case(50, 512, 512, rows, notes, 50)
        case(10, 224, 224, rows, notes, 10)
    text = "\n".join(head + rows + [""] + notes) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
