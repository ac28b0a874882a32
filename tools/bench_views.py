#!/usr/bin/env python
"""Timing record of the RGB-D view builder (spann3r_amd/views.py, csrc/views.hip, csrc/preproc.hip): 20 views of 480x640 with uint16
depth to 224x224, the batch of the 0.168 s training step.  Device: build_views timed with device events around a synchronised
window after warm-up, from host arrays (the raw bytes cross PCIe inside the window) and from arrays already on the device.  Host:
the numpy + Pillow statement of the same work (Pillow's crop / LANCZOS resize / crop and ImgNorm for the image, tests/views_ref.py
for the depth side) on this machine's CPU, one thread, in the same call, for scale.  Bytes moved per view and the share of the
HBM bandwidth they amount to are printed with the formula.  Nothing is asserted.  Writes the table to --out
(profiles/views.txt is the committed record)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from spann3r_amd import views as V

HBM_BYTES_PER_S = 8.0e12          # MI355X: 8 TB/s peak


def scene(n, H, W):
    import views_ref as VR
    rng = np.random.default_rng(0)
    K = np.array([[525.0, 0, 320.0], [0, 525.0, 240.0], [0, 0, 1]], np.float32)          # the 7Scenes intrinsics
    rgbs = [VR.seeded_image(H, W, s) for s in range(n)]
    depths = []
    for _ in range(n):
        d = rng.integers(400, 9000, (H, W)).astype(np.uint16)
        d[rng.random((H, W)) < 0.05] = 65535
        depths.append(d)
    poses = []
    for _ in range(n):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = q, rng.uniform(-1, 1, 3)
        poses.append(T)
    return rgbs, depths, [K] * n, poses


def device_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), min(ts), max(ts)


def host_view(rgb, depth, K, pose, res, kw):
    from PIL import Image
    import views_ref as VR
    p = V.plan_rgbd_view(depth.shape[0], depth.shape[1], K, res)
    im = Image.fromarray(rgb).crop(p["crop0"]).resize(p["resize"], resample=Image.LANCZOS).crop(p["crop1"])
    img = ((np.asarray(im).astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1)
    return (img,) + VR.view_depth_ref(depth, p, pose, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--resolution", type=int, default=224)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, H, W, res = args.views, args.height, args.width, args.resolution
    kw = dict(depth_div=1000.0, raw_invalid=65535, min_depth=1e-3, max_depth=10.0)
    rgbs, depths, Ks, poses = scene(n, H, W)
    rows = ["RGB-D view builder (libspann3r_hip.so), device %s" % torch.cuda.get_device_name(0),
            "%d views of %dx%d, uint16 depth -> %dx%d; times: median [min .. max] x%d after %d warm-up calls, device events around a "
            "synchronised window (launch overhead and, where stated, the host-to-device copies included)" % (n, W, H, res, res, args.reps, args.warmup)]

    def line(name, t, per=n):
        rows.append("%-78s %9.3f ms  [%9.3f .. %9.3f]   %8.4f ms/view  %9.0f views/s" % (name, t[0], t[1], t[2], t[0] / per, per / (t[0] * 1e-3)))

    before = V.LAUNCHES["sp3_view_depth"]
    t_host = device_ms(lambda: V.build_views(rgbs, depths, Ks, poses, resolution=res, **kw), args.warmup, args.reps)
    launches = V.LAUNCHES["sp3_view_depth"] - before
    line("build_views from host arrays (raw bytes cross PCIe in the window)", t_host)
    rgbs_d = [torch.from_numpy(x).cuda() for x in rgbs]
    depths_d = [torch.from_numpy(x.view(np.int16)).cuda().view(torch.uint16) for x in depths] if hasattr(torch, "uint16") else None
    if depths_d is not None:
        t_dev = device_ms(lambda: V.build_views(rgbs_d, depths_d, Ks, poses, resolution=res, **kw), args.warmup, args.reps)
        line("build_views from arrays already on the device", t_dev)
    else:
        t_dev = None
        rows.append("build_views from arrays already on the device: not measured (no torch.uint16)")
    rows.append("sp3_view_depth launches per build_views call: %.0f" % (launches / (args.warmup + args.reps)))
    p = V.plan_rgbd_view(H, W, Ks[0], res)
    W1, H1 = p["crop0"][2] - p["crop0"][0], p["crop0"][3] - p["crop0"][1]
    img_bytes = W1 * H1 * 3 + 2 * H1 * p["resize"][0] * 3 + res * res * 3 * 4          # source window read, 8-bit intermediate written + read, fp32 out
    depth_bytes = res * res * (2 + 4 + 12 + 1)                                         # one raw sample read; depth, point, mask written
    rows.append("bytes moved per view, lower bound: image %d (crop window read, 8-bit intermediate written and read, fp32 image written) + "
                "depth side %d (2 read, 17 written per pixel) = %d; raw bytes over PCIe per view: %d"
                % (img_bytes, depth_bytes, img_bytes + depth_bytes, H * W * 5))
    if t_dev is not None:
        share = (img_bytes + depth_bytes) * n / (t_dev[0] * 1e-3) / HBM_BYTES_PER_S
        rows.append("share of HBM bandwidth = bytes per view x views / device-resident time / %.1e B/s = %.4f %% (the call is %d small launches: "
                    "launch-bound, not bandwidth-bound)" % (HBM_BYTES_PER_S, 100 * share, 2 * n + 1))
    else:
        rows.append("share of HBM bandwidth: not measured")
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    ref = [host_view(rgbs[i], depths[i], Ks[i], poses[i], res, kw) for i in range(n)]
    t_cpu = (time.perf_counter() - t0) * 1e3
    rows.append("numpy + Pillow statement of the same work on this machine's CPU, host clock, one run, one thread: %.1f ms = %.2f ms/view "
                "(%.0f views/s) -> %.0f x the device path from host arrays" % (t_cpu, t_cpu / n, n / (t_cpu * 1e-3), t_cpu / t_host[0]))
    views = V.build_views(rgbs, depths, Ks, poses, resolution=res, **kw)
    same = all(np.array_equal(v["img"][0].cpu().numpy(), r[0]) and np.array_equal(v["depthmap"][0].cpu().numpy(), r[1])
               and np.array_equal(v["pts3d"][0].cpu().numpy(), r[3]) and np.array_equal(v["valid_mask"][0].cpu().numpy(), r[4])
               for v, r in zip(views, ref))
    rows.append("device equals the host statement (img, depthmap, pts3d, valid_mask): %s" % same)
    rows.append("for scale: the training step these views feed takes 0.168 s for 20 views (profiles/r06_training_step_time.txt)")
    text = "\n".join(rows) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
