#!/usr/bin/env python
"""Write a synthetic RGB-D sequence in the layout `demo_loop.py --rgbd DIR` reads: DIR/frame_XXX.npz with rgb uint8 [H, W, 3],
depth uint16 [H, W] in millimetres (0 and 65535 = no measurement), K float32 [3, 3], pose float32 [4, 4] (cam2world).
The scene is a relief over a plane seen by a camera that slides sideways, so the frames are consistent views of one surface."""
import argparse
import os

import numpy as np


def frame(i, n, H, W, rng):
    fx = 0.82 * W
    K = np.array([[fx, 0, W / 2 - 0.5], [0, fx, H / 2 - 0.5], [0, 0, 1]], np.float32)
    tx = 0.8 * (i / max(n - 1, 1) - 0.5)
    pose = np.eye(4, dtype=np.float32)
    pose[0, 3] = tx
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    z = np.full((H, W), 2.0)
    for _ in range(6):                                              # fixed point of z = surface(X(z), Y(z))
        X, Y = (u - K[0, 2]) / fx * z + tx, (v - K[1, 2]) / fx * z
        z = 2.0 + 0.25 * np.sin(3.0 * X) * np.cos(2.5 * Y) + 0.1 * np.cos(7.0 * X + 1.0)
    depth = np.round(z * 1000.0).astype(np.uint16)
    holes = rng.random((H, W))
    depth[holes < 0.02] = 0
    depth[holes > 0.985] = 65535
    tex = 0.5 + 0.5 * np.stack((np.sin(9 * X), np.cos(7 * Y), np.sin(5 * (X + Y))), -1)
    rgb = np.clip(tex * 255 + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8)
    return dict(rgb=rgb, depth=depth, K=K, pose=pose)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    rng = np.random.default_rng(0)
    for i in range(args.frames):
        np.savez(os.path.join(args.out, "frame_%03d.npz" % i), **frame(i, args.frames, args.height, args.width, rng))
    print("wrote %d frames of %dx%d to %s" % (args.frames, args.width, args.height, args.out))


if __name__ == "__main__":
    main()
