#!/usr/bin/env python
"""Writes tests/golden/vis_colormaps.npz from the installed matplotlib (3.10): what spann3r/tools/vis.py:168-169 and 188-189 compute.

  jet_lut   uint8 [256, 4]   plt.cm.jet's 256-entry table as (rgba * 255).astype(uint8)
  hsv_x     fp32 [4096, 3]   seeded inputs in [0, 1]; the first rows hold the exact values 0, 1 and the sector edges 1 - k / 6
  hsv_rgb   uint8 [4096, 3]  (matplotlib.colors.hsv_to_rgb(1 - x) * 255).astype(uint8)
  hsv_f64   fp64 [4096, 3]   hsv_to_rgb of the same fp32 (h, s, v) = 1 - x evaluated in float64
  hsv_near  bool [4096, 3]   |255 * hsv_f64 - nearest integer| <= 255 * 8 * 2^-24

hsv_near marks the entries where an evaluation in fp32 may truncate to the neighbouring level.  Both evaluations start from the same
fp32 (h, s, v) = 1 - x; from there a channel takes at most 8 individually rounded fp32 operations (h * 6, the subtraction of the
sector, 1 - f, the product with s, 1 - that, the product with v, * 255, one to spare), each off by at most 2^-24 of a value of at most
1, hence 255 * 8 * 2^-24 = 1.2e-4 levels.  The script insists that under 1 % of the entries are marked, so the allowance cannot hide a
wrong formula (try another seed otherwise)."""
import os
import sys

import matplotlib
import matplotlib.colors as mcolors
import matplotlib.pyplot as plt
import numpy as np

SEED = 0


def main():
    rng = np.random.default_rng(SEED)
    x = rng.random((4096, 3), dtype=np.float32)
    edges = np.array([0.0, 1.0] + [1.0 - k / 6.0 for k in range(7)], np.float32)         # 1 - x = k / 6 up to fp32 rounding
    x[:len(edges), 0] = edges
    x[:len(edges), 1] = rng.random(len(edges), dtype=np.float32)
    x[len(edges):2 * len(edges)] = edges[:, None]                                        # all three channels at the special values
    x[2 * len(edges), :] = (0.25, 1.0, 0.5)                                              # s = 0: grey
    x[2 * len(edges) + 1, :] = (0.25, 0.5, 1.0)                                          # v = 0: black
    hsv32 = (1 - x).astype(np.float32)
    rgb = (mcolors.hsv_to_rgb(hsv32) * 255).astype(np.uint8)
    f64 = mcolors.hsv_to_rgb(hsv32.astype(np.float64))
    near = np.abs(255 * f64 - np.rint(255 * f64)) <= 255 * 8 * 2.0 ** -24
    share = float(near.mean())
    # exact-valued channels (v itself at 0 or 1, p at s = 1, ...) sit on an integer by construction; count the share anyway
    print("matplotlib %s, near-integer entries: %d of %d (%.3f %%)" % (matplotlib.__version__, near.sum(), near.size, 100 * share))
    if share >= 0.01:
        sys.exit("more than 1 % of the entries are near an integer: choose another seed")
    jet = (plt.cm.jet(np.arange(256)) * 255).astype(np.uint8)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vis_colormaps.npz")
    np.savez_compressed(out, jet_lut=jet, hsv_x=x, hsv_rgb=rgb, hsv_f64=f64, hsv_near=near)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
