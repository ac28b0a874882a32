#!/usr/bin/env python
"""Timing record of the reconstruction-metric kernels (spann3r_amd/evaluate.py, csrc/eval.hip) at the size one eval.py scene has:
N x N points of a surface-like cloud (50 frames of 224^2 are 2.5 M; the default here is 1 M).  Device events around warmed-up
repeats that fill about a second per row; nothing is asserted.  Writes the table to --out (profiles/eval_metrics_nn.txt is the
committed record) and prints it."""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from spann3r_amd import evaluate as E
from spann3r_amd import lib as L


def clouds(n, seed=0):
    """gt on z = 0.3 sin(3u) cos(2v) over [-1, 1]^2; rec = gt + N(0, 0.01) noise, its first 0.01 % moved far outside the box"""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-1, 1, (2, n))
    gt = np.stack((u, v, 0.3 * np.sin(3 * u) * np.cos(2 * v)), 1)
    rec = gt + rng.normal(0, 0.01, gt.shape)
    rec[:max(n // 10000, 1)] += 5.0
    return gt.astype(np.float32), rec.astype(np.float32)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--brute-queries", type=int, default=50000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_metrics: needs the GPU (nothing here is measured on a CPU)")
    n = a.n
    gt_h, rec_h = clouds(n)
    gt, rec = torch.from_numpy(gt_h).cuda(), torch.from_numpy(rec_h).cuda()
    lib = L.load()
    rows, notes = [], []

    def row(name, t, work=None, unit=""):
        med, lo, hi, reps = t
        rate = "" if work is None else "%10.3e %s" % (work / (med * 1e-3), unit)
        rows.append("%-46s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (name, med, lo, hi, reps, rate))

    # grid build (bounding box, cell ids, sort, records, cell-start table)
    grid = E.CellGrid(gt)
    row("grid build (%d pts)" % n, timed(lambda: E.CellGrid(gt)), n, "points/s")
    # 1-NN query: rec -> gt (queries sorted by cell, rings, brute-force second pass)
    ws = torch.empty(lib.sp3_nn_query_ws_bytes(n), dtype=torch.uint8, device="cuda")
    grid.nn(rec, ws=ws)
    fb, cells, points = E._read_counters(ws)
    t_grid = timed(lambda: grid.nn(rec, ws=ws))
    row("1-NN grid query (%d x %d)" % (n, n), t_grid, float(n) * n, "point-pairs/s (N*M over time)")
    rows.append("%-46s %10.3e pairs/s evaluated (points visited over time)" % ("", points / (t_grid[0] * 1e-3)))
    order = grid.query_order(rec)
    dist, idx = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")

    def kernels_only():
        L.check(lib.sp3_nn_query(rec.data_ptr(), order.data_ptr(), n, grid.recs.data_ptr(), grid.cell_start.data_ptr(), n, E.C.byref(grid.g),
                                 E.RING_BUDGET, math.inf, ws.data_ptr(), dist.data_ptr(), idx.data_ptr(), L.stream_ptr()), "sp3_nn_query")
    row("  of which sp3_nn_query alone (queries pre-sorted)", timed(kernels_only))
    # brute force on a slice, scaled
    nb = min(a.brute_queries, n)
    sl = rec[n // 2:n // 2 + nb].contiguous() if n // 2 + nb <= n else rec[:nb].contiguous()
    bgrid = E.CellGrid(gt, brute=True)
    t_br = timed(lambda: bgrid.nn_brute(sl))
    row("brute-force kernel (%d x %d slice)" % (nb, n), t_br, float(nb) * n, "point-pairs/s")
    br_scaled = t_br[0] * n / nb
    rows.append("%-46s %10.3f ms  (slice time x %g: SCALED, not run at full size)" % ("brute-force kernel scaled to %d queries" % n, br_scaled, n / nb))
    # one ICP iteration; an evaluation = transform, match within 0.1, 17 sums, read back; the update = 3x3 SVD on the host
    row("ICP, max_iteration=1 (grid build, 2 evaluations, 1 update)", timed(lambda: E.icp_point_to_point(rec, gt, 0.1, max_iteration=1)))
    row("estimate_normals(knn=30) (%d pts)" % n, timed(lambda: E.estimate_normals(gt), budget=2.0), n, "points/s")

    # the same queries through scipy's KD-tree on this machine's CPU
    kd = None
    if not a.no_scipy:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            cKDTree = None
        if cKDTree is None:
            notes.append("scipy does not import here: cKDTree not measured")
        else:
            gt64, rec64 = gt_h.astype(np.float64), rec_h.astype(np.float64)
            t0 = time.perf_counter()
            tree = cKDTree(gt64)
            t_build = (time.perf_counter() - t0) * 1e3
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                d_kd, _ = tree.query(rec64, workers=16)
                ts.append((time.perf_counter() - t0) * 1e3)
            kd = (float(np.median(ts)), min(ts), max(ts), 3)
            rows.append("%-46s %10.3f ms" % ("cKDTree build (CPU, float64)", t_build))
            row("cKDTree.query(workers=16) (CPU, host clock)", kd, float(n) * n, "point-pairs/s (N*M over time)")
            err = np.abs(dist.cpu().numpy().astype(np.float64) - d_kd)
            bound = 8 * 2.0 ** -24 * max(np.abs(gt_h).max(), np.abs(rec_h).max()) + 4 * 2.0 ** -24 * d_kd
            notes.append("grid distances vs cKDTree at this size: worst |d - d64| = %.3e, %.3f of the fp32 bound" % (err.max(), (err / bound).max()))

    g = grid.g
    per_q = (points * 16 + cells * 8 + n * (12 + 8 + 8)) / n
    head = ["reconstruction-metric kernels, %d x %d points (surface cloud, rec = gt + N(0, 0.01), %d far outliers), device %s"
            % (n, n, max(n // 10000, 1), torch.cuda.get_device_name(0)),
            "grid %d x %d x %d = %d cells, h = %.5f; ring budget %d" % (g.nx, g.ny, g.nz, g.nx * g.ny * g.nz, g.h, E.RING_BUDGET),
            "per query (grid path): %.1f cells and %.1f points visited on average; %.0f bytes fetched (16 B per record visited, 8 B per cell-table"
            " pair, 28 B of query / order / result), from shapes and the kernel's own counters" % (cells / n, points / n, per_q),
            "fallback share: %d of %d queries (%.4f %%) went to the brute-force second pass" % (fb, n, 100.0 * fb / n),
            "times: median [min .. max] x repeats, device events (cKDTree: host clock)", ""]
    spread = (t_grid[2] - t_grid[1])
    verdict = []
    if kd is not None:
        gap = kd[1] - t_grid[2]
        verdict.append("grid path vs cKDTree on 16 threads: %.1f ms against %.1f ms -> %s (gap %.1f ms, run-to-run spread %.1f ms + %.1f ms)"
                       % (t_grid[0], kd[0], "beats it by more than the spread" if gap > 0 else "does NOT beat it beyond the spread", gap, spread, kd[2] - kd[1]))
    else:
        verdict.append("grid path vs cKDTree on 16 threads: not measured")
    gap = br_scaled * (t_br[1] / t_br[0]) - t_grid[2]
    verdict.append("grid path vs in-tree brute force (scaled): %.1f ms against %.1f ms -> %s"
                   % (t_grid[0], br_scaled, "beats it by more than the spread" if gap > 0 else "does NOT beat it beyond the spread"))
    text = "\n".join(head + rows + [""] + verdict + notes) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
