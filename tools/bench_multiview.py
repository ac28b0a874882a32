#!/usr/bin/env python
"""Timing record of the multi-view consistency sweep (spann3r_amd/multiview.py, csrc/multiview.hip) on the fusion bench's scene
(tools/bench_fusion.py): 50 frames of 224x224 -- a sphere on a plane seen from a ring of cameras -- as world pointmaps with their 50
cameras and a random confidence per pixel: T (T - 1) h w = 123 M lookups.  Rows: the counts launch, the sequence-order cleaning (T
launches), the parallel order (device events around the calls, warmed up, repeated; descriptor tables and buffers prepared outside),
and the route a user had before, in the same process: a torch loop over frame pairs on the device, written from the rule of
include/spann3r_hip.h, with its time and peak memory and whether its results equal the kernel's.  Nothing is asserted.  Writes the
table to --out (profiles/multiview.txt is the committed record)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from spann3r_amd import lib as L, multiview as MV
from tools.bench_fusion import ring_frames
from tools.bench_render import timed


def world_points(f):
    """the frame's depth map back-projected through its own K and pose: fp32 [h, w, 3]"""
    h, w = f["depth"].shape
    ys, xs = np.mgrid[0:h, 0:w]
    d = f["depth"].astype(np.float64)
    cam = np.stack([(xs - f["cu"]) / f["fu"] * d, (ys - f["cv"]) / f["fv"] * d, d], -1)
    return (cam @ f["cam2world"][:3, :3].T + f["cam2world"][:3, 3]).astype(np.float32)


def torch_pairs(pts, valid, conf, fk, w2c, tol, max_bad_conf, order):
    """The rule as a loop over frame pairs in eager torch (every elementwise op is its own kernel, so every fp32 operation is rounded
    on its own): -> (counts int32 [t, h, w, 4], cleaned confidence fp32 [t, h, w])"""
    t, h, w, _ = pts.shape
    counts = torch.zeros((t, h, w, 4), dtype=torch.int32, device=pts.device)
    out = conf.clone()
    tlo, thi = torch.tensor(1.0, device=pts.device) - tol, torch.tensor(1.0, device=pts.device) + tol
    for i in range(t):
        x, y, z = pts[i].unbind(-1)
        bad = torch.zeros((h, w), dtype=torch.bool, device=pts.device)
        for j in range(t):
            if j == i:
                continue
            m, (fu, fv, cu, cv) = w2c[j], fk[j]
            zc = ((m[8] * x + m[9] * y) + m[10] * z) + m[11]
            xc = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]
            yc = ((m[4] * x + m[5] * y) + m[6] * z) + m[7]
            ok = (zc > 0) & valid[i]
            fpx, fpy = torch.floor(fu * xc / zc + cu + 0.5), torch.floor(fv * yc / zc + cv + 0.5)
            ok = ok & (fpx >= 0) & (fpx < w) & (fpy >= 0) & (fpy < h)
            p = torch.where(ok, fpy * w + fpx, torch.zeros_like(fpx)).long().reshape(-1)
            ok = ok & valid[j].reshape(-1)[p].reshape(h, w)
            Q = pts[j].reshape(-1, 3)[p]
            d = (((m[8] * Q[:, 0] + m[9] * Q[:, 1]) + m[10] * Q[:, 2]) + m[11]).reshape(h, w)
            ok = ok & torch.isfinite(d) & (d > 0)
            front = ok & (zc < tlo * d)
            agree = ok & ~front & ~(zc > thi * d)
            st = front & (conf[i] < conf[j].reshape(-1)[p].reshape(h, w))
            counts[i] += torch.stack([ok, agree, front, st], -1).int()
            bad |= front & (conf[i] < out[j].reshape(-1)[p].reshape(h, w)) if (order == "sequence" and j < i) else st
        out[i] = torch.where(bad, torch.minimum(conf[i], torch.tensor(max_bad_conf, device=pts.device)), conf[i])
    return counts, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--tol", type=float, default=0.01)
    args = ap.parse_args()
    t, hw, tol = args.frames, args.size, args.tol
    frames = ring_frames(t, hw, hw)
    rng = np.random.default_rng(1)
    pts = torch.from_numpy(np.stack([world_points(f) for f in frames])).cuda()
    valid = torch.from_numpy(np.stack([f["valid"] for f in frames])).cuda()
    conf = torch.from_numpy((1 + rng.uniform(0, 9, (t, hw, hw))).astype(np.float32)).cuda()
    Ks, Ps = [f["K"] for f in frames], [f["cam2world"] for f in frames]
    lookups = t * (t - 1) * hw * hw
    rows = ["Multi-view consistency (libspann3r_hip.so), device %s" % torch.cuda.get_device_name(0),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead included)",
            "--- %d frames of %dx%d, %d cameras, %.1f %% of the pixels valid, tol %g: %.1f M lookups" %
            (t, hw, hw, t, 100 * float(valid.float().mean()), tol, lookups / 1e6)]

    def row(name, tm, extra=""):
        med, lo, hi, reps = tm
        rows.append("%-72s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (name, med, lo, hi, reps, extra))

    table, table_d, T, keep = MV.frame_table(pts, Ks, Ps, valid, conf)
    lib = L.load()
    counts = torch.empty((t, hw, hw, 4), dtype=torch.int32, device="cuda")
    clean = {o: torch.empty_like(conf) for o in ("parallel", "sequence")}

    def table_of(with_counts, conf_out):
        out = (L.MultiviewOut * T)()
        for i in range(T):
            out[i].counts = counts[i].data_ptr() if with_counts else None
            out[i].conf_out = conf_out[i].data_ptr() if conf_out is not None else None
        return out, torch.frombuffer(bytearray(bytes(out)), dtype=torch.uint8).cuda()

    def call(fn, name, out):
        L.check(fn(table, table_d.data_ptr(), T, tol, out[0], out[1].data_ptr(), L.stream_ptr()), name)

    o_counts, o_par, o_seq = table_of(True, None), table_of(False, clean["parallel"]), table_of(False, clean["sequence"])
    o_both = table_of(True, clean["sequence"])
    tm = timed(lambda: call(lib.sp3_multiview_counts, "sp3_multiview_counts", o_counts))
    row("sp3_multiview_counts, all pairs in ONE launch", tm, "%.3e lookups/s; %.1f MB of counts written" %
        (lookups / (tm[0] * 1e-3), counts.numel() * 4 / 1e6))
    tm_par = timed(lambda: call(lib.sp3_multiview_counts, "sp3_multiview_counts", o_par))
    row("parallel-order cleaning (the counts launch, conf_out only)", tm_par)
    tm_seq = timed(lambda: call(lib.sp3_multiview_clean, "sp3_multiview_clean", o_seq))
    row("sp3_multiview_clean, sequence order: %d launches" % t, tm_seq, "%.2f x the one launch" % (tm_seq[0] / tm_par[0]))
    row("sp3_multiview_clean with counts", timed(lambda: call(lib.sp3_multiview_clean, "sp3_multiview_clean", o_both)))
    row("clean_confidence(order='sequence') from tensors: tables, buffers, launches", timed(lambda: MV.clean_confidence(pts, conf, Ks, Ps, valid, tol=tol)))
    call(lib.sp3_multiview_counts, "sp3_multiview_counts", o_counts)
    torch.cuda.synchronize()
    c = counts.reshape(-1, 4).long().sum(0).tolist()
    rows.append("  totals: seen %d, agree %d, front %d, behind %d, stronger %d; clipped: sequence %d, parallel %d, pixels that differ %d" %
                (c[0], c[1], c[2], c[0] - c[1] - c[2], c[3], int((clean["sequence"] != conf).sum()), int((clean["parallel"] != conf).sum()),
                 int((clean["sequence"] != clean["parallel"]).sum())))

    # the route a user had before
    fk = [tuple(torch.tensor(float(np.float32(v)), device="cuda") for v in (f["fu"], f["fv"], f["cu"], f["cv"])) for f in frames]
    w2c = [torch.tensor(list(e.w2c), dtype=torch.float32, device="cuda") for e in table]      # the matrices the kernel is given
    vb = valid.bool()
    rows.append("torch loop over the %d frame pairs on the device (eager, fp32), host clock around a synchronised run, one warm-up:" % (t * (t - 1)))
    for order in ("parallel", "sequence"):
        torch_pairs(pts[:3], vb[:3], conf[:3], fk, w2c, tol, 0.0, order)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        tc, to = torch_pairs(pts, vb, conf, fk, w2c, tol, 0.0, order)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated() - base
        dev_ms = (tm_par if order == "parallel" else tm_seq)[0] + tm[0]
        rows.append("  %-9s order, counts and cleaning: %8.1f ms = %.0f x the device's %.3f ms (counts + cleaning); peak memory %.1f MB above the inputs, "
                    "its %.1f MB of outputs included (the kernel: its outputs only); counts equal: %s, confidences equal: %s" %
                    (order, dt * 1e3, dt * 1e3 / dev_ms, dev_ms, peak / 1e6, (tc.numel() + to.numel()) * 4 / 1e6, bool(torch.equal(tc, counts)),
                     bool(torch.equal(to.view(torch.int32), clean[order].view(torch.int32)))))
    text = "\n".join(rows)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
