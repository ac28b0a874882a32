#!/usr/bin/env python
"""Timing record of the global alignment (spann3r_amd/align.py, csrc/align.hip): 10 frames of 224x224 around a bumpy sheet (the
consistent scene of tests/align_ref.py at that size), complete symmetrised graph, E = 90.  Rows: sp3_align_loss_grad alone on prepared
tables; AlignLoss from tensors (small parameters to the host, tables, launch); one full iteration (parameter maps + launch + backward +
Adam); 300 iterations; init="mst" end to end; peak memory above the inputs -- and the route a user had before, in the same process:
the reference's formula as an eager torch module with autograd on the same device, its iteration time and peak memory, and the two
losses of every iteration pair.  Nothing is asserted.  Writes the table to --out (profiles/align.txt is the committed record)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import align_ref as R
from spann3r_amd import align as A
from tools.bench_render import timed


def torch_loss(al, Pi, Pj, Wi, Wj, ei, ej):
    """PointCloudOptimizer.forward with dist l1 as eager torch on stacked tensors (all images of one shape)"""
    pw, ad = al.get_pw_poses(), al.get_adaptors()[:, None]
    proj = torch.stack([p.reshape(-1, 3) for p in al.get_pts3d()])
    geo = lambda P: (ad * P) @ pw[:, :3, :3].transpose(1, 2) + pw[:, None, :3, 3]
    li = ((proj[ei] - geo(Pi)).norm(dim=-1) * Wi).sum() / al.problem.areas[0]
    lj = ((proj[ej] - geo(Pj)).norm(dim=-1) * Wj).sum() / al.problem.areas[1]
    return li + lj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=300)
    args = ap.parse_args()
    n, hw = args.frames, args.size
    sc = R.sheet_scene(n_cams=n, h=hw, w=hw)
    rows = ["Global alignment (libspann3r_hip.so), device %s" % torch.cuda.get_device_name(0),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead included) unless a host clock is named"]

    def row(name, tm, extra=""):
        med, lo, hi, reps = tm
        rows.append("%-78s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (name, med, lo, hi, reps, extra))

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    al = A.GlobalAligner(sc["pairs"])
    pb, be = al.problem, al.backend
    torch.cuda.synchronize()
    inputs = torch.cuda.memory_allocated() - base
    rows.append("--- %d frames of %dx%d, complete symmetrised graph: E = %d, %d items; inputs and parameters on the device %.1f MB" %
                (n, hw, hw, pb.E, 2 * pb.E, inputs / 1e6))
    t0 = time.perf_counter()
    al.init_minimum_spanning_tree()
    torch.cuda.synchronize()
    t_init = time.perf_counter() - t0
    t0 = time.perf_counter()
    al.init_minimum_spanning_tree()
    torch.cuda.synchronize()
    rows.append("init='mst' end to end (host clock): first call %.1f ms, second %.1f ms; loss after it %.3e" %
                (t_init * 1e3, (time.perf_counter() - t0) * 1e3, float(al().detach())))
    state = {k: v.detach().clone() for k, v in al.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in (al.pw_poses, al.im_poses, al.im_depthmaps, al.im_focals):
            p.add_((torch.randn(p.shape, generator=g) * 0.02).to(p.device))
    start = {k: v.detach().clone() for k, v in al.state_dict().items()}

    with torch.no_grad():
        tabs = be.tables(pb, *al.geometric_parameters())
    traffic = 2 * pb.E * hw * hw * 16 + n * hw * hw * 8
    tm = timed(lambda: be.launch(pb, tabs))
    row("sp3_align_loss_grad alone (prepared tables): loss launch + finishing launch", tm,
        "%.1f MB of P, W, d read and dL/dd written: %.2f TB/s" % (traffic / 1e6, traffic / (tm[0] * 1e-3) / 1e12))
    with torch.no_grad():
        row("AlignLoss forward from tensors: parameters to the host, tables, launch", timed(lambda: al()))

    opt = torch.optim.Adam([p for p in al.parameters() if p.requires_grad], lr=0.01, betas=(0.9, 0.9))

    def step(loss_fn):
        opt.zero_grad()
        out = loss_fn()
        out.backward()
        opt.step()
        return out
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    row("one full iteration: parameter maps + launch + backward + Adam", timed(lambda: step(al)))
    torch.cuda.synchronize()
    peak_dev = torch.cuda.max_memory_allocated() - before

    Pi, Pj = (torch.stack([p.reshape(-1, 3) for p in pb.P[s]]) for s in (0, 1))
    Wi, Wj = (torch.stack([w.reshape(-1) for w in pb.W[s]]) for s in (0, 1))
    ei, ej = (torch.tensor([p[s] for p in pb.ij], device="cuda") for s in (0, 1))
    eager = lambda: torch_loss(al, Pi, Pj, Wi, Wj, ei, ej)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    row("the route before: the same loss as eager torch with autograd, one full iteration", timed(lambda: step(eager)))
    torch.cuda.synchronize()
    peak_eager = torch.cuda.max_memory_allocated() - before
    rows.append("peak memory above the inputs during an iteration: kernel route %.1f MB (workspace %.1f MB included), eager torch %.1f MB "
                "(its stacked copies of P and W, %.1f MB, not counted)" %
                (peak_dev / 1e6, tabs["ws"].numel() * 8 / 1e6, peak_eager / 1e6, (Pi.numel() + Pj.numel() + Wi.numel() + Wj.numel()) * 4 / 1e6))

    traj = {}
    for name, fn in (("kernel", al), ("eager", eager)):
        al.load_state_dict(start)
        opt = torch.optim.Adam([p for p in al.parameters() if p.requires_grad], lr=0.01, betas=(0.9, 0.9))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = []
        for it in range(args.iters):
            for grp in opt.param_groups:
                grp["lr"] = A.cosine_schedule(it / args.iters, 0.01, 1e-6)
            losses.append(step(fn).detach())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        traj[name] = [float(x) for x in losses]
        rows.append("%d iterations, %s route (host clock, cosine schedule): %.1f ms = %.3f ms per iteration; loss %.4e -> %.4e" %
                    (args.iters, name, dt * 1e3, dt * 1e3 / args.iters, traj[name][0], traj[name][-1]))
    rel = [abs(a - b) / abs(b) for a, b in zip(traj["kernel"], traj["eager"])]
    rows.append("the two losses of every iteration pair, relative difference: iteration 0 %.2e, 1 %.2e, 10 %.2e, 100 %.2e, last %.2e, largest %.2e" %
                (rel[0], rel[min(1, len(rel) - 1)], rel[min(10, len(rel) - 1)], rel[min(100, len(rel) - 1)], rel[-1], max(rel)))
    al.load_state_dict(state)
    text = "\n".join(rows)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
