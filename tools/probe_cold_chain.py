#!/usr/bin/env python
"""Cold-weight chain probe for the weight cache policy (sp3_weight_stream_set; spann3r_amd/csrc/weight_stream.cpp).

The micro-benchmarks replay ONE launch, i.e. on warm weights -- the one state in which streaming (non-temporal) weight loads look worse
and which the per-frame chain never is in.  Here a chain of launches of one instance, each over ITS OWN copy of the weights (more than
512 MB of copies in all, twice the MALL), is captured into one hipGraph in stream order, so every launch starts when the one before it
ends and meets its weights cold in HBM, as in the model.  Reported: us per launch (graph time / launches, launch boundaries included)
under mode 0 (default policy) and mode 2 (every streaming variant), per kernel family.  A guide for the table, not its judge: the
table is decided in the model.

  python tools/probe_cold_chain.py [--mb 544] [--reps 5] [--only gemm,conv,wide,qproj] [--tiles 35,37]"""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch

import gemm_desc_ref as R
from spann3r_amd import lib as L
from spann3r_amd import ops

DEV = "cuda"
BF = torch.bfloat16
NAMES = {30: "val q/k/v", 31: "dec q/k/v + cross k/v pair", 32: "val fc1", 33: "dec fc1", 34: "val proj / value_out", 35: "val fc2",
         36: "dec proj / cross proj", 37: "dec fc2", 38: "key MLP out", 39: "decoder_embed", 42: "key MLP hidden (split A)",
         40: "small-map conv 16x16 tile", 41: "small-map conv 32x32 tile"}


def time_chain(issue, n, reps):
    """issue(i) enqueues launch i on the current stream; -> {mode: us per launch} for modes 0 and 2"""
    l = L.load()
    before = l.sp3_weight_stream_get()
    res = {}
    try:
        for mode in (0, 2):
            L.check(l.sp3_weight_stream_set(mode), "sp3_weight_stream_set")
            issue(0)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for i in range(n):
                    issue(i)
            g.replay()                                   # (one untimed pass: every copy has been through the caches once, and out again)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                g.replay()
            t1.record()
            torch.cuda.synchronize()
            res[mode] = 1e3 * t0.elapsed_time(t1) / (reps * n)
            del g
    finally:
        l.sp3_weight_stream_set(before)
    return res


def report(family, what, n, wbytes, res):
    print("%-6s %-34s %4d launches x %6.2f MB W: default %7.2f us  stream %7.2f us  (%+5.1f %%)"
          % (family, what, n, wbytes / 1e6, res[0], res[2], 100.0 * (res[2] / res[0] - 1.0)), flush=True)


def gemm_rows(a):
    """one chain per lean tile of the bf16 224 x 224 step: the first row of the launch census on that tile (GEMMs: at most two 196-row
    sides; small-map convolutions: tiles 40 / 41, single launches and levels as recorded)"""
    l = L.load()
    rows = [(i + 1, json.loads(s)) for i, s in enumerate(open(os.path.join(REPO, "tests", "golden", "gemm_plan_table.jsonl")))]
    seen = set()
    for line, row in rows:
        t = row["tiles"][0]
        conv = t in (40, 41)
        if row["lean"] != 1 or "bf16_224" not in row["from"] or t not in NAMES or t in seen or conv != (a.family == "conv"):
            continue
        if a.tiles and t not in a.tiles:
            continue
        if any(d["M"] > (2048 if conv else 392) or d.get("dyn_n") for d in row["descs"]):
            continue
        seen.add(t)
        cases = [c.materialize(DEV) for c in R.row_cases(row, line)]
        base = [c.desc(L) for c in cases]
        wbytes = sum(c.bufs["W"].t.numel() * c.bufs["W"].t.element_size() for c in cases)
        n = max(8, int(a.mb * 1e6 / wbytes) + 1)
        copies, descs = [], []
        for i in range(n):
            ds = []
            for c, d in zip(cases, base):
                w = c.bufs["W"].t.clone()
                copies.append(w)
                d2 = L.GemmDesc.from_buffer_copy(d)
                d2.W = w.data_ptr() + R.GUARD * w.element_size()
                ds.append(d2)
            descs.append(ds)
        arrs = [(C.POINTER(L.GemmDesc) * len(ds))(*[C.pointer(d) for d in ds]) for ds in descs]

        def issue(i):
            if len(descs[i]) == 1:
                L.check(l.sp3_gemm(C.byref(descs[i][0]), L.stream_ptr()), "sp3_gemm")
            else:
                L.check(l.sp3_gemm_n(arrs[i], len(descs[i]), L.stream_ptr()), "sp3_gemm_n")
        d0 = row["descs"][0]
        what = "tile %d %s M=%d N=%d K=%d%s" % (t, NAMES[t], d0["M"], d0["N"], d0["K"], " x%d" % max(d0.get("batch", 1), 1) if len(cases) == 1 else " pair")
        report(a.family, what, n, wbytes, time_chain(issue, n, a.reps))
        del copies, descs, arrs, cases, base
        torch.cuda.empty_cache()


def wide(a):
    """the wide 3x3 convolution at the head's maps (bf16, 256 -> 256): 56 x 56 (32-channel instance) and 112 x 112 (64-channel instance)"""
    g = torch.Generator().manual_seed(1)
    for hw in (56, 112):
        Cc = 256
        x = (torch.rand(1, hw, hw, Cc, generator=g) * 2 - 1).to(DEV).to(BF)
        out = torch.zeros(1, hw, hw, Cc, device=DEV, dtype=BF)
        w0 = ((torch.rand(Cc, 9 * Cc, generator=g) * 2 - 1) * 0.05).to(DEV).to(BF)
        wbytes = w0.numel() * 2
        n = int(a.mb * 1e6 / wbytes) + 1
        ws = [ops.PackedWeight(w0.clone()) for _ in range(n)]
        issue = lambda i: ops.conv3x3(x, ws[i], out, B=1, H=hw, W_=hw, Cin=Cc, Cout=Cc, stride=1, relu_in=True)
        report("wide", "%d x %d, 256 -> 256" % (hw, hw), n, wbytes, time_chain(issue, n, a.reps))
        del ws
        torch.cuda.empty_cache()


def qproj(a):
    """the decoder's cross-attention with its q projection inside: both sides of one frame, 12 heads, 196 tokens"""
    from spann3r_amd.engine import _rope_tables
    g = torch.Generator().manual_seed(2)
    rnd = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    B, nh, nw, D, heads = 1, 14, 14, 768, 12
    P = nh * nw
    npad = (P + 63) // 64 * 64
    xg = ops.PackedAct.group(2, P, D, BF, DEV)
    stg = torch.zeros(2, P, D // 32, 2, device=DEV)
    for s_ in (0, 1):
        ops.pack_stats((rnd(P, D) * 2 + 0.2).to(DEV), xg.at(s_), stg[s_], rows=P, C_=D)
    sg, bg = rnd(2, D).to(DEV).contiguous(), rnd(2, D).to(DEV).contiguous()
    yy, xx = torch.meshgrid(torch.arange(nh), torch.arange(nw), indexing="ij")
    pos = torch.stack([yy, xx], -1).reshape(-1, 2).to(torch.int32).to(DEV)
    cos, sin = _rope_tables(64, 100.0, DEV)
    kp = ops.PackedAct.from_dense((rnd(2 * B * npad, D) * 1.5).to(DEV).to(BF))
    vtp = rnd(2 * B * heads * npad * 64).to(DEV).to(BF)
    got = ops.PackedAct.group(2, P, D, BF, DEV)
    wbytes = 2 * D * D * 2
    n = int(a.mb * 1e6 / wbytes) + 1
    w0 = (rnd(D, D) * 0.05).to(DEV).to(BF)
    wgs = [ops.PackedWeightGroup([ops.PackedWeight(w0.clone()), ops.PackedWeight(w0.clone())]) for _ in range(n)]
    issue = lambda i: ops.attention_packed_qproj(xg, stg, wgs[i], sg, bg, pos, cos, sin, kp, D, 0, npad, vtp, got, D, B=2 * B, heads=heads, Nq=P, Nk=P,
                                                 scale=0.125, o_group=B, o_group_rows=xg.rows_pad, eps=1e-6, stats_group_stride=P * (D // 32) * 2,
                                                 vec_group_stride=D)
    report("qproj", "cross-attention, 2 sides x 12 heads x 196", n, wbytes, time_chain(issue, n, a.reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=544.0, help="MB of distinct weight copies per chain (> 512: twice the MALL)")
    ap.add_argument("--reps", type=int, default=5, help="timed replays of a chain")
    ap.add_argument("--only", default="gemm,conv,wide,qproj")
    ap.add_argument("--tiles", default="", help="gemm / conv chains: only these tile ids (comma separated)")
    a = ap.parse_args()
    a.tiles = {int(t) for t in a.tiles.split(",") if t}
    assert torch.cuda.is_available(), "needs an MI355X"
    print("cold-weight chains, %.0f MB of weight copies each, %d timed replays; us per launch, mode 0 (default) vs mode 2 (stream)" % (a.mb, a.reps))
    for fam in a.only.split(","):
        a.family = fam
        {"gemm": gemm_rows, "conv": gemm_rows, "wide": wide, "qproj": qproj}[fam](a)


if __name__ == "__main__":
    main()
