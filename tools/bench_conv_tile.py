"""Time sp3_conv3x3_tile with the 8 x 8 and the 8 x 16 pixel tile on the DPT-head shapes (hipGraph, HIP events):
python tools/bench_conv_tile.py           ->  one line per shape, us per launch and TFLOP/s for the three tiles; 20 launches on ONE weight
                                              buffer per replay: the weights are L2-warm from the second launch on
python tools/bench_conv_tile.py --cold    ->  the same with cold weights, as in the model (one step streams ~650 MB of weights against
                                              256 MB of Infinity Cache): every launch of a replay reads its own copy out of a pool of
                                              packed copies larger than 512 MB, so a copy is long evicted when its turn comes again.  The
                                              input map stays warm (in the model the previous launch has just written it).  Prints the
                                              median of the replays and their spread (min .. max) per tile.
--shapes B,H,W,Cin,Cout ...  restricts the sweep."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spann3r_amd import ops  # noqa: E402

SHAPES = [  # B, H, W, Cin, Cout (8x16n32 = the wide tile with 32 output channels per workgroup)          (config 2: 224 input -> 56 / 112 / 224 maps; config 3: 512 input -> 128 / 256 / 512)
    (1, 56, 56, 256, 256), (1, 48, 64, 256, 256), (2, 56, 56, 256, 256), (9, 56, 56, 256, 256), (1, 112, 112, 256, 256), (1, 112, 112, 256, 128), (9, 112, 112, 256, 256),
    (1, 224, 224, 128, 128), (9, 224, 224, 128, 128), (1, 128, 128, 256, 256), (1, 256, 256, 256, 256), (1, 256, 256, 256, 128),
    (1, 512, 512, 128, 128)]
TILES = ("8x8", "8x16", "8x16n32")
POOL_BYTES = 512 << 20


def weight_pool(wp, cold):
    """the packed weight itself (warm), or views of > 512 MB worth of copies of it in one allocation (cold)"""
    if not cold:
        return [wp]
    n = POOL_BYTES // (wp.data.numel() * wp.data.element_size()) + 1
    pool = wp.data.unsqueeze(0).repeat(n, *([1] * wp.data.dim()))
    return [ops.PackedWeight.wrap(pool[i], wp.N, wp.K) for i in range(n)]


def time_tile(run, pool, launches, replays):
    """us per launch of every replay of a graph of `launches` launches that walks the pool round robin"""
    run(pool[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(launches):
            run(pool[i % len(pool)])
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for _ in range(replays):
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1000 / launches)
    return sorted(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cold", action="store_true")
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=None)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in args.shapes] if args.shapes else SHAPES
    dev = "cuda"
    if args.cold:
        print("cold weights: pool of packed copies > %d MB, one launch per copy and replay; us = median (min .. max) of %d replays" % (POOL_BYTES >> 20, args.replays))
        print("%-28s %26s %26s %26s  %s" % ("B,H,W,Cin,Cout", "8x8 us", "8x16 us", "8x16n32 us", "wide workgroups"))
    else:
        print("%-28s %10s %10s %10s %10s %10s %10s  %s" % ("B,H,W,Cin,Cout", "8x8 us", "TFLOP/s", "8x16 us", "TFLOP/s", "8x16n32 us", "TFLOP/s", "wide workgroups"))
    for B, H, W, Cin, Cout in shapes:
        x = torch.randn(B, H, W, Cin, device=dev).to(torch.bfloat16)
        wp = ops.PackedWeight((torch.randn(Cout, 9 * Cin, device=dev) * 0.02).to(torch.bfloat16))
        pool = weight_pool(wp, args.cold)
        bias = torch.randn(Cout, device=dev)
        out = torch.empty(B, H, W, Cout, device=dev, dtype=torch.bfloat16)
        res = {}
        for px in TILES:
            run = lambda w: ops.conv3x3(x, w, out, B=B, H=H, W_=W, Cin=Cin, Cout=Cout, bias=bias, relu_in=True, tile_px=px)
            res[px] = time_tile(run, pool, len(pool) if args.cold else 20, args.replays)
        fl = 2.0 * B * H * W * Cout * 9 * Cin
        wgs = ((W + 15) // 16) * ((H + 7) // 8) * B * (Cout // 64)
        name = "%d,%d,%d,%d,%d" % (B, H, W, Cin, Cout)
        if args.cold:
            cell = lambda u: "%8.2f (%7.2f ..%7.2f)" % (u[len(u) // 2], u[0], u[-1])
            print("%-28s %26s %26s %26s  %d" % (name, cell(res["8x8"]), cell(res["8x16"]), cell(res["8x16n32"]), wgs), flush=True)
        else:
            best = {px: res[px][0] for px in TILES}
            print("%-28s %10.2f %10.1f %10.2f %10.1f %10.2f %10.1f  %d" % (name, best["8x8"], fl / best["8x8"] / 1e6, best["8x16"], fl / best["8x16"] / 1e6,
                                                                         best["8x16n32"], fl / best["8x16n32"] / 1e6, wgs), flush=True)
        del pool


if __name__ == "__main__":
    main()
