#!/usr/bin/env python
"""Timing record of the streaming session (spann3r_amd/stream.py) next to Spann3R.forward at the same commit: 50 frames of 224x224,
B = 1, full model, seeded weights, in bf16 and f16x3, warm graphs.
 (a) push latency with a device synchronise after every push (host clock: what a camera loop sees per frame),
 (b) frames/s of unsynchronised pushes (one synchronise at the end of the sequence),
 (c) forward on the same frames: the default schedule (whole-sequence encoder, deferred view-2 head) and batch_encode = False,
 (d) the number of hipGraphs the session holds after 50 and after 100 frames.
Nothing is asserted.  Without --precision the tool is a driver that touches no GPU itself: every precision is measured by a child
process of its own under a time limit, the first child that fails ends the run, and the parts are joined into --out
(profiles/stream.txt is the committed record)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(args):
    import numpy as np
    import torch
    from spann3r_amd import Spann3R, FULL, TINY
    from spann3r_amd.weights import synth_state_dict, synth_frames
    cfg = TINY if args.tiny else FULL
    dev = "cuda"
    m = Spann3R(dus3r_name=None, cfg=cfg, init_weights=False).to(dev)
    m.load_state_dict(synth_state_dict(0, cfg))
    m.eval().set_precision(args.precision)
    n, hw = args.frames, args.size
    frames = [{"img": f["img"].to(dev)} for f in synth_frames(2 * n, hw, hw)]
    seq = frames[:n]
    rows = ["--- %s, %d frames of %dx%d, B = 1, %s" % (args.precision, n, hw, hw, "TINY" if args.tiny else "full model")]

    def sync():
        torch.cuda.synchronize()

    def pct(x, q):
        return float(np.percentile(np.asarray(x), q))

    s = m.stream()
    for _ in range(2):                                    # eager pass (workspaces), then the pass that captures
        s.reset()
        for f in seq:
            s.push(f)
    sync()
    # (a) one synchronise per push
    first, lat, replayed = [], [], 0
    t_all = 0.0
    for _ in range(args.repeat):
        s.reset()
        sync()
        r0 = s.replays
        t_seq = time.perf_counter()
        for t, f in enumerate(seq):
            t0 = time.perf_counter()
            s.push(f)
            sync()
            dt = (time.perf_counter() - t0) * 1e3
            if t == 1:
                first.append(dt)
            elif t > 1:
                lat.append(dt)
        t_all += time.perf_counter() - t_seq
        replayed = s.replays - r0
    rows.append("(a) push + synchronise, pushes 2..%d of %d passes: median %.3f ms, p95 %.3f ms, max %.3f ms; push 1 (the first step, eager, "
                "encodes two frames) median %.3f ms; %.1f frames/s overall; %d of %d pushes of a pass replayed a graph"
                % (n - 1, args.repeat, pct(lat, 50), pct(lat, 95), max(lat), pct(first, 50), args.repeat * n / t_all, replayed, n - 1))
    # (b) no synchronise inside the sequence
    fps = []
    for _ in range(args.repeat):
        s.reset()
        sync()
        t0 = time.perf_counter()
        for f in seq:
            s.push(f)
        sync()
        fps.append(n / (time.perf_counter() - t0))
    rows.append("(b) unsynchronised pushes (one synchronise per sequence): median %.1f frames/s [%.1f .. %.1f] x%d"
                % (pct(fps, 50), min(fps), max(fps), args.repeat))
    stream_fps = pct(fps, 50)
    # (d) graphs held
    g50 = len(s._run.graphs)
    s.reset()
    for f in frames:
        s.push(f)
    sync()
    g100 = len(s._run.graphs)
    eager_keys = s._run.graphs.length_keys_eager
    s.close()
    # (c) forward on the same frames
    for name, be in (("default schedule", True), ("batch_encode = False", False)):
        m.batch_encode = be
        for _ in range(3):
            m(seq)
        sync()
        ff = []
        for _ in range(args.repeat):
            sync()
            t0 = time.perf_counter()
            m(seq)
            sync()
            ff.append(n / (time.perf_counter() - t0))
        rows.append("(c) forward, %-22s median %.1f frames/s [%.1f .. %.1f] x%d; unsynchronised stream / forward = %.3f"
                    % (name + ":", pct(ff, 50), min(ff), max(ff), args.repeat, stream_fps / pct(ff, 50)))
    m.batch_encode = True
    rows.append("(d) hipGraphs the session holds: %d after %d frames, %d after %d frames%s"
                % (g50, n, g100, 2 * n, " (per-length step keys launch eagerly)" if eager_keys else ""))
    text = "\n".join(rows)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--precision", default=None, help="measure this precision in this process (what the driver starts)")
    ap.add_argument("--precisions", default="bf16,f16x3")
    ap.add_argument("--limit", type=int, default=300, help="seconds each child may take")
    args = ap.parse_args()
    if args.precision:
        return measure(args)
    parts = []
    for p in args.precisions.split(","):
        part = (args.out or os.path.join(ROOT, "stream")) + "." + p + ".part"
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--precision", p, "--out", part,
               "--frames", str(args.frames), "--size", str(args.size), "--repeat", str(args.repeat)] + (["--tiny"] if args.tiny else [])
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit("bench_stream: the %s run ended with status %d; nothing more is started" % (p, rc))
        with open(part) as f:
            parts.append(f.read())
        os.remove(part)
    if args.out:
        with open(args.out, "w") as f:
            f.write("Streaming session against forward (tools/bench_stream.py); host clock around work that ends in a device synchronise\n")
            f.write("".join(parts))


if __name__ == "__main__":
    main()
