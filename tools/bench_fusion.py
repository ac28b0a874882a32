#!/usr/bin/env python
"""Timing record of the TSDF fusion (spann3r_amd/fusion.py, csrc/fusion.hip): 50 frames of 224x224 -- a sphere on a plane seen from
a ring of cameras, analytic depth -- into a 256^3 volume with colours.  Rows: one sp3_tsdf_integrate call for all frames, 50
one-frame calls, sp3_tsdf_extract and extract_mesh (device events around the calls, warmed up, repeated; descriptor tables and
buffers prepared outside), the effective bandwidth of the one-call integration as (volume bytes read + written once) / time next to
the HBM peak, and the numpy restatement of tests/fusion_ref.py on this machine's CPU (fp32, numpy's own single thread) as the
baseline, on a part of the work and scaled, since the whole would take minutes.  Nothing is asserted except that device and numpy
agree on that part.  Writes the table to --out (profiles/fusion.txt is the committed record)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import fusion_ref as FR
from spann3r_amd import fusion as F
from tools.bench_render import timed

HBM_PEAK_TBS, HBM_MEASURED_TBS = 8.0, 6.3          # spec and float4-copy figures of the MI355X


def ring_frames(t, h, w):
    rng = np.random.default_rng(0)
    centre, radius = (0.0, 0.0, 0.45), 0.45
    out = []
    for i in range(t):
        ang = 2 * np.pi * i / t
        P = FR.look_at((2.0 * np.cos(ang), 2.0 * np.sin(ang), 1.3 + 0.2 * np.sin(3 * ang)), (0.0, 0.0, 0.3))
        fu = fv = 0.9 * w
        cu, cv = (w - 1) / 2, (h - 1) / 2
        d, _, _ = FR.analytic_depth(P, fu, fv, cu, cv, h, w, centre, radius)
        d = np.where(d > 6.0, 0.0, d)
        byte = rng.integers(0, 256, (h, w, 3))
        out.append(dict(depth=d.astype(np.float32), pts=None, valid=(d > 0).astype(np.uint8), pixel_weight=None,
                        images=(byte / 255.0).astype(np.float32), rgba=(byte[..., 0] | byte[..., 1] << 8 | byte[..., 2] << 16 | 255 << 24).astype(np.uint32),
                        K=np.array([[fu, 0, cu], [0, fv, cv], [0, 0, 1]]), cam2world=P, fu=fu, fv=fv, cu=cu, cv=cv))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--dims", type=int, default=256)
    ap.add_argument("--cpu_frames", type=int, default=2, help="frames of the numpy integration baseline (scaled to --frames)")
    ap.add_argument("--cpu_dims", type=int, default=96, help="edge of the sub-volume of the numpy extraction baseline (scaled by voxels)")
    args = ap.parse_args()
    t, hw, n1 = args.frames, args.size, args.dims
    rows = ["TSDF fusion (libspann3r_hip.so), device %s" % torch.cuda.get_device_name(0),
            "times: median [min .. max] x repeats; device events around whole calls (launch overhead included) unless a row says host clock",
            "--- %d frames of %dx%d into %d^3 voxels (%.1f M), colours on, trunc 3 voxels" % (t, hw, hw, n1, n1 ** 3 / 1e6)]

    def row(name, tm, extra=""):
        med, lo, hi, reps = tm
        rows.append("%-72s %10.3f ms  [%9.3f .. %9.3f] x%-3d %s" % (name, med, lo, hi, reps, extra))

    frames = ring_frames(t, hw, hw)
    voxel = 2.4 / n1
    vol = F.TSDFVolume((-1.2, -1.2, -0.3), voxel, (n1, n1, n1))
    dev = [dict(depth=torch.from_numpy(f["depth"]).cuda(), valid=torch.from_numpy(f["valid"]).cuda(), images=torch.from_numpy(f["images"]).cuda())
           for f in frames]
    Ks, Ps = [f["K"] for f in frames], [f["cam2world"] for f in frames]
    whole = vol.frame_table([d["depth"] for d in dev], True, Ks, Ps, [d["valid"] for d in dev], None, [d["images"] for d in dev])
    singles = [vol.frame_table([dev[i]["depth"]], True, Ks[i:i + 1], Ps[i:i + 1], [dev[i]["valid"]], None, [dev[i]["images"]]) for i in range(t)]
    for f, e in zip(frames, whole[0]):
        f["w2c"] = np.array(list(e.w2c), np.float32)                            # the matrices the kernel is given

    def one_call():
        vol.integrate_table(whole)

    def many_calls():
        for s in singles:
            vol.integrate_table(s)

    nbytes = 2 * vol.tsdf.numel() * 4 * 5                                   # tsdf + weight + rgb, read once and written once
    vol.reset()
    tm = timed(one_call)
    row("sp3_tsdf_integrate, %d frames in ONE call" % t, tm,
        "%.2f TB/s effective = %.1f MB once in, once out (HBM: %.1f TB/s spec, %.1f measured copy); %.3e voxel-frames/s"
        % (nbytes / (tm[0] * 1e-3) / 1e12, nbytes / 1e6, HBM_PEAK_TBS, HBM_MEASURED_TBS, vol.tsdf.numel() * t / (tm[0] * 1e-3)))
    vol.reset()
    tm2 = timed(many_calls)
    row("sp3_tsdf_integrate, %d one-frame calls" % t, tm2, "%.2f x the one call; volume traffic %.1f GB" % (tm2[0] / tm[0], nbytes * t / 1e9))
    vol.reset()
    one_call()
    torch.cuda.synchronize()
    state = (vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.rgb.cpu().numpy())
    vol.reset()
    many_calls()
    same = all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(state, (vol.tsdf, vol.weight, vol.rgb)))
    rows.append("  one call and %d calls give the same bits: %s; voxels observed: %.1f %%" % (t, same, 100 * float((state[1] > 0).mean())))

    counts = vol.extract_raw()[3].cpu().tolist()
    cap_v, cap_f = counts

    def extract():
        vol.extract_raw(1.0, cap_v, cap_f)

    tm3 = timed(extract)
    row("sp3_tsdf_extract (6 launches; buffers from torch's cache): V %d, F %d" % (cap_v, cap_f), tm3, "%.3e voxels/s" % (vol.tsdf.numel() / (tm3[0] * 1e-3)))
    tm4 = timed(lambda: vol.extract_mesh())
    row("extract_mesh: extract, one host read of the counts, compact_vertices", tm4)
    mesh = vol.extract_mesh()
    rows.append("  after compaction: %d vertices, %d faces (app.py's sheets of the same frames: %d faces)"
                % (mesh["vertices"].shape[0], mesh["faces"].shape[0], 2 * t * (hw - 1) * (hw - 1)))

    return rows, args, vol, frames, state, (tm, tm3)


def cpu_part(rows, args, vol, frames, state, tms):
    t, n1 = args.frames, args.dims
    tm, tm3 = tms
    o, vx, tr = vol.origin, np.float32(vol.voxel_size), np.float32(vol.trunc)
    k = args.cpu_frames
    t0 = time.perf_counter()
    ref = FR.integrate_ref(*FR.empty_volume(vol.dims), frames[:k], o, vx, tr, np.float32)
    dt = time.perf_counter() - t0
    v2 = F.TSDFVolume(vol.origin, vol.voxel_size, vol.dims, trunc=vol.trunc)
    v2.integrate(depth=[torch.from_numpy(f["depth"]).cuda() for f in frames[:k]], intrinsics=[f["K"] for f in frames[:k]],
                 cam2world=[f["cam2world"] for f in frames[:k]], valid=[torch.from_numpy(f["valid"]).cuda() for f in frames[:k]],
                 images=[torch.from_numpy(f["images"]).cuda() for f in frames[:k]])
    same = all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(ref, (v2.tsdf, v2.weight, v2.rgb)))
    rows.append("numpy path (tests/fusion_ref.py, fp32), host clock, one run, numpy's own single thread:")
    rows.append("  integrate, %d frames: %.1f s -> %.1f s for %d frames = %.0f x the device's %.3f ms; device equals numpy on those frames: %s"
                % (k, dt, dt * t / k, t, dt * t / k * 1e3 / tm[0], tm[0], same))
    c = args.cpu_dims
    lo = (n1 - c) // 2
    sub = tuple(np.ascontiguousarray(a[:c, lo:lo + c, lo:lo + c]) for a in state)      # low z: the plane and the sphere
    so = np.float32([o[0] + np.float32(lo) * vx, o[1] + np.float32(lo) * vx, o[2]])
    t0 = time.perf_counter()
    rv, rc, rf = FR.extract_ref(*sub, so, vx, 1.0, np.float32)
    dt = time.perf_counter() - t0
    v3 = F.TSDFVolume(so, vol.voxel_size, (c, c, c), trunc=vol.trunc)
    for dst, src in zip((v3.tsdf, v3.weight, v3.rgb), sub):
        dst.copy_(torch.from_numpy(src).cuda())
    gv, gc, gf, cnt = v3.extract_raw(1.0, 7 * c ** 3, 12 * c ** 3)
    nv, nf = cnt.cpu().tolist()
    same = (nv, nf) == (len(rv), len(rf)) and np.array_equal(gf[:nf].cpu().numpy(), rf) and np.array_equal(gv[:nv].cpu().numpy(), rv)
    scale = (n1 / c) ** 3
    rows.append("  extract, a %d^3 part (V %d, F %d): %.2f s -> %.1f s scaled by voxels to %d^3 = %.0f x the device's %.3f ms; device equals numpy on that part: %s"
                % (c, len(rv), len(rf), dt, dt * scale, n1, dt * scale * 1e3 / tm3[0], tm3[0], same))
    text = "\n".join(rows)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    cpu_part(*main())
