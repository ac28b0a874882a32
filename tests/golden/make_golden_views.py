#!/usr/bin/env python
"""Generate tests/golden/views_rgbd.npz, views_sampling.json and views_eval_align.npz from the UNMODIFIED reference.

    python tests/golden/make_golden_views.py --reference <checkout of the reference>

views_rgbd.npz: the reference's own `BaseStereoViewDataset.__getitem__` on a tiny in-memory subclass whose `_get_views` sanitises
seeded raw depth maps the way the data-set classes do (spann3r/datasets/seven_scenes.py:123-126, with the constants as parameters;
non-finite values become 0) and calls `_crop_resize_if_necessary`.  That covers both crops, the resize, the intrinsics,
`depthmap_to_absolute_camera_coordinates`, the mask and `transpose_to_landscape`.  cv2 and torchvision are not installed: both are
stubbed in sys.modules before the reference is imported.  `cv2.resize` is the numpy statement of OpenCV's INTER_NEAREST rule for a
given dsize (include/spann3r_hip.h, "RGB-D views"; parity with cv2 itself is unpinned), and the data set's `transform` is a numpy
stand-in for ImgNorm.  Keys per case <c>: <c>_raw<i> / _K<i> (inputs of view i), <c>_rgb_seed (the image of view i is tests/views_ref.py seeded_image(H, W, seed)), <c>_pose, <c>_cfg (JSON: resolution, seed,
aug_crop, the sanitising parameters) and the outputs <c>_img, _depthmap, _pts3d, _valid_mask, _camera_intrinsics, _camera_pose,
_true_shape, stacked over the views, plus <c>_xcam: the camera-frame points the reference rotated, and <c>_plan: per view crop0 (4),
resize (2), crop1 (4) as the reference's own calls received them.

The generator ASSERTS that in at least two cases the depth map tells the OpenCV rule from floor(x * src / dst) -- i.e. the two rules
pick different source pixels inside the final crop and those carry different depths -- and that the reference's own float32 `pts3d`
meets the bound the device output is held to: |err_i| <= 4 * 2^-24 * (sum_k |R_ik| |X_k| + |t_i|) against the float64 product.

views_sampling.json: `sample_frames` / `sample_frame_idx` of spann3r/datasets/base_many_view_dataset.py for seeded tuples, with the
number of sample_frames calls each took and the generator's next draw (so a restatement that consumes other draws is caught).  The
recursion of sample_frames:33-34 cannot be reached with a threshold >= 1: every pick leaves room for the remaining frames, so the
list of candidates is never empty (with a threshold of 0 it recurses without end); `calls` is 1 in every row.

views_eval_align.npz: for two seeded sequences (tests/views_ref.py eval_align_case: 4 frames of 24 x 32, B = 1) the reference's
Regr3D_t_ScaleShiftInv(L21, norm_mode=False, gt_scale=True).get_all_pts3d_t -- s<seed>_gt_pts, _pred_l, _pred_r, _monitoring -- and
the lines eval.py:138-168 applied to it, s<seed>_pts_all / _pts_gt_all (the masked clouds of eval.py:189-191 are these stacks under
the case's masks, in order).  `meta` (JSON) holds per sequence the digest of the seeded inputs and D = max |float32 chain - float64
chain| / max |ground-truth coordinate| over the valid pixels: the scale of the tolerance the device output is held to (4 D)."""
import argparse
import json
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
from views_ref import eval_align_batch, eval_align_case, eval_align_digest, seeded_image  # noqa: E402


def nearest_index(dst, src):
    ifx = 1.0 / (float(dst) / float(src))
    return np.minimum(np.floor(np.arange(dst) * ifx).astype(int), src - 1)


def other_index(dst, src):
    return (np.arange(dst) * src / dst).astype(int).clip(0, src - 1)


RESIZE_RULE = [nearest_index]


def stub_modules():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST, cv2.IMREAD_UNCHANGED, cv2.IMREAD_COLOR = 0, -1, 1

    def resize(a, dsize, fx=None, fy=None, interpolation=None):
        w, h = int(dsize[0]), int(dsize[1])
        rule = RESIZE_RULE[0]
        return a[rule(h, a.shape[0])][:, rule(w, a.shape[1])]
    cv2.resize = resize
    tv, tvf = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    for n in ("Compose", "ToTensor", "Normalize", "ColorJitter"):
        setattr(tvf, n, lambda *a, **k: None)
    tv.transforms = tvf
    sys.modules["cv2"], sys.modules["torchvision"], sys.modules["torchvision.transforms"] = cv2, tv, tvf


def img_norm(img):
    a = np.asarray(img).astype(np.float32)
    return ((a / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1)


def sanitise(raw, cfg):
    d = raw.copy()
    if cfg["raw_invalid"] is not None:
        d[d == cfg["raw_invalid"]] = 0
    d = d.astype(np.float32) / np.float32(cfg["depth_div"])
    d[~np.isfinite(d)] = 0
    d[d > np.float32(cfg["max_depth"])] = 0
    d[d < np.float32(cfg["min_depth"])] = 0
    return d


def pose(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = q.astype(np.float32), rng.uniform(-2, 2, 3).astype(np.float32)
    return T


def cases():
    """name -> (cfg, [(H, W, (fx, fy, cx, cy))], depth kind)"""
    base = dict(resolution=(32, 24), seed=7, aug_crop=0, depth_div=1.0, raw_invalid=None, min_depth=0.0, max_depth=float("inf"))
    c = {}
    # sizes chosen so that a crop -> resize pair is one where OpenCV's rule and floor(x * src / dst) pick different pixels:
    # (60, 50) -> (32, 26), (76, 66) -> (32, 27), (66, 58) -> (32, 28), (72, 60) -> (32, 26), (66, 76) -> (27, 32), (56, 54) -> (32, 30)
    c["landscape"] = (dict(base), [(50, 60, (60.0, 61.0, 30.0, 25.0))] * 3, "metres")
    c["offcentre"] = (dict(base, seed=8), [(70, 84, (70.0, 70.0, 46.3, 32.6)), (64, 76, (70.0, 71.0, 32.7, 35.4)),
                                           (66, 80, (64.0, 64.0, 44.3, 30.4))], "metres")
    c["portrait"] = (dict(base, seed=9), [(80, 70, (58.0, 58.5, 33.0, 42.0)), (76, 62, (58.0, 58.5, 30.4, 36.2)),
                                          (80, 70, (58.0, 58.5, 37.0, 38.0))], "metres")
    for s in (11, 12):
        c["square_s%d" % s] = (dict(base, seed=s), [(56, 58, (55.0, 55.0, 28.0, 27.0)), (50, 48, (55.0, 55.0, 23.0, 25.0)),
                                                    (50, 46, (55.0, 55.0, 22.4, 23.6))], "metres")
    c["augcrop"] = (dict(base, seed=15, aug_crop=8), [(48, 64, (60.0, 60.0, 32.0, 24.0)), (48, 64, (60.0, 60.0, 30.0, 25.0)),
                                                      (52, 70, (60.0, 60.0, 35.0, 26.0)), (48, 64, (60.0, 60.0, 33.0, 23.0))], "metres")
    c["uint16"] = (dict(base, seed=16, depth_div=1000.0, raw_invalid=65535, min_depth=1e-3, max_depth=10.0),
                   [(62, 80, (75.0, 75.0, 36.0, 30.0)), (60, 80, (75.0, 75.0, 39.0, 31.0)), (58, 78, (75.0, 75.0, 39.0, 29.0))], "uint16")
    c["nonfinite"] = (dict(base, seed=17), [(54, 74, (66.0, 66.0, 37.0, 27.0)), (54, 74, (66.0, 66.0, 36.0, 28.0)),
                                            (54, 74, (66.0, 66.0, 38.0, 26.0))], "nonfinite")
    return c


def raw_depth(kind, h, w, rng):
    if kind == "uint16":
        d = rng.integers(300, 9000, (h, w)).astype(np.uint16)
        d[rng.random((h, w)) < 0.05] = 0
        d[rng.random((h, w)) < 0.05] = 65535
        d[rng.random((h, w)) < 0.05] = 12000            # beyond max_depth
        d[h // 2, w // 2], d[h // 2 + 1, w // 2], d[h // 2, w // 2 + 1] = 0, 65535, 10001
        return d
    d = (rng.integers(512, 4096, (h, w)) / 1024.0).astype(np.float32)          # multiples of 2^-10 m: the file stays small
    if kind == "nonfinite":
        d[rng.random((h, w)) < 0.04] = np.inf
        d[rng.random((h, w)) < 0.04] = np.nan
        d[rng.random((h, w)) < 0.02] = -np.inf
        d[h // 2, w // 2], d[h // 2 + 1, w // 2] = np.inf, np.nan
    return d


def make_rgbd(out_path):
    import dust3r.datasets.utils.cropping as cropping
    import dust3r.utils.geometry as geometry
    from dust3r.datasets.base.base_stereo_view_dataset import BaseStereoViewDataset

    rec = {"crops": [], "resize": [], "xcam": []}
    real_crop, real_resize, real_cam = cropping.crop_image_depthmap, cropping.ImageList.resize, geometry.depthmap_to_camera_coordinates

    def crop(image, depthmap, K, bbox):
        rec["crops"].append(tuple(int(v) for v in bbox))
        return real_crop(image, depthmap, K, bbox)

    def resize(self, size, **kw):
        rec["resize"].append(tuple(int(v) for v in size))
        return real_resize(self, size, **kw)

    def cam(*a, **k):
        X, m = real_cam(*a, **k)
        rec["xcam"].append(X)
        return X, m
    cropping.crop_image_depthmap, cropping.ImageList.resize, geometry.depthmap_to_camera_coordinates = crop, resize, cam

    class Memory(BaseStereoViewDataset):
        def __init__(self, frames, cfg, **kw):
            super().__init__(**kw)
            self.frames, self.cfg, self.scenes = frames, cfg, [0]

        def _get_views(self, idx, resolution, rng):
            views = []
            for i, (rgb, raw, K, T) in enumerate(self.frames):
                img, depth, K2 = self._crop_resize_if_necessary(rgb, sanitise(raw, self.cfg), K, resolution, rng=rng, info=str(i))
                views.append(dict(img=img, depthmap=depth, camera_pose=T, camera_intrinsics=K2, dataset="rgbd", label=str(i), instance=str(i)))
            return views

    def run(frames, cfg):
        for v in rec.values():
            del v[:]
        ds = Memory(frames, cfg, split="train", resolution=tuple(cfg["resolution"]), transform=img_norm, aug_crop=cfg["aug_crop"],
                    seed=cfg["seed"])
        return ds[0]

    out, names, told_apart, worst_units = {}, [], 0, 0.0
    for name, (cfg, specs, kind) in cases().items():
        rng = np.random.default_rng(1000 + cfg["seed"])
        frames, seeds = [], []
        for (h, w, (fx, fy, cx, cy)) in specs:
            K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)
            seeds.append(100 * cfg["seed"] + len(frames))
            frames.append((seeded_image(h, w, seeds[-1]), raw_depth(kind, h, w, rng), K, pose(rng)))
        RESIZE_RULE[0] = other_index
        alt = np.stack([v["depthmap"] for v in run(frames, cfg)])
        RESIZE_RULE[0] = nearest_index
        views = run(frames, cfg)
        n = len(views)
        plan = np.int32([list(rec["crops"][2 * i]) + list(rec["resize"][i]) + list(rec["crops"][2 * i + 1]) for i in range(n)])
        xcam = []
        for i, v in enumerate(views):
            h, w = v["true_shape"]
            X = rec["xcam"][i]
            xcam.append(X.swapaxes(0, 1) if w < h else X)
            # the bound of the world check, for the reference's own float32 output
            R, t = v["camera_pose"][:3, :3].astype(np.float64), v["camera_pose"][:3, 3].astype(np.float64)
            X64 = xcam[-1].astype(np.float64)
            exact = X64 @ R.T + t
            unit = 2.0 ** -24 * (np.abs(X64) @ np.abs(R).T + np.abs(t))
            worst_units = max(worst_units, float((np.abs(v["pts3d"].astype(np.float64) - exact) / unit).max()))
            assert v["pts3d"].dtype == np.float32 and X.dtype == np.float32
        depth = np.stack([v["depthmap"] for v in views])
        differs = int((alt != depth).sum())
        told_apart += differs > 0
        for i, (rgb, raw, K, T) in enumerate(frames):
            out["%s_raw%d" % (name, i)], out["%s_K%d" % (name, i)] = raw, K
        out[name + "_rgb_seed"] = np.int32(seeds)
        out[name + "_pose"] = np.stack([f[3] for f in frames])
        out[name + "_cfg"] = np.array(json.dumps(cfg))
        out[name + "_plan"], out[name + "_xcam"] = plan, np.stack(xcam)
        for k in ("img", "depthmap", "pts3d", "valid_mask", "camera_intrinsics", "camera_pose", "true_shape"):
            out["%s_%s" % (name, k)] = np.stack([np.asarray(v[k]) for v in views])
        names.append(name)
        print("%-12s views %d  true_shape %s  pixels where the two index rules give different depths: %d  valid %.2f" % (
            name, n, [tuple(int(x) for x in v["true_shape"]) for v in views], differs, out[name + "_valid_mask"].mean()))
    assert told_apart >= 2, "the fixture cannot tell the two nearest-neighbour rules apart"
    assert worst_units <= 4.0, worst_units
    shapes = {n: {tuple(s) for s in out[n + "_true_shape"].tolist()} for n in names if n.startswith("square")}
    assert any(len(s) == 2 or (24, 32) in s for s in shapes.values()) and any((32, 24) in s for s in shapes.values()), shapes
    out["names"] = np.array(names)
    out["meta"] = np.array(json.dumps(dict(worst_world_error_units_of_2p24=worst_units)))
    np.savez_compressed(out_path, **out)
    print("%s: %d cases, %.0f KB, reference's own pts3d error %.2f units (bound 4)" % (os.path.basename(out_path), len(names),
                                                                                      os.path.getsize(out_path) / 1024, worst_units))


def make_sampling(out_path):
    from spann3r.datasets.base_many_view_dataset import BaseManyViewDataset
    tuples = []
    for seed in range(6):
        tuples += [(60, 5, 3, 9, 1.0, seed), (40, 5, 2, 12, 0.5, seed), (12, 5, 1, 3, 1.0, seed), (9, 4, 1, 2, 0.0, seed),
                   (200, 8, 5, 30, 0.3, seed)]
    rows, recursions, calls = [], 0, [0]

    class Counted(BaseManyViewDataset):             # sees the recursive self.sample_frames calls too
        def sample_frames(self, img_idxs, rng):
            calls[0] += 1
            return super().sample_frames(img_idxs, rng)
    for (length, num_frames, lo, hi, ratio, seed) in tuples:
        ds = Counted.__new__(Counted)
        ds.num_frames, ds.min_thresh, ds.max_thresh, ds.train_ratio, ds.kf_every = num_frames, lo, hi, ratio, 3
        calls[0] = 0
        names = ["%06d" % i for i in range(length)]
        rng = np.random.default_rng(seed)
        picked = ds.sample_frame_idx(names, rng, full_video=False)
        after = int(rng.integers(1 << 30))
        recursions += calls[0] > 1
        full = ds.sample_frame_idx(names, np.random.default_rng(seed), full_video=True)
        rows.append(dict(length=length, num_frames=num_frames, min_thresh=lo, max_thresh=hi, train_ratio=ratio, seed=seed,
                         picked=picked, calls=calls[0], next_draw=after, kf_every=3, full_video=full))
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=0)
        f.write("\n")
    print("%s: %d tuples, %d of them recursed" % (os.path.basename(out_path), len(rows), recursions))


def make_eval_align(out_path):
    """the reference's own Regr3D_t_ScaleShiftInv(L21, norm_mode=False, gt_scale=True).get_all_pts3d_t on seeded sequences, and the
    lines eval.py:138-168 applied to it (restated here with the reference's geotrf: eval.py itself imports open3d), in float32 as the
    reference runs it and in float64 for the error scale D."""
    import torch
    from dust3r.losses import L21
    from dust3r.utils.geometry import geotrf
    from spann3r.loss import Regr3D_t_ScaleShiftInv

    def chain(case, dtype):
        views, preds, preds_all = eval_align_batch(case, lambda a: torch.from_numpy(a.copy()), dtype)      # (the reference scales in place)
        crit = Regr3D_t_ScaleShiftInv(L21, norm_mode=False, gt_scale=True)
        with torch.no_grad():
            gt_pts, pred_pts, gt_factor, pr_factor, masks, monitoring = crit.get_all_pts3d_t(views, preds_all)
        assert gt_factor is None and pr_factor is None
        res = dict(gt_pts=torch.cat(gt_pts).numpy().copy(), pred_l=torch.cat(pred_pts[0]).numpy().copy(),
                   pred_r=torch.cat(pred_pts[1]).numpy().copy(), monitoring=np.array([float(monitoring[k]) for k in MONITORING]))
        gt_shift_z = monitoring["gt_shift_z"]
        in_camera1, pts_all, pts_gt_all = None, [], []
        for j, view in enumerate(views):                                   # eval.py:138-162
            if in_camera1 is None:
                in_camera1 = view["camera_pose"][0].cpu()
            pts = pred_pts[0][j].cpu().numpy()[0] if j < len(pred_pts[0]) else pred_pts[1][-1].cpu().numpy()[0]
            pts_gt = gt_pts[j].detach().cpu().numpy()[0]
            pts[..., -1] += gt_shift_z.cpu().numpy().item()
            pts = geotrf(in_camera1, pts)
            pts_gt[..., -1] += gt_shift_z.cpu().numpy().item()
            pts_gt = geotrf(in_camera1, pts_gt)
            pts_all.append(np.asarray(pts)[None])
            pts_gt_all.append(np.asarray(pts_gt)[None])
        res["pts_all"], res["pts_gt_all"] = np.concatenate(pts_all), np.concatenate(pts_gt_all)
        return res

    out, meta = {}, {}
    for seed in (21, 22):
        case = eval_align_case(seed)
        assert not np.allclose(case["poses"][0], np.eye(4)) and 0.6 < case["masks"].mean() < 0.8
        r32, r64 = chain(case, None), chain(case, np.float64)
        assert r32["pts_all"].dtype == np.float32 and r64["pts_all"].dtype == np.float64
        m = case["masks"]
        scale = float(np.abs(case["world"][m]).max())
        D = max(float(np.abs(r32[k][m] - r64[k][m]).max()) for k in ("pts_all", "pts_gt_all")) / scale
        tag = "s%d_" % seed
        for k, v in r32.items():
            out[tag + k] = v
        meta[tag[:-1]] = dict(seed=seed, D=D, max_abs_gt=scale, digest=eval_align_digest(case), monitoring=MONITORING,
                              monitoring_float64=r64["monitoring"].tolist())
        print("eval align seed %d: D = %.3g, valid %.2f, monitoring %s" % (seed, D, m.mean(), r32["monitoring"]))
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(out_path, **out)
    print("%s: %.0f KB" % (os.path.basename(out_path), os.path.getsize(out_path) / 1024))


MONITORING = ["gt_shift_z", "pred_shift_z", "gt_scale", "pred_scale"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("SPANN3R_REFERENCE"), required="SPANN3R_REFERENCE" not in os.environ)
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    stub_modules()
    make_rgbd(os.path.join(HERE, "views_rgbd.npz"))
    make_sampling(os.path.join(HERE, "views_sampling.json"))
    make_eval_align(os.path.join(HERE, "views_eval_align.npz"))


if __name__ == "__main__":
    main()
