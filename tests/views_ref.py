"""Numpy restatement of the rules of include/spann3r_hip.h, "RGB-D views" (sp3_view_depth): the nearest-neighbour index rule, the depth
sanitising, the double-then-round unprojection, the fp32 rotation in the header's order, the mask and the landscape transpose.  It is
checked against the reference's own output (tests/golden/views_rgbd.npz) in tests/test_views_cpu.py -- depth, mask and camera-frame
points exactly, world points within the rounding bound below -- and is then the pin of the kernel on further shapes in
tests/test_views_gpu.py."""
import numpy as np


def seeded_image(h, w, seed):
    """the RGB input of a fixture view (the fixture stores the seed, not the bytes)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (np.sin(xx / 7.0) + np.cos(yy / 5.0)) * 60 + 128
    img = base[..., None] + rng.normal(0, 40, (h, w, 3))
    img[h // 3: h // 3 + 2] = 255
    img[:, w // 2: w // 2 + 2] = 0
    return np.clip(img, 0, 255).astype(np.uint8)


def nearest_index(dst, src):
    """OpenCV's INTER_NEAREST for a given dsize: ifx = 1 / (dst / src), sx = min(floor(x * ifx), src - 1), in double"""
    ifx = 1.0 / (float(dst) / float(src))
    return np.minimum(np.floor(np.arange(dst) * ifx).astype(np.int64), src - 1)


def sanitise(raw, depth_div=1.0, raw_invalid=None, min_depth=0.0, max_depth=np.inf):
    d = np.array(raw)
    if raw_invalid is not None:
        d[d == raw_invalid] = 0
    with np.errstate(all="ignore"):
        d = d.astype(np.float32) / np.float32(depth_div)
    d[~np.isfinite(d)] = 0
    d[d > np.float32(max_depth)] = 0
    d[d < np.float32(min_depth)] = 0
    return d


def view_depth_ref(raw, plan, pose, **sanitising):
    """raw [H, W] uint16 / float32; plan: crop0 (l, t, r, b), resize (W2, H2), crop1 (l2, t2, ..), out (w, h), K_crop float32 3x3;
    pose 4x4.  -> depth [oh, ow], xcam [oh, ow, 3], pts [oh, ow, 3], mask [oh, ow]: landscape, as the kernel stores them."""
    l, t, r, b = plan["crop0"]
    W2, H2 = plan["resize"]
    l2, t2 = plan["crop1"][:2]
    w, h = plan["out"]
    sx = nearest_index(W2, r - l)[l2:l2 + w] + l
    sy = nearest_index(H2, b - t)[t2:t2 + h] + t
    z = sanitise(np.asarray(raw)[sy][:, sx], **sanitising)
    K = np.asarray(plan["K_crop"], np.float32)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    z64 = z.astype(np.float64)
    with np.errstate(all="ignore"):
        xc = ((u - np.float64(K[0, 2])) * z64 / np.float64(K[0, 0])).astype(np.float32)
        yc = ((v - np.float64(K[1, 2])) * z64 / np.float64(K[1, 1])).astype(np.float32)
        xcam = np.stack((xc, yc, z), -1)
        P = np.asarray(pose, np.float32)
        pts = np.stack([((P[i, 0] * xc + P[i, 1] * yc) + P[i, 2] * z) + P[i, 3] for i in range(3)], -1)    # fp32, each op rounded
    assert pts.dtype == np.float32
    mask = (z > 0) & np.isfinite(pts).all(-1)
    if h > w:
        z, xcam, pts, mask = z.swapaxes(0, 1), xcam.swapaxes(0, 1), pts.swapaxes(0, 1), mask.swapaxes(0, 1)
    return z, xcam, pts, mask


def world_bound(xcam, pose):
    """(float64 product of the float32 camera-frame points with the pose, the unit 2^-24 (sum_k |R_ik| |X_k| + |t_i|)): the world
    points may err by 4 units -- three products, two sums and the translation round at most four times along any one path"""
    P = np.asarray(pose, np.float64)
    X = np.asarray(xcam, np.float64)
    return X @ P[:3, :3].T + P[:3, 3], 2.0 ** -24 * (np.abs(X) @ np.abs(P[:3, :3]).T + np.abs(P[:3, 3]))


# ------------------------------------------------------------------------------------------------ evaluation alignment
def eval_align_case(seed, n=4, H=24, W=32):
    """Seeded inputs of the alignment fixture (tests/golden/views_eval_align.npz stores their digest and the reference's outputs):
    one sequence, B = 1: ground truth in the world of a non-identity first pose, masks about 70 % valid, predictions = the ground
    truth in camera 0, scaled, z-shifted and perturbed.  numpy arrays: world [n, H, W, 3], masks [n, H, W], poses [n, 4, 4],
    pred_l / pred_r [n - 1, H, W, 3] (left prediction of frames 0..n-2, right prediction of frames 1..n-1), conf_l / conf_r
    [n - 1, H, W], conf [n, H, W] (the per-frame `preds`), img [n, 3, H, W] in [-1, 1]."""
    rng = np.random.default_rng(seed)
    poses = []
    for _ in range(n):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = q, rng.uniform(-1.5, 1.5, 3)
        poses.append(T)
    poses = np.stack(poses)
    z = rng.uniform(1.0, 4.0, (n, H, W))
    cam0 = np.stack((rng.uniform(-0.6, 0.6, (n, H, W)) * z, rng.uniform(-0.45, 0.45, (n, H, W)) * z, z), -1)
    world = (cam0 @ poses[0, :3, :3].astype(np.float64).T + poses[0, :3, 3].astype(np.float64)).astype(np.float32)
    masks = rng.random((n, H, W)) < 0.7
    scale, shift = rng.uniform(0.4, 2.0), rng.uniform(-0.5, 0.5)

    def predict(frames):
        return ((cam0[frames] + rng.normal(0, 0.02, cam0[frames].shape)) * scale + np.array([0, 0, shift])).astype(np.float32)
    pred_l, pred_r = predict(slice(0, n - 1)), predict(slice(1, n))
    conf_l, conf_r, conf = (1 + rng.random(s).astype(np.float32) for s in ((n - 1, H, W), (n - 1, H, W), (n, H, W)))
    img = (rng.integers(0, 256, (n, 3, H, W)) / np.float32(127.5) - np.float32(1.0)).astype(np.float32)
    return dict(world=world, masks=masks, poses=poses, pred_l=pred_l, pred_r=pred_r, conf_l=conf_l, conf_r=conf_r, conf=conf, img=img)


def eval_align_digest(case):
    import hashlib
    h = hashlib.sha256()
    for k in sorted(case):
        h.update(np.ascontiguousarray(case[k]).tobytes())
    return h.hexdigest()


def eval_align_batch(case, to_tensor, dtype=None):
    """(views, preds, preds_all) shaped like the reference's batch and Spann3R.forward's outputs (res1 has 'pts3d' for the first
    pair, 'pts3d_in_other_view' afterwards; res2 always the latter); to_tensor(array) makes the tensors"""
    def t(a):
        a = np.asarray(a)
        return to_tensor(a.astype(dtype) if dtype is not None and a.dtype == np.float32 else a)
    n = len(case["world"])
    views = [dict(pts3d=t(case["world"][i][None]), valid_mask=t(case["masks"][i][None]), camera_pose=t(case["poses"][i][None]),
                  img=t(case["img"][i][None])) for i in range(n)]
    preds_all = [({("pts3d" if i == 0 else "pts3d_in_other_view"): t(case["pred_l"][i][None]), "conf": t(case["conf_l"][i][None])},
                  {"pts3d_in_other_view": t(case["pred_r"][i][None]), "conf": t(case["conf_r"][i][None])}) for i in range(n - 1)]
    preds = [dict(conf=t(case["conf"][i][None])) for i in range(n)]
    return views, preds, preds_all


def lower_median(x):
    x = np.sort(np.asarray(x).ravel())
    return x[(len(x) - 1) // 2]


def eval_align_ref(case, dtype=np.float64):
    """The rule of sp3_eval_align and sp3_ssi_align_stats in numpy (float64 by default): medians (torch.nanmedian: the lower
    middle element) over the valid pixels of the sequence, then the alignment of include/spann3r_hip.h and the masked clouds in
    row-major order.  -> dict of gt_pts, pred_l, pred_r, monitoring (gt_shift_z, pred_shift_z, gt_scale, pred_scale), pts_all,
    pts_gt_all, images_all, pred_cloud, gt_cloud, cloud_colors, cloud_index."""
    f = lambda a: np.asarray(a).astype(dtype)
    world, m, P0 = f(case["world"]), case["masks"], f(case["poses"][0])
    n = len(world)
    Pi = np.linalg.inv(P0)
    gt = world @ Pi[:3, :3].T + Pi[:3, 3]
    pl, pr = f(case["pred_l"]), f(case["pred_r"])
    sel = np.concatenate((pl, pr[-1:]))
    gs, ps = lower_median(gt[..., 2][m]), lower_median(sel[..., 2][m])
    gt = gt - np.array([0, 0, gs], dtype)
    shift = np.array([0, 0, ps], dtype)
    pl, pr, sel = pl - shift, pr - shift, sel - shift
    gsc = lower_median(np.linalg.norm(gt[m] - np.array([lower_median(gt[..., c][m]) for c in range(3)], dtype), axis=-1))
    psc = lower_median(np.linalg.norm(sel[m] - np.array([lower_median(sel[..., c][m]) for c in range(3)], dtype), axis=-1))
    psc = min(max(psc, 1e-3), 1e3)
    pl, pr, sel = pl * (gsc / psc), pr * (gsc / psc), sel * (gsc / psc)
    back = np.array([0, 0, gs], dtype)
    pts_all = (sel + back) @ P0[:3, :3].T + P0[:3, 3]
    pts_gt_all = (gt + back) @ P0[:3, :3].T + P0[:3, 3]
    images = (f(case["img"]).transpose(0, 2, 3, 1) + 1.0) / 2.0
    return dict(gt_pts=gt, pred_l=pl, pred_r=pr, monitoring=dict(gt_shift_z=gs, pred_shift_z=ps, gt_scale=gsc, pred_scale=psc),
                pts_all=pts_all, pts_gt_all=pts_gt_all, images_all=images, pred_cloud=pts_all[m], gt_cloud=pts_gt_all[m],
                cloud_colors=images[m], cloud_index=np.flatnonzero(m.ravel()))
