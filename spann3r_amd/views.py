"""RGB-D views with ground truth, on the MI355X: decoded frames (image, depth, K, cam2world) -> the list of view dicts that the
reference's `DataLoader(SevenScenes(...), batch_size=1)` yields for one sequence, i.e. what `TrainStep`, `ConfLoss_t.compute_frame_loss`,
`Regr3D_t_ScaleShiftInv` and the evaluation consume as `gts`.

Mirrors, per view, `BaseStereoViewDataset._crop_resize_if_necessary` + `__getitem__` + `transpose_to_landscape`
(dust3r/datasets/base/base_stereo_view_dataset.py:63-119,143-194,215-220), the cropping helpers (dust3r/datasets/utils/cropping.py:54-120),
`depthmap_to_absolute_camera_coordinates` (dust3r/utils/geometry.py:165-217), the depth sanitising of the data-set classes
(spann3r/datasets/seven_scenes.py:123-126) and the frame sampling of spann3r/datasets/base_many_view_dataset.py:9-50.

Host part (this file): the crop plan for real intrinsics and the camera-matrix arithmetic in the reference's dtypes and order, the
sampling draws, the descriptor table.  Device part: the image through sp3_preprocess_image (csrc/preproc.hip, bit-exact with Pillow),
the depth side of the WHOLE sequence through one sp3_view_depth launch (csrc/views.hip).  There is no CPU path; tests/views_ref.py
holds the restatement the kernel is checked against.

Not here: file decoding (PNG / EXR readers, the per-data-set folder layouts, Co3D's mask_bg) and ColorJitter -- see INTEGRATION.md.
The nearest-neighbour index rule restates OpenCV's INTER_NEAREST (include/spann3r_hip.h); parity with cv2 itself is unpinned."""
import ctypes as C
import math

import numpy as np
import torch

from . import lib as L
from . import preprocess as PP

LAUNCHES = {"sp3_view_depth": 0}        # launch counter: build_views issues exactly one sp3_view_depth per call


def plan_rgbd_view(H, W, K, resolution, rng=None, aug_crop=0):
    """The plan of `_crop_resize_if_necessary` for an H x W frame with REAL intrinsics K (3x3, taken as float32 like the data-set
    classes build it).  resolution = (width, height) with width >= height, or an int.  Returns
      crop0 (l, t, r, b) around K[:2, 2].round(); resize (W2, H2); crop1 (l2, t2, r2, b2) in the resized image; out (w, h);
      transpose (h > w: the view is rectified to landscape); K_crop: the float32 intrinsics of the cropped [h, w] view (camera-matrix
      arithmetic in the reference's dtypes and order -- the final offset is a ROUNDED difference); camera_intrinsics: what the view
      dict carries, K_crop with rows permuted [1, 0, 2] for a portrait view, exactly as transpose_to_landscape leaves it.
    rng: the data set's per-item generator -- `rng.integers(2)` for a near-square crop with a non-square resolution, then
    `rng.integers(0, aug_crop)` when aug_crop > 1, in the reference's order.  rng=None: no coin (landscape), and aug_crop must be 0."""
    if isinstance(resolution, int):
        resolution = (resolution, resolution)
    K = np.array(K, dtype=np.float32)
    if K.shape != (3, 3):
        raise ValueError("K must be 3x3")
    cx, cy = K[:2, 2].round().astype(int)
    mx, my = min(cx, W - cx), min(cy, H - cy)
    if not mx > W / 5:
        raise ValueError("Bad principal point: column %d of a %d-wide frame" % (cx, W))
    if not my > H / 5:
        raise ValueError("Bad principal point: row %d of a %d-high frame" % (cy, H))
    l, t, r, b = int(cx - mx), int(cy - my), int(cx + mx), int(cy + my)
    K[0, 2] -= l
    K[1, 2] -= t
    W1, H1 = r - l, b - t
    res = tuple(int(v) for v in resolution)
    if res[0] < res[1]:
        raise ValueError("resolution must be (width, height) with width >= height")
    if H1 > 1.1 * W1:
        res = res[::-1]
    elif 0.9 < H1 / W1 < 1.1 and res[0] != res[1]:
        if rng is not None and rng.integers(2):
            res = res[::-1]
    target = np.array(res)
    if aug_crop > 1:
        if rng is None:
            raise ValueError("aug_crop needs the generator it draws from")
        target += rng.integers(0, aug_crop)
    in_res = np.array((W1, H1))
    scale_final = max(target / in_res) + 1e-8
    out_res = np.floor(in_res * scale_final).astype(int)
    K1 = PP._crop_matrix(K, in_res, out_res, scaling=scale_final)
    K2 = PP._crop_matrix(K1, tuple(out_res), res)
    l2, t2 = np.int32(np.round(K1[:2, 2] - K2[:2, 2]))
    Kc = K1.copy()
    Kc[0, 2] -= l2
    Kc[1, 2] -= t2
    transpose = res[1] > res[0]
    return dict(crop0=(l, t, r, b), resize=(int(out_res[0]), int(out_res[1])), crop1=(int(l2), int(t2), int(l2) + res[0], int(t2) + res[1]),
                out=res, transpose=transpose, K_crop=Kc, camera_intrinsics=Kc[[1, 0, 2]] if transpose else Kc)


def _depth_to_device(depth, device):
    """uint16 or float32 [H, W] -> (contiguous device tensor, dtype code of sp3_view_desc).  uint16 travels as its int16 bit pattern."""
    if isinstance(depth, np.ndarray):
        if depth.dtype == np.uint16:
            return torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(device), 0
        if depth.dtype == np.float32:
            return torch.from_numpy(np.ascontiguousarray(depth)).to(device), 1
    elif isinstance(depth, torch.Tensor):
        if depth.dtype == getattr(torch, "uint16", None):
            return depth.to(device).contiguous(), 0
        if depth.dtype == torch.float32:
            return depth.to(device).contiguous(), 1
    raise TypeError("expected a uint16 or float32 [H, W] depth map")


def build_views(rgbs, depths, intrinsics, poses, resolution=224, device="cuda", rng=None, aug_crop=0, depth_div=1.0, raw_invalid=None,
                min_depth=0.0, max_depth=math.inf, dataset="rgbd", labels=None, debug_xcam=False):
    """One sequence of decoded frames -> the list of n view dicts the reference's DataLoader(batch_size=1) yields for it:
    img [1, 3, h, w] in [-1, 1], depthmap [1, h, w], camera_pose [1, 4, 4], camera_intrinsics [1, 3, 3], pts3d [1, h, w, 3] (world),
    valid_mask [1, h, w] bool -- all on the device, views of the per-sequence buffers -- true_shape int32 [1, 2] on the CPU, idx,
    instance, label, dataset.  rgbs: uint8 [H, W, 3]; depths: uint16 or float32 [H, W]; intrinsics: 3x3; poses: 4x4 cam2world
    (arrays or tensors, host or device; frames of one call may differ in size and dtype, the output size is common).

    Depth is sanitised on the device as the data-set classes do on the host: raw == raw_invalid -> 0, float32(raw) / depth_div,
    non-finite -> 0, > max_depth -> 0, < min_depth -> 0.  The images go through sp3_preprocess_image with the K-derived plan, the depth
    side of all views through ONE sp3_view_depth launch.  Host -> device copies: the raw bytes, one block of poses and intrinsics,
    the descriptor table (and, once per size, the cached resampling tables).  Nothing synchronises.
    debug_xcam: every view also carries `pts3d_cam`, the camera-frame points the kernel rotated."""
    n = len(rgbs)
    if not (len(depths) == len(intrinsics) == len(poses) == n) or (labels is not None and len(labels) != n):
        raise ValueError("build_views: rgbs, depths, intrinsics, poses (and labels) must have one entry per view")
    if n == 0:
        return []
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("build_views runs on the GPU (HIP kernels); there is no CPU path")
    plans, srcs, cams = [], [], np.empty((n, 25), np.float32)
    table = (L.ViewDesc * n)()
    for i in range(n):
        src = PP._rgb_to_device(rgbs[i], dev)
        H, W, _ = src.shape
        d, code = _depth_to_device(depths[i], dev)
        if tuple(d.shape) != (H, W):
            raise ValueError("view %d: depth map %s does not match the %dx%d image" % (i, tuple(d.shape), H, W))
        Ki = intrinsics[i].cpu().numpy() if isinstance(intrinsics[i], torch.Tensor) else np.asarray(intrinsics[i])
        if Ki[0, 1] != 0.0 or Ki[1, 0] != 0.0:
            raise ValueError("view %d: intrinsics with a skew term" % i)
        p = plan_rgbd_view(H, W, Ki, resolution, rng, aug_crop)
        pose = poses[i].cpu().numpy() if isinstance(poses[i], torch.Tensor) else np.asarray(poses[i])
        pose = pose.astype(np.float32)
        if pose.shape != (4, 4) or not np.isfinite(pose).all():
            raise ValueError("view %d: camera pose must be a finite 4x4 cam2world matrix" % i)
        cams[i, :16], cams[i, 16:] = pose.ravel(), p["camera_intrinsics"].ravel()
        Kc, e = p["K_crop"], table[i]
        e.src, e.row_stride, e.dtype, e.src_w, e.src_h = d.data_ptr(), W, code, W, H
        e.crop_l, e.crop_t, e.W1, e.H1 = p["crop0"][0], p["crop0"][1], p["crop0"][2] - p["crop0"][0], p["crop0"][3] - p["crop0"][1]
        e.W2, e.H2 = p["resize"]
        e.l2, e.t2 = p["crop1"][:2]
        e.w, e.h = p["out"]
        e.transpose = int(p["transpose"])
        e.fu, e.fv, e.cu, e.cv = float(Kc[0, 0]), float(Kc[1, 1]), float(Kc[0, 2]), float(Kc[1, 2])
        e.pose[:] = pose[:3].ravel().tolist()
        e.use_raw_invalid, e.raw_invalid = (0, 0.0) if raw_invalid is None else (1, float(raw_invalid))
        e.depth_div, e.min_depth, e.max_depth = float(depth_div), float(min_depth), float(max_depth)
        plans.append(p)
        srcs.append((src, d))
    sizes = {(max(p["out"]), min(p["out"])) for p in plans}
    if len(sizes) != 1:
        raise ValueError("build_views: the views of one call must share one output size, got %s" % sorted(sizes))
    (ow, oh), = sizes
    imgs = torch.empty(n, 3, oh, ow, device=dev)
    depth = torch.empty(n, oh, ow, device=dev)
    pts = torch.empty(n, oh, ow, 3, device=dev)
    mask = torch.empty(n, oh, ow, dtype=torch.uint8, device=dev)
    xcam = torch.empty(n, oh, ow, 3, device=dev) if debug_xcam else None
    for i in range(n):
        PP.run_plan(srcs[i][0], plans[i], out=imgs[i:i + 1])
    cams_d = torch.from_numpy(cams).to(dev)
    table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    L.check(L.load().sp3_view_depth(table, table_d.data_ptr(), n, oh, ow, depth.data_ptr(), pts.data_ptr(), mask.data_ptr(), L.ptr(xcam),
                                    L.stream_ptr()), "sp3_view_depth")
    LAUNCHES["sp3_view_depth"] += 1
    valid = mask.view(torch.bool)
    views = []
    for i, p in enumerate(plans):
        w, h = p["out"]
        v = dict(img=imgs[i:i + 1], depthmap=depth[i:i + 1], camera_pose=cams_d[i:i + 1, :16].reshape(1, 4, 4),
                 camera_intrinsics=cams_d[i:i + 1, 16:].reshape(1, 3, 3), pts3d=pts[i:i + 1], valid_mask=valid[i:i + 1],
                 true_shape=torch.tensor([[h, w]], dtype=torch.int32), idx=i, instance=str(i),
                 label=str(i) if labels is None else labels[i], dataset=dataset)
        if debug_xcam:
            v["pts3d_cam"] = xcam[i:i + 1]
        views.append(v)
    return views


def stack_sequences(list_of_view_lists):
    """B sequences of n views each (build_views) -> one list of n views with batch size B, for TrainStep and the criteria: a plain
    concatenation along dim 0 of views of equal shape; idx / instance / label / dataset become lists."""
    seqs = list(list_of_view_lists)
    if not seqs or any(len(s) != len(seqs[0]) for s in seqs):
        raise ValueError("stack_sequences: need sequences of one common length")
    out = []
    for frame in zip(*seqs):
        v = {}
        for k in frame[0]:
            vals = [f[k] for f in frame]
            if isinstance(vals[0], torch.Tensor):
                if any(x.shape[1:] != vals[0].shape[1:] for x in vals):
                    raise ValueError("stack_sequences: views of different shapes for %r" % k)
                v[k] = torch.cat(vals, 0)
            else:
                v[k] = vals
        out.append(v)
    return out


def sample_frames(n_images, num_frames, min_thresh, max_thresh, train_ratio, rng):
    """spann3r/datasets/base_many_view_dataset.py:9-41, draw for draw: num_frames increasing indices into a video of n_images frames
    with gaps of at most thresh = int(min_thresh + train_ratio * (max_thresh - min_thresh)), the whole draw repeated when it runs out
    of room, reversed on a final coin.  The same rng.choice calls on the same lists in the same order as the reference."""
    thresh = int(min_thresh + train_ratio * (max_thresh - min_thresh))
    idx = list(range(n_images))
    sel = []
    first = max(len(idx) // num_frames, len(idx) - thresh * (num_frames - 1))
    cur = rng.choice(idx[:first])
    sel.append(cur)
    while len(sel) < num_frames:
        lo, hi = cur + 1, min(cur + thresh, len(idx) - (num_frames - len(sel)))
        possible = [i for i in range(lo, hi + 1) if i not in sel]
        if not possible:
            break
        cur = rng.choice(possible)
        sel.append(cur)
    if len(sel) < num_frames:
        return sample_frames(n_images, num_frames, min_thresh, max_thresh, train_ratio, rng)
    sel = [int(i) for i in sel]
    if rng.choice([True, False]):
        sel.reverse()
    return sel


def sample_frame_idx(img_idxs, rng, num_frames=5, min_thresh=10, max_thresh=30, train_ratio=1.0, full_video=False, kf_every=1):
    """base_many_view_dataset.py:44-50: the sampled frames of `img_idxs`, or every kf_every-th one for full_video."""
    if full_video:
        return img_idxs[::kf_every]
    return [img_idxs[i] for i in sample_frames(len(img_idxs), num_frames, min_thresh, max_thresh, train_ratio, rng)]
