"""Multi-view consistency of pointmaps on the device; cleaned confidences.

`Spann3R.forward` gives every frame a pointmap in the first camera's frame and a confidence, and everything downstream keeps or
drops a pixel by that one per-frame number.  Nothing asks the other frames whether a point can be where it claims to be: a flying
pixel at a depth discontinuity survives although other cameras look straight through it.  Here every pixel's point is looked up in
every other frame (sp3_multiview_counts: ONE launch for all pairs, one lane per pixel): how many frames see it, agree with it, have it
floating in front of what they measured, or have it behind; and its confidence is clipped where a more confident frame looks
through it (sp3_multiview_clean) -- the rule of DUSt3R's BasePCOptimizer.clean_pointcloud with the projection and lookup of
sp3_tsdf_integrate.  csrc/multiview.hip; rules in include/spann3r_hip.h "Multi-view consistency".

What is unpinned: parity with clean_pointcloud itself (dust3r.cloud_opt cannot be imported here); tests/multiview_ref.py restates
the header's rule in numpy and the kernel is checked against that bit for bit.  `clean_sequence` inherits whatever error
`estimate_poses` and the single shared focal of `estimate_focal_knowing_depth` have.  torch provides memory; there is no CPU path."""
import math

import numpy as np
import torch

from . import lib as L
from .fusion import _dev, _frames_list, camera_tables

COUNT_NAMES = ("seen", "agree", "front", "stronger")


def frame_table(pts, intrinsics, cam2world, valid=None, conf=None):
    """The sp3_tsdf_frame table of T pointmaps: pts [t, h, w, 3] or a list of device tensors [h, w, 3] of mixed sizes; intrinsics
    [3, 3] or [t, 3, 3]; cam2world [t, 4, 4], inverted in float64 on the host; valid (bool / uint8) and conf (fp32, the table's
    pixel_weight) are optional, and lists of them may hold None for single frames.  Skewed intrinsics and non-finite or singular
    poses are refused exactly as fusion.camera_tables refuses them.  -> (host table, device copy, T, the tensors it points to:
    dict(pts, valid, conf) of lists)."""
    src = _frames_list(pts, "pts", (3,))
    if src is None:
        raise ValueError("frame_table: pts is required")
    T = len(src)
    fk, w2c = camera_tables(intrinsics, cam2world, T)
    maps = {"valid": _frames_list(valid, "valid", (), True), "conf": _frames_list(conf, "conf", (), True)}
    for name, m in maps.items():
        if m is not None and len(m) != T:
            raise RuntimeError("frame_table: mismatched lengths: %d frames, %d %s maps" % (T, len(m), name))
    table = (L.TsdfFrame * max(T, 1))()
    keep = dict(pts=[], valid=[], conf=[])
    for i in range(T):
        s = src[i].float().contiguous()
        h, w = s.shape[:2]
        e = table[i]
        e.depth, e.pts = None, s.data_ptr()
        keep["pts"].append(s)
        for name, m in maps.items():
            if m is not None and m[i] is not None and tuple(m[i].shape[:2]) != (h, w):
                raise RuntimeError("frame_table: mismatched shapes: frame %d is %d x %d, its %s map %s" % (i, h, w, name, tuple(m[i].shape)))
            if m is not None and m[i] is not None and m[i].device != s.device:
                raise RuntimeError("frame_table: frame %d: its %s map is on another device" % (i, name))
        v = a = None
        if maps["valid"] is not None and maps["valid"][i] is not None:
            v = maps["valid"][i].to(torch.uint8).contiguous()
            e.valid = v.data_ptr()
        if maps["conf"] is not None and maps["conf"][i] is not None:
            a = maps["conf"][i].float().contiguous()
            e.pixel_weight = a.data_ptr()
        keep["valid"].append(v)
        keep["conf"].append(a)
        e.row_stride, e.w, e.h = w, w, h
        e.fu, e.fv, e.cu, e.cv = (float(x) for x in fk[i])
        e.w2c[:] = w2c[i].tolist()
    table_d = None
    if T:
        table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(src[0].device)
    return table, table_d, T, keep


def _check_tol(what, tol):
    tol = float(tol)
    if not (0.0 <= tol < 1.0) or not (0.0 <= float(np.float32(tol)) < 1.0):
        raise ValueError("%s: tol %r must lie in [0, 1)" % (what, tol))
    return tol


def _run(what, tbl, tol, want_counts, clean, max_bad_conf):
    """one counts call (clean None or "parallel") or one sequence-order call over a frame_table -> (counts: list of int32 [h, w, 4] or
    None, conf: list of fp32 [h, w] or None)"""
    table, table_d, T, keep = tbl
    counts = conf = None
    shapes = [tuple(p.shape[:2]) for p in keep["pts"]]
    if want_counts:      # (every pixel of a launched frame is written; a frame the launch does not reach holds zeros)
        counts = [torch.zeros(s + (4,), dtype=torch.int32, device=p.device) for s, p in zip(shapes, keep["pts"])]
    if clean is not None:
        conf = [torch.empty_like(c) for c in keep["conf"]]
    if T == 0:
        return counts, conf
    if min(min(s) for s in shapes) == 0:      # an empty frame: no descriptor can say that
        if max(max(s) for s in shapes) != 0:
            raise RuntimeError("%s: a frame without pixels among frames with pixels" % what)
        return counts, conf
    out = (L.MultiviewOut * T)()
    for i in range(T):
        out[i].counts = counts[i].data_ptr() if want_counts else None
        out[i].conf_out = conf[i].data_ptr() if clean is not None else None
        out[i].max_bad_conf = float(max_bad_conf)
    out_d = torch.frombuffer(bytearray(bytes(out)), dtype=torch.uint8).to(table_d.device)
    lib = L.load()
    fn, name = (lib.sp3_multiview_clean, "sp3_multiview_clean") if clean == "sequence" else (lib.sp3_multiview_counts, "sp3_multiview_counts")
    L.check(fn(table, table_d.data_ptr(), T, tol, out, out_d.data_ptr(), L.stream_ptr()), name)
    return counts, conf


def _counts_dict(counts, stacked):
    """list of [h, w, 4] -> dict of seen, agree, front, behind, stronger: int32 [t, h, w] stacks, or lists for frames given as a list"""
    per = []
    for c in counts:
        d = {n: c[..., k].contiguous() for k, n in enumerate(COUNT_NAMES)}
        d["behind"] = d["seen"] - d["agree"] - d["front"]
        per.append(d)
    names = COUNT_NAMES[:3] + ("behind", "stronger")
    if stacked:
        return {n: torch.stack([d[n] for d in per]) for n in names}
    return {n: [d[n] for d in per] for n in names}


def _empty_stack(pts, dtype):
    return torch.zeros(tuple(pts.shape[:3]), dtype=dtype, device=pts.device)


def view_consistency(pts, intrinsics, cam2world, valid=None, conf=None, tol=1e-3):
    """Every pixel's world point looked up in every other frame, in ONE launch -> dict of seen, agree, front, behind, stronger, each
    int32 [t, h, w] (lists of [h, w] when pts is a list: frames of mixed sizes).  Arguments as frame_table.  A lookup is *seen* when
    the point projects in front of frame j into a valid pixel with a finite positive depth d (the camera z of j's own point there);
    it is *front* when its camera z is below (1 - tol) d -- it floats in front of what j measured, a free-space violation --,
    *behind* when above (1 + tol) d -- occluded, which says nothing -- and *agree* otherwise; *stronger* counts the front lookups
    where j is the more confident (both frames need conf; 0 otherwise).  An invalid pixel has all counts 0.  tol is a RELATIVE DEPTH
    TOLERANCE, a convention and not an error bound (see clean_confidence).  Nothing synchronises."""
    tol = _check_tol("view_consistency", tol)
    stacked = isinstance(pts, torch.Tensor)
    tbl = frame_table(pts, intrinsics, cam2world, valid, conf)
    if stacked and tbl[2] == 0:
        z = _empty_stack(_dev(pts, "view_consistency: pts"), torch.int32)
        return {n: z.clone() for n in COUNT_NAMES[:3] + ("behind", "stronger")}
    counts, _ = _run("view_consistency", tbl, tol, True, None, 0.0)
    return _counts_dict(counts, stacked)


def clean_confidence(pts, conf, intrinsics, cam2world, valid=None, tol=1e-3, max_bad_conf=0.0, order="sequence", return_counts=False):
    """The confidences with every pixel clipped to at most max_bad_conf that floats in front of what a MORE CONFIDENT frame measured
    there (DUSt3R's clean_pointcloud; tol and max_bad_conf default to its values) -> fp32 shaped like conf ([t, h, w], or a list);
    with return_counts also view_consistency's dict, against the original confidences.  Every frame needs a confidence.
    order="sequence" (that method's in-place loop, T launches): frames are cleaned in order, and frame i is judged against the
    already cleaned confidences of the frames before it and the original ones of the frames after it.  order="parallel" (one launch):
    every frame is judged against the original confidences; a pixel is clipped iff its `stronger` count is > 0.
    tol is a convention, not a pass/fail number: that method runs on optimised depth maps; raw predictions want a larger tol (a few
    per cent), or nearly every overlap counts as front or behind.  The depth of frame j is taken at the NEAREST pixel, so a slanted
    surface seen at low resolution looks inconsistent by up to its depth change over half a pixel however good the prediction is.
    A NaN confidence is never clipped.  Nothing synchronises."""
    tol = _check_tol("clean_confidence", tol)
    if order not in ("sequence", "parallel"):
        raise ValueError("clean_confidence: order must be 'sequence' or 'parallel', got %r" % (order,))
    max_bad_conf = float(max_bad_conf)
    if math.isnan(max_bad_conf):
        raise ValueError("clean_confidence: max_bad_conf is NaN")
    if conf is None or (not isinstance(conf, torch.Tensor) and any(c is None for c in conf)):
        raise ValueError("clean_confidence: every frame needs a confidence")
    stacked = isinstance(conf, torch.Tensor)
    tbl = frame_table(pts, intrinsics, cam2world, valid, conf)
    if tbl[2] == 0:
        clean = conf.float().clone() if stacked else []
        names = COUNT_NAMES[:3] + ("behind", "stronger")
        return (clean, {n: (torch.zeros(tuple(conf.shape), dtype=torch.int32, device=conf.device) if stacked else []) for n in names}) \
            if return_counts else clean
    counts, out = _run("clean_confidence", tbl, tol, return_counts, order, max_bad_conf)
    clean = torch.stack(out) if stacked else out
    return (clean, _counts_dict(counts, isinstance(pts, torch.Tensor))) if return_counts else clean


def support_mask(counts, min_agree=1, max_front=0):
    """The pixels at least min_agree other frames agree with and at most max_front look through: bool, shaped like the counts of
    view_consistency's dict (the geometric filter of multi-view stereo fusion).  Plain torch on the counts."""
    a, f = counts["agree"], counts["front"]
    if isinstance(a, torch.Tensor):
        return (a >= min_agree) & (f <= max_front)
    return [(x >= min_agree) & (y <= max_front) for x, y in zip(a, f)]


def clean_sequence(preds, batch, tol=1e-3, max_bad_conf=0.0, order="sequence", focal=None, poses=None):
    """clean_confidence for model.forward's `preds` and its `batch`, behind the front end of fusion.fuse_sequence: the stacked pointmaps
    (mesh.sequence_tensors), the focal of frame 0 (estimate_focal_knowing_depth) and one pose per frame (estimate_poses), unless focal /
    poses (cam2world [t, 4, 4]) are given.  -> (pts_all, images_all, conf_clean, dict(focal, poses, cleaned = the pixels clipped per
    frame, a list)).  Pointmaps without geometry give a focal near 0: that raises, as in fuse_sequence."""
    from . import mesh as M
    from .postprocess import estimate_focal_knowing_depth, estimate_poses
    pts_all, images_all, conf_all = M.sequence_tensors(preds, batch)
    _dev(pts_all, "clean_sequence: pts3d")
    t, h, w, _ = pts_all.shape
    pp = (w / 2, h / 2)
    if focal is None:
        focal = float(estimate_focal_knowing_depth(pts_all[:1], torch.tensor(pp), focal_mode="weiszfeld").item())
        if not (focal > 1e-3 and math.isfinite(focal)):
            raise RuntimeError("clean_sequence: degenerate pointmaps: the focal of the first frame came out as %g" % focal)
    focal = float(focal)
    if not (focal > 0 and math.isfinite(focal)):
        raise ValueError("clean_sequence: focal must be positive and finite, got %r" % focal)
    if poses is None:
        poses, _ = estimate_poses(pts_all, focal, pp)
    poses = np.asarray(poses, np.float64)
    K = np.array([[focal, 0, pp[0]], [0, focal, pp[1]], [0, 0, 1]], np.float64)
    conf_clean = clean_confidence(pts_all, conf_all, K, poses, tol=tol, max_bad_conf=max_bad_conf, order=order)
    # (a clipped pixel is one whose bits changed; NaN passes through, so compare the bit patterns)
    cleaned = (conf_clean.view(torch.int32) != conf_all.contiguous().view(torch.int32)).flatten(1).sum(1).cpu().tolist()
    return pts_all, images_all, conf_clean, dict(focal=focal, poses=poses, cleaned=cleaned)
