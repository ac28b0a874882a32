"""Headless `--vis` of demo.py on the device (reference: demo.py:221-225, spann3r/tools/vis.py:17-76 and 135-201).

The reference replays a reconstruction through an Open3D `Visualizer` window: one 1920x1080 picture of the cloud as it grows (or of
each frame's points alone with `--dynamic`), re-uploading the whole accumulated cloud for every frame.  That needs a display and
Open3D.  Here the predictions already live on the device and a z-buffered point rasteriser draws them (csrc/render.hip): the
z-buffer is one 64-bit key per pixel, (depth bits) << 32 | point index, updated by atomic min, so it persists between frames and a
frame costs its NEW points only; the picture is bitwise reproducible.  `vis_pred_and_imgs`' hue images and jet-coloured
confidences are HIP as well.  torch provides memory, the min / max of the normalisation and the sorts behind `fit_camera`'s
quantiles; Pillow writes the PNGs.

Conventions: OpenCV cameras as in postprocess.estimate_poses (+z forward, pixel centres at integer coordinates); the world frame is
the first camera's frame.  What the rasteriser draws is pinned to a float64 restatement of its own rule (tests/render_ref.py).
Open3D is not available to the tests: parity with Open3D's OpenGL point rendering (its near / far planes, its point sprites) is
unpinned.  There is no mp4 output either: imageio and ffmpeg are absent, the PNG folders are the product."""
import ctypes as C
import json
import math
import os

import numpy as np
import torch

from . import lib as L

WIDTH, HEIGHT = 1920, 1080            # the reference's window (vis.py:21)


# ------------------------------------------------------------------------------------------------ cameras
class Camera:
    """A pinhole camera: intrinsic 3x3, extrinsic 4x4 world-to-camera (float64 numpy, held as given), image size."""

    def __init__(self, intrinsic, extrinsic, width=WIDTH, height=HEIGHT):
        self.intrinsic = np.array(intrinsic, dtype=np.float64).reshape(3, 3)
        self.extrinsic = np.array(extrinsic, dtype=np.float64).reshape(4, 4)
        self.width, self.height = int(width), int(height)

    def render_cam(self, point_size=1, z_near=0.0):
        """the sp3_render_cam the kernels read (fp32)"""
        K, E = self.intrinsic, self.extrinsic
        return L.RenderCam((C.c_float * 9)(*E[:3, :3].reshape(-1)), (C.c_float * 3)(*E[:3, 3]), K[0, 0], K[1, 1], K[0, 2], K[1, 2],
                           self.width, self.height, z_near, int(point_size))


def save_camera(path, cam):
    """Open3D's PinholeCameraParameters JSON (what write_pinhole_camera_parameters writes): matrices column-major."""
    d = {"class_name": "PinholeCameraParameters",
         "extrinsic": [float(v) for v in cam.extrinsic.T.reshape(-1)],
         "intrinsic": {"height": cam.height, "intrinsic_matrix": [float(v) for v in cam.intrinsic.T.reshape(-1)], "width": cam.width},
         "version_major": 1, "version_minor": 0}
    with open(path, "w") as f:
        json.dump(d, f, indent="\t")          # (repr of a float64 round-trips bit for bit)


_save_camera = save_camera          # (render_frames has the reference's boolean parameter of that name)


def load_camera(path):
    """A camera saved by `save_camera`, or by Open3D (e.g. one picked with the reference's interactive find_render_cam)."""
    with open(path) as f:
        d = json.load(f)
    if d.get("class_name") != "PinholeCameraParameters":
        raise ValueError("%s: class_name %r, expected 'PinholeCameraParameters'" % (path, d.get("class_name")))
    it = d["intrinsic"]
    if len(d["extrinsic"]) != 16 or len(it["intrinsic_matrix"]) != 9:
        raise ValueError("%s: expected 16 extrinsic and 9 intrinsic numbers" % path)
    return Camera(np.array(it["intrinsic_matrix"], np.float64).reshape(3, 3).T, np.array(d["extrinsic"], np.float64).reshape(4, 4).T,
                  it["width"], it["height"])


def camera_for_box(lo, hi, width=WIDTH, height=HEIGHT, fov_deg=60.0):
    """The camera `fit_camera` gives for the box [lo, hi] (host, float64): it looks along the first camera's +z from the axis through
    the box centre, at the distance where the near face of the box just fits the frustum of vertical field of view `fov_deg`
    (principal point at the image centre): every corner projects inside the image and the binding one onto its border."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    f = 0.5 * height / math.tan(math.radians(fov_deg) / 2)
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    d = max(half[0] * f / max(cx, 0.5), half[1] * f / max(cy, 0.5)) * (1 + 1e-6)
    d = max(d, 1e-6 * max(float(np.abs(hi - lo).max()), 1e-30))
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.float64)
    E = np.eye(4)
    E[:3, 3] = -np.array([mid[0], mid[1], lo[2] - d])
    return Camera(K, E, width, height)


def fit_camera(points, width=WIDTH, height=HEIGHT, fov_deg=60.0, quantile=0.02, conf=None, conf_thresh=None):
    """The headless stand-in for the reference's interactive find_render_cam: `camera_for_box` of the per-axis [q, 1 - q] quantile box
    of the finite points (those with (conf - 1) / conf > conf_thresh when both are given); the quantiles are order statistics taken
    on the device."""
    pts = _dev(points, "fit_camera: points").reshape(-1, 3).float()
    keep = torch.isfinite(pts).all(dim=1)
    if conf is not None and conf_thresh is not None:
        c = _dev(conf, "fit_camera: conf").reshape(-1).float()
        if c.numel() != pts.shape[0]:
            raise RuntimeError("fit_camera: %d confidences for %d points" % (c.numel(), pts.shape[0]))
        keep &= (c - 1) / c > conf_thresh
    pts = pts[keep]
    n = pts.shape[0]
    if n == 0:
        raise RuntimeError("fit_camera: no finite point passes the confidence threshold")
    s = torch.sort(pts, dim=0)[0]
    k0, k1 = int(math.floor(quantile * (n - 1))), int(math.ceil((1 - quantile) * (n - 1)))
    box = s[[k0, k1]].double().cpu().numpy()
    return camera_for_box(box[0], box[1], width, height, fov_deg)


# ------------------------------------------------------------------------------------------------ the rasteriser
def _dev(x, name):
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s: expected a CUDA tensor, got %s" % (name, type(x).__name__))
    if not x.is_cuda:
        raise RuntimeError("%s: rendering runs on the GPU (HIP kernels); there is no CPU path -- pass a CUDA tensor" % name)
    return x


def _rgb_word(rgb):
    r, g, b = (min(max(int(math.floor(float(c) * 255 + 0.5)), 0), 255) for c in rgb)
    return r | g << 8 | b << 16 | 255 << 24


class PointRenderer:
    """A persistent z-buffer and the colour store of every point drawn into it.

    add(pts, colors, conf=None) splats one frame's points (cost: those points); image() resolves the buffer to a picture.  With
    dynamic=True every add() clears first and restarts the index, so the picture shows the last frame alone.  `background` and
    `colors` are floats in [0, 1].  conf_thresh: points are kept when (conf - 1) / conf > conf_thresh, tested in the kernel.
    Memory comes from torch, outside any graph capture; the colour store grows geometrically."""

    def __init__(self, width=None, height=None, camera=None, point_size=1, background=(0, 0, 0), conf_thresh=None, dynamic=False,
                 z_near=0.0, device="cuda"):
        if camera is None:
            raise ValueError("PointRenderer: a camera is required (vis.fit_camera, vis.load_camera or vis.Camera)")
        if (width is not None and width != camera.width) or (height is not None and height != camera.height):
            raise ValueError("PointRenderer: %sx%s asked, the camera is %dx%d" % (width, height, camera.width, camera.height))
        self.camera, self.width, self.height = camera, camera.width, camera.height
        self.cam = camera.render_cam(point_size, z_near)
        self.background, self.conf_thresh, self.dynamic = _rgb_word(background), conf_thresh, dynamic
        self.device = torch.device(device)
        self._lib = L.load()
        L.check(self._lib.sp3_render_splat(0, 0, 0.0, 0, 0, C.byref(self.cam), 0, 0), "sp3_render_splat")      # validates the camera
        self.keys = torch.empty(self.width * self.height, dtype=torch.int64, device=self.device)
        self.rgba = torch.empty(0, dtype=torch.int32, device=self.device)
        self.count = 0
        self.mesh_stats = None
        self.clear()

    def clear(self):
        L.check(self._lib.sp3_render_clear(self.keys.data_ptr(), self.keys.numel(), L.stream_ptr()), "sp3_render_clear")
        self.count = 0

    def _reserve(self, total):
        if total > self.rgba.numel():
            grown = torch.empty(max(total, 2 * self.rgba.numel()), dtype=torch.int32, device=self.device)
            grown[:self.count] = self.rgba[:self.count]
            self.rgba = grown

    def add(self, pts, colors, conf=None):
        pts, colors = _dev(pts, "PointRenderer.add: pts"), _dev(colors, "PointRenderer.add: colors")
        if pts.shape[-1] != 3 or colors.shape[-1] != 3:
            raise RuntimeError("PointRenderer.add: pts %s and colors %s must end in 3" % (tuple(pts.shape), tuple(colors.shape)))
        pts, colors = pts.reshape(-1, 3).float().contiguous(), colors.reshape(-1, 3).float().contiguous()
        n = pts.shape[0]
        if colors.shape[0] != n:
            raise RuntimeError("PointRenderer.add: mismatched lengths: %d points, %d colours" % (n, colors.shape[0]))
        if conf is not None:
            conf = _dev(conf, "PointRenderer.add: conf").reshape(-1).float().contiguous()
            if conf.numel() != n:
                raise RuntimeError("PointRenderer.add: mismatched lengths: %d points, %d confidences" % (n, conf.numel()))
            if self.conf_thresh is None:
                raise RuntimeError("PointRenderer.add: conf given but the renderer has no conf_thresh")
        if self.dynamic:
            self.clear()
        self._reserve(self.count + n)
        st = L.stream_ptr()
        L.check(self._lib.sp3_pack_rgba8(colors.data_ptr(), n, self.rgba.data_ptr() + 4 * self.count, st), "sp3_pack_rgba8")
        L.check(self._lib.sp3_render_splat(pts.data_ptr(), L.ptr(conf), float(self.conf_thresh or 0.0), n, self.count, C.byref(self.cam),
                                           self.keys.data_ptr(), st), "sp3_render_splat")
        self.count += n

    def add_mesh(self, pts, colors, conf=None, valid=None, max_bbox_px=4096):
        """One frame's pointmap pts [h, w, 3] drawn as its mesh (app.py:68-105: two triangles per pixel cell, forward windings; the
        rasteriser draws both orientations) instead of its points: sp3_mesh_faces builds the faces of the pixels that are finite,
        pass `valid` bool [h, w] or (conf - 1) / conf > conf_thresh, and sp3_render_tris draws them into the same key buffer, so
        add() and add_mesh() mix.  A triangle whose clipped bounding box holds more than max_bbox_px pixels is not drawn (a sheet
        stretched across a depth edge is no surface).  The index image counts pixels as add() counts points; nothing is read back."""
        from . import mesh as M
        pts, colors = _dev(pts, "PointRenderer.add_mesh: pts"), _dev(colors, "PointRenderer.add_mesh: colors")
        if pts.dim() != 3 or pts.shape[-1] != 3 or colors.shape != pts.shape:
            raise RuntimeError("PointRenderer.add_mesh: pts %s and colors %s must both be [h, w, 3]" % (tuple(pts.shape), tuple(colors.shape)))
        h, w = pts.shape[:2]
        n = h * w
        if conf is not None and valid is not None:
            raise RuntimeError("PointRenderer.add_mesh: give conf or valid, not both")
        if conf is not None:
            conf = _dev(conf, "PointRenderer.add_mesh: conf").float().contiguous()
            if conf.numel() != n:
                raise RuntimeError("PointRenderer.add_mesh: mismatched lengths: %d points, %d confidences" % (n, conf.numel()))
            if self.conf_thresh is None:
                raise RuntimeError("PointRenderer.add_mesh: conf given but the renderer has no conf_thresh")
        if valid is not None:
            if _dev(valid, "PointRenderer.add_mesh: valid").numel() != n:
                raise RuntimeError("PointRenderer.add_mesh: mismatched lengths: %d points, %d valid flags" % (n, valid.numel()))
            valid = valid.to(torch.uint8).contiguous()
        if int(max_bbox_px) <= 0:
            raise ValueError("PointRenderer.add_mesh: max_bbox_px must be > 0")
        pts, colors = pts.float().contiguous(), colors.float().contiguous()
        if self.dynamic:
            self.clear()
        self._reserve(self.count + n)
        st = L.stream_ptr()
        L.check(self._lib.sp3_pack_rgba8(colors.data_ptr(), n, self.rgba.data_ptr() + 4 * self.count, st), "sp3_pack_rgba8")
        faces, colour_px, counts = M.build_faces(1, h, w, self.device, valid=valid, conf=conf, conf_thresh=float(self.conf_thresh or 0.0), pts=pts,
                                                 both_windings=False, sync=False)
        if self.mesh_stats is None:
            self.mesh_stats = torch.zeros(2, dtype=torch.int64, device=self.device)      # triangles given, culled by max_bbox_px
        self.mesh_stats[0] += counts[0]
        L.check(self._lib.sp3_render_tris(pts.data_ptr(), n, faces.data_ptr(), colour_px.data_ptr(), faces.shape[0], counts.data_ptr(), self.count,
                                          C.byref(self.cam), int(max_bbox_px), self.keys.data_ptr(), self.mesh_stats.data_ptr() + 8, st),
                "sp3_render_tris")
        self.count += n

    def add_triangles(self, vertices, faces, colors, max_bbox_px=4096):
        """An indexed mesh -- vertices fp32 [V, 3], faces int32 [F, 3], colors uint8 [V, 4] / [V, 3] or floats in [0, 1] [V, 3] (the
        dict of fusion.TSDFVolume.extract_mesh or mesh.scene_mesh) -- drawn through sp3_render_tris into the same key buffer as add()
        and add_mesh().  A face takes the colour of its first vertex.  The index image counts the vertices as add() counts points."""
        vertices, faces, colors = (_dev(x, "PointRenderer.add_triangles: " + n) for x, n in ((vertices, "vertices"), (faces, "faces"), (colors, "colors")))
        if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
            raise RuntimeError("PointRenderer.add_triangles: vertices %s must be [V, 3] and faces %s [F, 3]" % (tuple(vertices.shape), tuple(faces.shape)))
        n = vertices.shape[0]
        if colors.dim() != 2 or colors.shape[0] != n or colors.shape[1] not in (3, 4):
            raise RuntimeError("PointRenderer.add_triangles: mismatched lengths: %d vertices, colours %s" % (n, tuple(colors.shape)))
        if int(max_bbox_px) <= 0:
            raise ValueError("PointRenderer.add_triangles: max_bbox_px must be > 0")
        if self.dynamic:
            self.clear()
        if n == 0 or faces.shape[0] == 0:
            return
        vertices, faces = vertices.float().contiguous(), faces.to(torch.int32).contiguous()
        self._reserve(self.count + n)
        st = L.stream_ptr()
        if colors.dtype == torch.uint8:
            if colors.shape[1] == 3:
                colors = torch.cat([colors, torch.full((n, 1), 255, dtype=torch.uint8, device=colors.device)], dim=1)
            self.rgba[self.count:self.count + n] = colors.contiguous().view(torch.int32).reshape(-1)
        else:
            if colors.shape[1] != 3:
                raise RuntimeError("PointRenderer.add_triangles: float colours must be [V, 3]")
            L.check(self._lib.sp3_pack_rgba8(colors.float().contiguous().data_ptr(), n, self.rgba.data_ptr() + 4 * self.count, st), "sp3_pack_rgba8")
        if self.mesh_stats is None:
            self.mesh_stats = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.mesh_stats[0] += faces.shape[0]
        L.check(self._lib.sp3_render_tris(vertices.data_ptr(), n, faces.data_ptr(), 0, faces.shape[0], 0, self.count, C.byref(self.cam),
                                          int(max_bbox_px), self.keys.data_ptr(), self.mesh_stats.data_ptr() + 8, st), "sp3_render_tris")
        self.count += n

    def image(self, return_depth=False, return_index=False):
        """uint8 [H, W, 3] on the device; with the flags, also depth fp32 [H, W] (+inf: empty) and index int32 [H, W] (-1: empty;
        the index counts every point given to add(), kept or not, in order)."""
        shape = (self.height, self.width)
        rgb = torch.empty(shape + (3,), dtype=torch.uint8, device=self.device)
        depth = torch.empty(shape, dtype=torch.float32, device=self.device) if return_depth else None
        index = torch.empty(shape, dtype=torch.int32, device=self.device) if return_index else None
        L.check(self._lib.sp3_render_resolve(self.keys.data_ptr(), L.ptr(self.rgba) if self.rgba.numel() else 0, C.byref(self.cam),
                                             self.background, rgb.data_ptr(), L.ptr(depth), L.ptr(index), L.stream_ptr()),
                "sp3_render_resolve")
        out = (rgb,) + ((depth,) if return_depth else ()) + ((index,) if return_index else ())
        return out[0] if len(out) == 1 else out


def _save_png(path, img):
    from PIL import Image
    Image.fromarray(img).save(path)


def render_frames(pts_all, images_all, camera, output_dir=None, mask=None, conf_all=None, conf_thresh=None, dynamic=False, save_camera=True,
                  point_size=1, background=(0, 0, 0), surface=False, max_bbox_px=4096):
    """vis.py:17-76: t pictures of pts_all [t, h, w, 3] coloured by images_all [t, h, w, 3] (floats in [0, 1]) seen from `camera`:
    the cloud as it grows, or each frame's points alone with dynamic=True.  Returned as a uint8 [t, H, W, 3] device tensor and, when
    output_dir is given, written as output_dir/render_frames/frame_%03d.png (plus camera.json with save_camera).  Points are
    selected by the reference's boolean `mask` [t, h, w] or by conf_all [t, h, w] and conf_thresh, tested in the kernel.
    With surface=True every frame is drawn as its mesh (PointRenderer.add_mesh, max_bbox_px) instead of its points: a solid
    surface where the point splat leaves a dot screen.
    There is no mp4 output (the reference's save_video): imageio and ffmpeg are not available."""
    pts_all, images_all = _dev(pts_all, "render_frames: pts_all"), _dev(images_all, "render_frames: images_all")
    t = pts_all.shape[0]
    if pts_all.dim() != 4 or pts_all.shape[-1] != 3 or images_all.shape != pts_all.shape:
        raise RuntimeError("render_frames: pts_all %s and images_all %s must both be [t, h, w, 3]" % (tuple(pts_all.shape), tuple(images_all.shape)))
    if mask is not None and conf_all is not None:
        raise RuntimeError("render_frames: give mask or conf_all, not both")
    if mask is not None and _dev(mask, "render_frames: mask").shape != pts_all.shape[:3]:
        raise RuntimeError("render_frames: mask %s does not match pts_all %s" % (tuple(mask.shape), tuple(pts_all.shape)))
    if conf_all is not None and (_dev(conf_all, "render_frames: conf_all").shape != pts_all.shape[:3] or conf_thresh is None):
        raise RuntimeError("render_frames: conf_all must be [t, h, w] and come with conf_thresh")
    r = PointRenderer(camera=camera, point_size=point_size, background=background, conf_thresh=conf_thresh if conf_all is not None else None,
                      dynamic=dynamic, device=pts_all.device)
    out = torch.empty((t, r.height, r.width, 3), dtype=torch.uint8, device=pts_all.device)
    for i in range(t):
        if surface:
            r.add_mesh(pts_all[i], images_all[i], None if conf_all is None else conf_all[i], None if mask is None else mask[i], max_bbox_px)
        elif mask is not None:
            m = mask[i].reshape(-1)
            r.add(pts_all[i].reshape(-1, 3)[m], images_all[i].reshape(-1, 3)[m])
        else:
            r.add(pts_all[i], images_all[i], None if conf_all is None else conf_all[i])
        out[i] = r.image()
    if output_dir is not None:
        d = os.path.join(output_dir, "render_frames")
        os.makedirs(d, exist_ok=True)
        if save_camera:
            _save_camera(os.path.join(d, "camera.json"), camera)
        host = out.cpu().numpy()
        for i in range(t):
            _save_png(os.path.join(d, "frame_%03d.png" % i), host[i])
    return out


# ------------------------------------------------------------------------------------------------ pointmap / confidence images
_JET = {"red": ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
        "green": ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
        "blue": ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0))}


def jet_lut():
    """The 256-entry table of matplotlib's `jet` as (rgba * 255).astype(uint8) [256, 4], from its segment data by the linear
    interpolation of LinearSegmentedColormap (float64, the same order of operations)."""
    n = 256
    lut = np.ones((n, 4), np.float64)
    xind = np.linspace(0, 1, n)
    for ch, name in enumerate(("red", "green", "blue")):
        adata = np.array(_JET[name], np.float64)
        x, y0, y1 = adata[:, 0], adata[:, 1], adata[:, 2]
        xs = x * (n - 1)
        xi = xind * (n - 1)
        ind = np.searchsorted(xs, xi)[1:-1]
        distance = (xi[1:-1] - xs[ind - 1]) / (xs[ind] - xs[ind - 1])
        lut[:, ch] = np.clip(np.concatenate([[y1[0]], distance * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]]), 0, 1)
    return (lut * 255).astype(np.uint8)


def colorize_hsv(x):
    """uint8 [..., 3] = trunc(255 * hsv_to_rgb(1 - x)) of x fp32 [..., 3] in [0, 1] (vis.py:168-169)"""
    x = _dev(x, "colorize_hsv: x").float().contiguous()
    if x.shape[-1] != 3:
        raise RuntimeError("colorize_hsv: x %s must end in 3" % (tuple(x.shape),))
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    L.check(L.load().sp3_colorize_hsv(x.data_ptr(), x.numel() // 3, out.data_ptr(), L.stream_ptr()), "sp3_colorize_hsv")
    return out


def colorize_lut(x, lut):
    """uint8 [..., 4] = lut[clamp(trunc(x * 256), 0, 255)] of x fp32 [...], lut uint8 [256, 4] on the device (plt.cm.jet(x) for x in
    [0, 1], vis.py:188-189; a NaN takes entry 0)"""
    x, lut = _dev(x, "colorize_lut: x").float().contiguous(), _dev(lut, "colorize_lut: lut")
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 4) or not lut.is_contiguous():
        raise RuntimeError("colorize_lut: lut must be a contiguous uint8 [256, 4] tensor")
    out = torch.empty(x.shape + (4,), dtype=torch.uint8, device=x.device)
    L.check(L.load().sp3_colorize_lut(x.data_ptr(), x.numel(), lut.data_ptr(), out.data_ptr(), L.stream_ptr()), "sp3_colorize_lut")
    return out


def vis_pred_and_imgs(pts_all, save_path, images_all=None, conf_all=None):
    """vis.py:135-201 without the videos: the pointmaps [t, h, w, 3], normalised per coordinate over all frames and pixels, as hue
    images save_path/pts/pts_%04d.png; images_all (floats in [0, 1]) as imgs/img_%04d.png; conf_all [t, h, w] in [0, 1] through the
    jet table as confs/conf_%04d.png (RGBA).  Returns the uint8 device tensors {"pts", "imgs", "confs"} that were written."""
    pts_all = _dev(pts_all, "vis_pred_and_imgs: pts_all").float()
    if pts_all.dim() != 4 or pts_all.shape[-1] != 3:
        raise RuntimeError("vis_pred_and_imgs: pts_all %s must be [t, h, w, 3]" % (tuple(pts_all.shape),))
    lo, hi = torch.amin(pts_all, dim=(0, 1, 2), keepdim=True), torch.amax(pts_all, dim=(0, 1, 2), keepdim=True)
    out = {"pts": colorize_hsv((pts_all - lo) / (hi - lo))}
    if images_all is not None:
        out["imgs"] = (_dev(images_all, "vis_pred_and_imgs: images_all").float() * 255).to(torch.uint8)      # (image * 255).astype(np.uint8)
    if conf_all is not None:
        lut = torch.from_numpy(jet_lut()).to(pts_all.device)
        out["confs"] = colorize_lut(_dev(conf_all, "vis_pred_and_imgs: conf_all"), lut)
    for key, folder, stem in (("pts", "pts", "pts"), ("imgs", "imgs", "img"), ("confs", "confs", "conf")):
        if key in out:
            d = os.path.join(save_path, folder)
            os.makedirs(d, exist_ok=True)
            host = out[key].cpu().numpy()
            for i in range(host.shape[0]):
                _save_png(os.path.join(d, "%s_%04d.png" % (stem, i)), host[i])
    return out
