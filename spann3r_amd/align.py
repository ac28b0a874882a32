"""Global alignment of DUSt3R pair graphs on the device: one set of camera poses, focals and depth maps that explains all pairs.

`runner.pair_graph` gives, for every ordered pair (i, j), two pointmaps in i's camera frame and two confidences.  GlobalAligner takes
that dict where DUSt3R users call dust3r.cloud_opt.global_aligner(...).compute_global_alignment(init="mst"): it keeps that optimiser's
parametrisation (pairwise poses with a log scale, image poses, log focals, log depth maps) in plain differentiable torch on the
device and evaluates the loss -- the confidence-weighted distance between the E moved pairwise pointmaps and the N unprojected depth
maps -- with ALL its gradients in one launch (sp3_align_loss_grad, csrc/align.hip; rules in include/spann3r_hip.h "Global
alignment"): nothing per edge is stored for backward.  AlignLoss is the autograd function around that launch.  The spanning-tree
initialisation registers point sets through sp3_align_moments (17 fp64 sums per registration) and a weighted Umeyama solve in fp64
on the host.

What is unpinned: dust3r.cloud_opt cannot be imported here, roma and cv2 are absent.  The anchors are tests/align_ref.py -- the
header's rule in numpy, which the kernel is checked against -- and a float64 torch statement of the reference's formulas from the
parametrisation down.  init="mst" uses this repository's estimate_poses, not cv2.solvePnPRansac; the rigid registration is its own
Umeyama with the reflection fixed, not roma's; a focal estimate is held to acceptable_focal_range (0.5 .. 3.5 of the 60 degree
focal), which the reference computes but does not apply; init="known_poses" takes the pairwise scale from the baseline between the
two known centres, not from align_multiple_poses; the spanning tree is plain Kruskal with ties broken by edge index, grown from the
strongest edge in descending score order.  torch provides memory and the small parameter maps; without `backend` there is no CPU path."""
import copy
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from . import lib as L

_IMG_DT = np.dtype([("depth", "u8"), ("grad_depth", "u8"), ("row_stride", "i8"), ("w", "i4"), ("h", "i4"), ("f", "f4"), ("cx", "f4"),
                    ("cy", "f4"), ("c2w", "f4", 12)], align=True)
_EDGE_DT = np.dtype([("pts", "u8", 2), ("weight", "u8", 2), ("row_stride", "i8", 2), ("img", "i4", 2), ("M", "f4", 12), ("a", "f4", 3)],
                    align=True)
_TRIPLE_DT = np.dtype([("src", "u8"), ("dst", "u8"), ("w", "u8"), ("n", "i8")], align=True)
assert _IMG_DT.itemsize == ctypes.sizeof(L.AlignImage) and _EDGE_DT.itemsize == ctypes.sizeof(L.AlignEdge)
assert _TRIPLE_DT.itemsize == ctypes.sizeof(L.AlignTriple)


# ------------------------------------------------------------------------------------------------ host helpers
def make_items(n_imgs, ij):
    """CSR of the items (edge, side) per image: edges in order, side 0 before side 1 -> item_first [N + 1], item_edge, item_side (int32).
    One pass over the edges: a stable sort of the 2 E (edge, side) pairs by their image."""
    img = np.asarray(ij, np.int64).reshape(-1, 2).reshape(-1)      # item 2 e + s belongs to image ij[e][s]
    order = np.argsort(img, kind="stable")
    first = np.zeros(n_imgs + 1, np.int64)
    np.cumsum(np.bincount(img, minlength=n_imgs)[:n_imgs], out=first[1:])
    return first.astype(np.int32), (order // 2).astype(np.int32), (order % 2).astype(np.int32)


def maximum_spanning_tree(n_imgs, ij, scores):
    """Kruskal over the E scored edges (direction ignored), strongest first, ties broken by edge index -> the edge indices of the
    tree (a forest if the graph is not connected), in the order they were taken"""
    parent = list(range(n_imgs))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    tree = []
    for e in sorted(range(len(ij)), key=lambda e: (-float(scores[e]), e)):
        a, b = find(ij[e][0]), find(ij[e][1])
        if a != b:
            parent[a] = b
            tree.append(e)
    return tree


def umeyama_from_moments(m):
    """the 17 sums of sp3_align_moments -> (s, R [3, 3], T [3]) with dst ~ s R src + T, float64: weighted Umeyama, the reflection
    fixed (det R = +1); the 3 x 3 SVD goes through torch.linalg on the CPU"""
    m = np.asarray(m, np.float64)
    sw = m[0]
    mp, mq = m[1:4] / sw, m[4:7] / sw
    H = m[7:16].reshape(3, 3) / sw - np.outer(mp, mq)
    var_p = m[16] / sw - mp @ mp
    U, D, Vh = (x.numpy() for x in torch.linalg.svd(torch.from_numpy(H)))
    sign = 1.0 if np.linalg.det(Vh.T @ U.T) >= 0 else -1.0
    J = np.array([1.0, 1.0, sign])
    R = (Vh.T * J) @ U.T
    s = float((D * J).sum() / var_p)
    return s, R, mq - s * R @ mp


def rotmat_to_quat(R):
    """rotation matrix -> unit quaternion (x, y, z, w), float64"""
    R = np.asarray(R, np.float64)
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(max(R[i, i] - R[j, j] - R[k, k] + 1.0, 0.0)) * 2
        q = [0.0, 0.0, 0.0, (R[k, j] - R[j, k]) / s]
        q[i], q[j], q[k] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    q = np.array(q)
    return q / np.linalg.norm(q)


def quat_to_rotmat(q):
    """quaternions (x, y, z, w) [..., 4], normalised here -> rotation matrices [..., 3, 3] (differentiable torch)"""
    q = q / q.norm(dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def signed_log1p(x):
    return torch.sign(x) * torch.log1p(torch.abs(x))


def signed_expm1(x):
    return torch.sign(x) * torch.expm1(torch.abs(x))


def cosine_schedule(t, lr_start, lr_end):
    return lr_end + (lr_start - lr_end) * (1 + math.cos(t * math.pi)) / 2


def linear_schedule(t, lr_start, lr_end):
    return lr_start + (lr_end - lr_start) * t


def acceptable_focal_range(H, W, minf=0.5, maxf=3.5):
    base = max(H, W) / (2 * math.tan(math.radians(60) / 2))
    return minf * base, maxf * base


def conf_transform(mode):
    if mode == "log":
        return torch.log
    if mode == "sqrt":
        return torch.sqrt
    if mode == "m1":
        return lambda x: x - 1
    if mode in ("id", "none"):
        return lambda x: x
    raise ValueError("conf must be one of log, sqrt, m1, id, none; got %r" % (mode,))


# ------------------------------------------------------------------------------------------------ the problem and the device backend
class AlignProblem:
    """What does not change over the optimisation: the edges (i, j), the image shapes, the per-edge pointmaps P[side][e] fp32
    [h, w, 3] and weights W[side][e] fp32 [h, w] (contiguous, on `device`), the CSR item tables and the offsets of the images in the
    flat depth vector."""

    def __init__(self, ij, shapes, P, W, device):
        self.ij = [(int(i), int(j)) for i, j in ij]
        self.shapes = [(int(h), int(w)) for h, w in shapes]
        self.N, self.E = len(self.shapes), len(self.ij)
        if self.E == 0:
            raise ValueError("AlignProblem: no edges")
        for e, pair in enumerate(self.ij):
            for s in (0, 1):
                if not 0 <= pair[s] < self.N:
                    raise ValueError("AlignProblem: edge %d: image index %d outside 0..%d" % (e, pair[s], self.N - 1))
                h, w = self.shapes[pair[s]]
                if tuple(P[s][e].shape) != (h, w, 3) or tuple(W[s][e].shape) != (h, w):
                    raise ValueError("AlignProblem: edge %d side %d: pointmap %s / weight %s do not match image %d (%d x %d)"
                                     % (e, s, tuple(P[s][e].shape), tuple(W[s][e].shape), pair[s], h, w))
        if min(min(s) for s in self.shapes) < 1:
            raise ValueError("AlignProblem: an image without pixels")
        self.device = torch.device(device)
        self.P = [[p.to(self.device, torch.float32).contiguous() for p in P[s]] for s in (0, 1)]
        self.W = [[w.to(self.device, torch.float32).contiguous() for w in W[s]] for s in (0, 1)]
        sizes = [h * w for h, w in self.shapes]
        self.offsets = [0] + list(np.cumsum(sizes)[:-1])
        self.total = int(sum(sizes))
        self.items = make_items(self.N, self.ij)
        self.areas = [float(sum(sizes[p[s]] for p in self.ij)) for s in (0, 1)]
        self._tables = None


class DeviceBackend:
    """sp3_align_loss_grad / sp3_align_moments and the repository's focal and PnP estimators."""

    def _static(self, pb):
        if pb._tables is None:
            imgs, edges = np.zeros(pb.N, _IMG_DT), np.zeros(pb.E, _EDGE_DT)
            for n, (h, w) in enumerate(pb.shapes):
                imgs[n]["row_stride"], imgs[n]["w"], imgs[n]["h"] = w, w, h
            for e, pair in enumerate(pb.ij):
                for s in (0, 1):
                    edges[e]["pts"][s], edges[e]["weight"][s] = pb.P[s][e].data_ptr(), pb.W[s][e].data_ptr()
                    edges[e]["row_stride"][s], edges[e]["img"][s] = pb.shapes[pair[s]][1], pair[s]
            items_d = [torch.from_numpy(t).to(pb.device) for t in pb.items]
            hmax, wmax = max(h for h, _ in pb.shapes), max(w for _, w in pb.shapes)
            ws = torch.empty(L.load().sp3_align_loss_grad_ws_bytes(pb.N, pb.E, wmax, hmax) // 8, dtype=torch.float64, device=pb.device)
            pb._tables = (imgs, edges, items_d, ws)
        return pb._tables

    def tables(self, pb, depth, C, f, pp, M, a):
        """the descriptor tables of one evaluation, on the host and on the device, and its output buffers.  The small parameters come to
        the host here (one synchronising copy): the entry point checks them there before it launches."""
        if not depth.is_cuda:
            raise RuntimeError("AlignLoss runs on the GPU (HIP kernel); there is no CPU path")
        imgs, edges, items_d, ws = self._static(pb)
        depth = depth.contiguous()
        small = torch.cat((C.reshape(-1), f.reshape(-1), pp.reshape(-1), M.reshape(-1), a.reshape(-1))).detach().float().cpu().numpy()
        N, E, dev = pb.N, pb.E, pb.device
        o = np.cumsum([0, 12 * N, N, 2 * N, 12 * E, 3 * E])
        ppn = small[o[2]:o[3]].reshape(N, 2)
        gd = torch.empty_like(depth)
        off = np.asarray(pb.offsets, np.uint64) * np.uint64(4)
        imgs["depth"], imgs["grad_depth"] = np.uint64(depth.data_ptr()) + off, np.uint64(gd.data_ptr()) + off
        imgs["c2w"], imgs["f"], imgs["cx"], imgs["cy"] = small[o[0]:o[1]].reshape(N, 12), small[o[1]:o[2]], ppn[:, 0], ppn[:, 1]
        edges["M"], edges["a"] = small[o[3]:o[4]].reshape(E, 12), small[o[4]:o[5]].reshape(E, 3)
        return dict(depth=depth, gd=gd, imgs=imgs, edges=edges, items_d=items_d, ws=ws,
                    imgs_d=torch.from_numpy(imgs.view(np.uint8).copy()).to(dev), edges_d=torch.from_numpy(edges.view(np.uint8).copy()).to(dev),
                    img_sums=torch.empty(N, 15, dtype=torch.float64, device=dev), edge_sums=torch.empty(E, 15, dtype=torch.float64, device=dev),
                    loss3=torch.empty(3, dtype=torch.float64, device=dev))

    def launch(self, pb, t):
        """sp3_align_loss_grad on prepared tables (the loss launch and its finishing launch; nothing synchronises)"""
        i32p = ctypes.POINTER(ctypes.c_int32)
        L.check(L.load().sp3_align_loss_grad(ctypes.cast(t["imgs"].ctypes.data, ctypes.POINTER(L.AlignImage)), t["imgs_d"].data_ptr(), pb.N,
                                             ctypes.cast(t["edges"].ctypes.data, ctypes.POINTER(L.AlignEdge)), t["edges_d"].data_ptr(), pb.E,
                                             pb.items[0].ctypes.data_as(i32p), pb.items[1].ctypes.data_as(i32p), pb.items[2].ctypes.data_as(i32p),
                                             t["items_d"][0].data_ptr(), t["items_d"][1].data_ptr(), t["items_d"][2].data_ptr(), t["ws"].data_ptr(),
                                             t["img_sums"].data_ptr(), t["edge_sums"].data_ptr(), t["loss3"].data_ptr(), L.stream_ptr()),
                "sp3_align_loss_grad")

    def loss_grad(self, pb, depth, C, f, pp, M, a):
        t = self.tables(pb, depth, C, f, pp, M, a)
        self.launch(pb, t)
        return t["loss3"], t["gd"], t["img_sums"], t["edge_sums"]

    def moments(self, triples):
        """list of (src [.., 3], dst [.., 3], w [..]) device tensors -> the 17 sums of each, float64 [B, 17] on the host (one launch)"""
        B = len(triples)
        if B == 0:
            raise ValueError("align moments: no triples")
        tab = np.zeros(B, _TRIPLE_DT)
        keep = []
        for b, (s, d, w) in enumerate(triples):
            if not (s.is_cuda and d.is_cuda and w.is_cuda):
                raise RuntimeError("align moments run on the GPU (HIP kernel); there is no CPU path")
            s, d, w = s.float().contiguous(), d.float().contiguous(), w.float().contiguous()
            if s.numel() != 3 * w.numel() or d.numel() != 3 * w.numel() or w.numel() == 0:
                raise ValueError("align moments: triple %d: sizes %s, %s, %s do not match" % (b, tuple(s.shape), tuple(d.shape), tuple(w.shape)))
            keep.append((s, d, w))
            tab[b] = (s.data_ptr(), d.data_ptr(), w.data_ptr(), w.numel())
        dev = keep[0][0].device
        lib = L.load()
        ws = torch.empty(lib.sp3_align_moments_ws_bytes(B, int(tab["n"].max())) // 8, dtype=torch.float64, device=dev)
        out = torch.empty(B, 17, dtype=torch.float64, device=dev)
        tab_d = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
        L.check(lib.sp3_align_moments(ctypes.cast(tab.ctypes.data, ctypes.POINTER(L.AlignTriple)), tab_d.data_ptr(), B, ws.data_ptr(),
                                      out.data_ptr(), L.stream_ptr()), "sp3_align_moments")
        return out.cpu()

    def focal(self, pts, pp):
        from .postprocess import estimate_focal_knowing_depth
        return float(estimate_focal_knowing_depth(pts[None], pp, focal_mode="weiszfeld", min_focal=0.5, max_focal=3.5).item())

    def pose(self, pts, focal, pp):
        from .postprocess import estimate_poses
        return estimate_poses(pts[None], focal, pp)[0][0]


class AlignLoss(torch.autograd.Function):
    """L(depth [sum h w], C [N, 12], f [N], pp [N, 2], M [E, 12], a [E, 3]) of an AlignProblem: forward makes the one launch that
    returns the loss and every gradient; backward hands the stored gradients back, scaled by the incoming one."""

    @staticmethod
    def forward(ctx, depth, C, f, pp, M, a, problem, backend):
        loss3, gd, img_sums, edge_sums = backend.loss_grad(problem, depth.detach(), C.detach(), f.detach(), pp.detach(), M.detach(), a.detach())
        ctx.save_for_backward(gd, img_sums, edge_sums)
        ctx.sums = loss3
        return loss3[2].to(device=depth.device, dtype=depth.dtype)

    @staticmethod
    def backward(ctx, go):
        gd, img, edge = ctx.saved_tensors
        dt, dev = gd.dtype, go.device
        img, edge = img.to(dev), edge.to(dev)
        return (go * gd.to(dev), (go * img[:, :12]).to(dt), (go * img[:, 12]).to(dt), (go * img[:, 13:15]).to(dt), (go * edge[:, :12]).to(dt),
                (go * edge[:, 12:15]).to(dt), None, None)


# ------------------------------------------------------------------------------------------------ the aligner
class GlobalAligner(nn.Module):
    """PointCloudOptimizer of dust3r/cloud_opt/optimizer.py over the dict of runner.pair_graph (dist "l1"), see the module docstring.
    backend: None = the device kernels (the parameters live on `device`, default "cuda"); the tests pass their CPU restatement."""

    def __init__(self, pairs, conf="log", min_conf_thr=3, base_scale=0.5, pw_break=20, focal_break=20, allow_pw_adaptors=False,
                 optimize_pp=False, seed=0, device=None, backend=None):
        super().__init__()
        self.backend = DeviceBackend() if backend is None else backend
        device = torch.device(device if device is not None else ("cuda" if backend is None else "cpu"))
        try:
            idx1, idx2 = pairs["view1"]["idx"], pairs["view2"]["idx"]
            P = [list(pairs["pred1"]["pts3d"]), list(pairs["pred2"]["pts3d_in_other_view"])]
            cf = [list(pairs["pred1"]["conf"]), list(pairs["pred2"]["conf"])]
        except (KeyError, TypeError) as e:
            raise ValueError("GlobalAligner: pairs must be the dict of runner.pair_graph (%s)" % (e,))
        ij = [(int(i), int(j)) for i, j in zip(idx1, idx2)]
        if len(ij) == 0:
            raise ValueError("GlobalAligner: the pair graph has no edges (E = 0)")
        if not (len(P[0]) == len(P[1]) == len(cf[0]) == len(cf[1]) == len(ij)):
            raise ValueError("GlobalAligner: %d edges but %d / %d pointmaps and %d / %d confidences" % (len(ij), len(P[0]), len(P[1]), len(cf[0]), len(cf[1])))
        ids = sorted({n for pair in ij for n in pair})
        if ids != list(range(len(ids))):
            raise ValueError("GlobalAligner: bad pair indices: the images must be numbered 0..N-1 without gaps, got %s" % (ids,))
        shapes = [None] * len(ids)
        for e, pair in enumerate(ij):
            for s in (0, 1):
                shp = tuple(P[s][e].shape[:2])
                if shapes[pair[s]] not in (None, shp):
                    raise ValueError("GlobalAligner: image %d has shape %s in edge %d and %s before" % (pair[s], shp, e, shapes[pair[s]]))
                shapes[pair[s]] = shp
        self.conf_trf = conf_transform(conf)
        self.min_conf_thr, self.base_scale, self.pw_break, self.focal_break = min_conf_thr, base_scale, pw_break, focal_break
        self.norm_pw_scale = True
        self.edges, self.imshapes, self.n_imgs, self.n_edges = ij, shapes, len(shapes), len(ij)
        self.is_symmetrized = set(ij) == {(j, i) for i, j in ij}
        self.conf_i = [c.to(device, torch.float32) for c in cf[0]]
        self.conf_j = [c.to(device, torch.float32) for c in cf[1]]
        self.problem = AlignProblem(ij, shapes, P, [[self.conf_trf(c) for c in self.conf_i], [self.conf_trf(c) for c in self.conf_j]], device)
        self.im_conf = [torch.zeros(s, device=device) for s in shapes]
        for e, (i, j) in enumerate(ij):      # the running maximum over the edges
            self.im_conf[i] = torch.maximum(self.im_conf[i], self.conf_i[e])
            self.im_conf[j] = torch.maximum(self.im_conf[j], self.conf_j[e])
        g = torch.Generator().manual_seed(int(seed))      # drawn on the host: the same start on every device
        rnd = lambda *s: torch.randn(*s, generator=g)
        self.pw_poses = nn.Parameter(rnd(self.n_edges, 8).to(device))
        self.pw_adaptors = nn.Parameter(torch.zeros(self.n_edges, 2, device=device), requires_grad=bool(allow_pw_adaptors))
        self.im_depthmaps = nn.Parameter((rnd(self.problem.total) / 10 - 3).to(device))      # log depth, the images one after another
        self.im_poses = nn.Parameter(rnd(self.n_imgs, 7).to(device))
        self.im_focals = nn.Parameter(torch.tensor([[focal_break * math.log(max(h, w))] for h, w in shapes], dtype=torch.float32, device=device))
        self.im_pp = nn.Parameter(torch.zeros(self.n_imgs, 2, device=device), requires_grad=bool(optimize_pp))
        self.register_buffer("_pp", torch.tensor([(w / 2, h / 2) for h, w in shapes], dtype=torch.float32, device=device))

    @property
    def device(self):
        return self.pw_poses.device

    # ---- the parameter maps (plain torch)
    def _get_poses(self, poses):
        R, T = quat_to_rotmat(poses[:, :4]), signed_expm1(poses[:, 4:7])
        bottom = torch.zeros(len(poses), 1, 4, device=poses.device, dtype=poses.dtype)
        bottom[:, 0, 3] = 1
        return torch.cat((torch.cat((R, T[:, :, None]), 2), bottom), 1)

    def get_pw_norm_scale_factor(self):
        if self.norm_pw_scale:      # exp(scale) ~ base_scale on average
            return (math.log(self.base_scale) - self.pw_poses[:, -1].mean()).exp()
        return 1

    def get_pw_scale(self):
        return self.pw_poses[:, -1].exp() * self.get_pw_norm_scale_factor()

    def get_pw_poses(self):
        RT = self._get_poses(self.pw_poses)
        return torch.cat((RT[:, :3] * self.get_pw_scale().view(-1, 1, 1), RT[:, 3:]), 1)

    def get_adaptors(self):
        ad = torch.cat((self.pw_adaptors[:, 0:1], self.pw_adaptors), -1)      # (xy, xy, z)
        if self.norm_pw_scale:
            ad = ad - ad.mean(1, keepdim=True)
        return (ad / self.pw_break).exp()

    def get_im_poses(self):
        return self._get_poses(self.im_poses)

    def get_focals(self):
        return (self.im_focals / self.focal_break).exp()

    def get_known_focal_mask(self):
        return torch.full((self.n_imgs,), not self.im_focals.requires_grad)

    def get_principal_points(self):
        return self._pp + 10 * self.im_pp

    def get_intrinsics(self):
        K = torch.zeros(self.n_imgs, 3, 3, device=self.device)
        K[:, 0, 0] = K[:, 1, 1] = self.get_focals().flatten()
        K[:, :2, 2] = self.get_principal_points()
        K[:, 2, 2] = 1
        return K

    def _split(self, flat, tail=()):
        pb = self.problem
        return [flat[o:o + h * w].view((h, w) + tail) for o, (h, w) in zip(pb.offsets, pb.shapes)]

    def get_depthmaps(self):
        return self._split(self.im_depthmaps.exp())

    def get_pts3d(self):
        """the world pointmaps of the current parameters, a list of [h, w, 3] (plain torch, the reference's depth_to_pts3d)"""
        f, pp, poses, out = self.get_focals().flatten(), self.get_principal_points(), self.get_im_poses(), []
        for n, d in enumerate(self.get_depthmaps()):
            h, w = d.shape
            u = torch.arange(w, device=d.device, dtype=d.dtype)[None, :]
            v = torch.arange(h, device=d.device, dtype=d.dtype)[:, None]
            cam = torch.stack((d * (u - pp[n, 0]) / f[n], d * (v - pp[n, 1]) / f[n], d), -1)
            out.append(cam @ poses[n, :3, :3].T + poses[n, :3, 3])
        return out

    def get_masks(self):
        return [c > self.min_conf_thr for c in self.im_conf]

    def get_conf(self, mode=None):
        trf = self.conf_trf if mode is None else conf_transform(mode)
        return [trf(c) for c in self.im_conf]

    # ---- presets
    def _indices(self, msk):
        if msk is None:
            return list(range(self.n_imgs))
        if isinstance(msk, int):
            return [msk]
        msk = np.asarray(msk)
        return list(np.where(msk)[0]) if msk.dtype == bool else [int(x) for x in msk]

    def _all_selected(self, msk):
        if self._indices(msk) != list(range(self.n_imgs)):
            raise ValueError("GlobalAligner: a preset must cover every image (incomplete mask)")

    @torch.no_grad()
    def _set_pose(self, poses, idx, R, T=None, scale=None, force=False):
        if not (poses.requires_grad or force):
            return
        R = np.asarray(R.detach().cpu() if isinstance(R, torch.Tensor) else R, np.float64)
        if R.shape == (4, 4):
            R, T = R[:3, :3], R[:3, 3]
        poses.data[idx, 0:4] = torch.from_numpy(rotmat_to_quat(R)).to(poses)
        if T is not None:
            T = torch.as_tensor(np.asarray(T.detach().cpu() if isinstance(T, torch.Tensor) else T, np.float64) / (scale or 1))
            poses.data[idx, 4:7] = signed_log1p(T).to(poses)      # the translation is a function of the scale
        if scale is not None:
            poses.data[idx, -1] = math.log(float(scale))

    def preset_pose(self, known_poses, pose_msk=None):
        """cam-to-world poses for every image: they are set, frozen (im_poses.requires_grad False) and norm_pw_scale goes off"""
        self._all_selected(pose_msk)
        if isinstance(known_poses, torch.Tensor) and known_poses.ndim == 2:
            known_poses = [known_poses]
        for idx, pose in zip(self._indices(pose_msk), known_poses):
            self._set_pose(self.im_poses, idx, pose)
        self.im_poses.requires_grad_(False)
        self.norm_pw_scale = False

    @torch.no_grad()
    def _set_focal(self, idx, focal, force=False):
        if self.im_focals.requires_grad or force:
            self.im_focals.data[idx] = self.focal_break * math.log(float(focal))

    def preset_focal(self, known_focals, msk=None):
        self._all_selected(msk)
        for idx, focal in zip(self._indices(msk), known_focals):
            self._set_focal(idx, focal)
        self.im_focals.requires_grad_(False)

    def preset_principal_point(self, known_pp, msk=None):
        self._all_selected(msk)
        with torch.no_grad():
            for idx, pp in zip(self._indices(msk), known_pp):
                h, w = self.imshapes[idx]
                self.im_pp.data[idx] = torch.as_tensor([(float(pp[0]) - w / 2) / 10, (float(pp[1]) - h / 2) / 10]).to(self.im_pp)
        self.im_pp.requires_grad_(False)

    @torch.no_grad()
    def _set_depthmap(self, idx, depth, force=False):
        if self.im_depthmaps.requires_grad or force:
            o, (h, w) = self.problem.offsets[idx], self.imshapes[idx]
            self.im_depthmaps.data[o:o + h * w] = depth.reshape(-1).log().nan_to_num(neginf=0).to(self.im_depthmaps)

    # ---- the loss
    def geometric_parameters(self):
        """(depth [sum h w], C [N, 12], f [N], pp [N, 2], M [E, 12], a [E, 3]): what the kernel sees, differentiable torch"""
        return (self.im_depthmaps.exp(), self.get_im_poses()[:, :3].reshape(-1, 12), self.get_focals().flatten(), self.get_principal_points(),
                self.get_pw_poses()[:, :3].reshape(-1, 12), self.get_adaptors())

    def forward(self):
        return AlignLoss.apply(*self.geometric_parameters(), self.problem, self.backend)

    def clean_pointcloud(self, tol=0.001, max_bad_conf=0):
        """a shallow copy of this aligner (the parameters are shared) whose im_conf went through multiview.clean_confidence in the
        sequence order: a pixel that floats in front of what a more confident image measured is clipped to max_bad_conf"""
        from .multiview import clean_confidence
        with torch.no_grad():
            pts = [p.contiguous() for p in self.get_pts3d()]
            K = self.get_intrinsics().double().cpu().numpy()
            c2w = self.get_im_poses().double().cpu().numpy()
            conf = clean_confidence(pts, [c.contiguous() for c in self.im_conf], K, c2w, tol=tol, max_bad_conf=max_bad_conf, order="sequence")
        res = copy.copy(self)
        res.im_conf = list(conf)
        return res

    # ---- initialisation
    def edge_scores(self):
        return [float(a.mean() * b.mean()) for a, b in zip(self.conf_i, self.conf_j)]

    def get_mst_tree(self):
        """the edge indices of the maximum spanning tree over mean(conf_i) * mean(conf_j)"""
        return maximum_spanning_tree(self.n_imgs, self.edges, self.edge_scores())

    def _register(self, triples):
        return [umeyama_from_moments(m) for m in self.backend.moments(triples).numpy()]

    def _trf(self, s, R, T):
        M = torch.eye(4, dtype=torch.float64)
        M[:3, :3], M[:3, 3] = torch.from_numpy(R * s), torch.from_numpy(T)
        return M.to(self.device, torch.float32)

    @torch.no_grad()
    def init_minimum_spanning_tree(self, niter_PnP=10):
        """init_im_poses.py:67-225 in this repository's terms (see the module docstring for what differs) -> the tree's edge indices"""
        if not self.im_poses.requires_grad:
            raise NotImplementedError("init='mst' with preset poses: use init='known_poses'")
        pb, scores = self.problem, self.edge_scores()
        tree = self.get_mst_tree()
        geo = lambda M, p: p @ M[:3, :3].T + M[:3, 3]
        pts3d, im_poses, im_focals = [None] * self.n_imgs, [None] * self.n_imgs, [None] * self.n_imgs
        pp_of = lambda n: (self.imshapes[n][1] / 2, self.imshapes[n][0] / 2)
        todo = sorted(tree, key=lambda e: (-scores[e], e))
        e0 = todo.pop(0)
        i, j = self.edges[e0]
        pts3d[i], pts3d[j] = pb.P[0][e0].clone(), pb.P[1][e0].clone()
        im_poses[i] = torch.eye(4, device=self.device)
        im_focals[i] = self.backend.focal(pb.P[0][e0], pp_of(i))
        done, order = {i, j}, [e0]
        while todo:
            for k, e in enumerate(todo):      # the strongest edge that touches what is placed
                if self.edges[e][0] in done or self.edges[e][1] in done:
                    break
            else:
                break                          # a disconnected graph: the rest keeps its random start
            todo.pop(k)
            i, j = self.edges[e]
            known, new, side = (i, j, 0) if i in done else (j, i, 1)
            s, R, T = self._register([(pb.P[side][e], pts3d[known], (self.conf_i, self.conf_j)[side][e])])[0]
            pts3d[new] = geo(self._trf(s, R, T), pb.P[1 - side][e])
            done.add(new)
            order.append(e)
            if im_poses[i] is None:            # both cases give image i's camera: the pair lives in i's frame
                im_poses[i] = self._trf(1.0, R, T)
        for e in sorted(range(self.n_edges), key=lambda e: (-scores[e], e)):
            i = self.edges[e][0]
            if im_focals[i] is None:
                im_focals[i] = self.backend.focal(pb.P[0][e], pp_of(i))
        for n in range(self.n_imgs):
            if pts3d[n] is None:
                continue
            if im_poses[n] is None:
                msk = self.im_conf[n] > self.min_conf_thr
                if int(msk.sum()) >= 6:
                    focal = im_focals[n] if im_focals[n] is not None else float(self.get_focals()[n])
                    p = torch.where(msk[..., None], pts3d[n], torch.full_like(pts3d[n], float("nan")))
                    im_poses[n] = torch.as_tensor(np.asarray(self.backend.pose(p, focal, pp_of(n))), dtype=torch.float32, device=self.device)
            if im_poses[n] is None:
                im_poses[n] = torch.eye(4, device=self.device)
        self._init_from_pts3d(pts3d, im_focals, im_poses)
        return order

    @torch.no_grad()
    def _init_from_pts3d(self, pts3d, im_focals, im_poses):
        pb = self.problem
        todo = [e for e, (i, j) in enumerate(self.edges) if pts3d[i] is not None]
        regs = self._register([(pb.P[0][e], pts3d[self.edges[e][0]], self.conf_i[e]) for e in todo])      # ONE launch for all edges
        for e, (s, R, T) in zip(todo, regs):
            self._set_pose(self.pw_poses, e, R, T, scale=s)
        s_factor = float(self.get_pw_norm_scale_factor())
        for n in range(self.n_imgs):
            if pts3d[n] is None:
                continue
            c2w = im_poses[n].detach().double().cpu()      # (4 x 4: inverted on the host)
            c2w[:3, 3] *= s_factor
            p = pts3d[n].double() * s_factor
            w2c = torch.linalg.inv(c2w).to(p.device)
            depth = (p @ w2c[:3, :3].T + w2c[:3, 3])[..., 2]
            self._set_depthmap(n, depth)
            self._set_pose(self.im_poses, n, c2w)
            if im_focals[n] is not None:
                self._set_focal(n, im_focals[n])

    @torch.no_grad()
    def init_from_known_poses(self, niter_PnP=10):
        """init_im_poses.py:24-63: every pose and focal is preset; the pairwise similarity of edge e takes the pair's frame (camera i)
        onto the known pose of i, its scale from the distance between the two known centres over the PnP estimate of j in the pair's
        frame; the depth of an image comes from its most confident edge, times that scale."""
        if self.im_poses.requires_grad or self.im_focals.requires_grad:
            raise ValueError("init='known_poses' needs preset_pose and preset_focal for every image")
        pb, poses = self.problem, self.get_im_poses().double().cpu().numpy()
        focals, pps = self.get_focals().flatten().cpu().numpy(), self.get_principal_points().cpu().numpy()
        best = {}
        for e, (i, j) in enumerate(self.edges):
            thr = min(self.min_conf_thr, float(self.conf_i[e].min()) - 0.1)
            # camera j in the frame of i, from the pointmap of j's pixels given in i's frame
            p = torch.where((self.conf_j[e] > thr)[..., None], pb.P[1][e], torch.full_like(pb.P[1][e], float("nan")))
            P2 = np.asarray(self.backend.pose(p, float(focals[j]), tuple(pps[j])), np.float64)
            base_pred, base_true = np.linalg.norm(P2[:3, 3]), np.linalg.norm(poses[j][:3, 3] - poses[i][:3, 3])
            s = base_true / base_pred if base_pred > 1e-9 and base_true > 0 else 1.0
            self._set_pose(self.pw_poses, e, poses[i][:3, :3], poses[i][:3, 3], scale=s)
            score = float(self.conf_i[e].mean())
            if score > best.get(i, (0.0,))[0]:
                best[i] = (score, e, s)
        for n in range(self.n_imgs):
            if n in best:
                _, e, s = best[n]
                self._set_depthmap(n, pb.P[0][e][..., 2] * s)

    def compute_global_alignment(self, init=None, niter=300, lr=0.01, schedule="cosine", lr_min=1e-6, niter_PnP=10):
        """initialise (None, "mst" or "known_poses"), then niter steps of Adam(betas 0.9, 0.9) with the learning rate set per iteration
        by the cosine or linear schedule -> the last loss (float); `losses` keeps the whole trajectory"""
        if schedule not in ("cosine", "linear"):
            raise ValueError("compute_global_alignment: schedule must be 'cosine' or 'linear', got %r" % (schedule,))
        if init in ("mst", "msp"):
            self.init_minimum_spanning_tree(niter_PnP=niter_PnP)
        elif init == "known_poses":
            self.init_from_known_poses(niter_PnP=niter_PnP)
        elif init is not None:
            raise ValueError("compute_global_alignment: init must be None, 'mst' or 'known_poses', got %r" % (init,))
        params = [p for p in self.parameters() if p.requires_grad]
        self.losses = []
        if not params or niter <= 0:
            return float("inf")
        opt = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.9))
        sched = cosine_schedule if schedule == "cosine" else linear_schedule
        loss = float("inf")
        for it in range(niter):
            for g in opt.param_groups:
                g["lr"] = sched(it / niter, lr, lr_min)
            opt.zero_grad()
            out = self()
            out.backward()
            opt.step()
            loss = float(out.detach())
            self.losses.append(loss)
        return loss
