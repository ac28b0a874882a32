"""spann3r_amd.mesh and PointRenderer.add_mesh on the device: the face list against the reference's own output
(tests/golden/mesh_faces.npz), everything else against the numpy restatement of the header's rules (tests/mesh_ref.py)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
import mesh_ref as MR
import render_ref as RR
from spann3r_amd import mesh as M
from test_mesh_cpu import CASES_1, read_glb

pytestmark = pytest.mark.gpu
W, H = 48, 32
# Depth tolerance of the rasteriser tests (relative).  Measured on the inputs of raster_cases() below: the header's rule evaluated
# with every operation rounded to fp32 (mesh_ref.raster, dtype=np.float32) against the same rule in float64 differs by at most
# 1.8e-7 relative over all covered pixels (python tests/test_mesh_gpu.py prints it; no GPU involved).  The bound is that figure times
# a margin of 4, rounded up: about 16 fp32 roundings of 2^-24 = 6e-8 each would give 9.5e-7 at worst.
DEPTH_MEASURED, DEPTH_RTOL = 1.8e-7, 1e-6


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ mesh build
@pytest.fixture(scope="module")
def golden():
    return dict(load_golden("mesh_faces.npz"))


@pytest.fixture(scope="module")
def big():
    """3 frames of 64 x 80: 4977 cells per block, 20 scan tiles per block; one frame's mask is random, one sparse, one dense"""
    rng = np.random.default_rng(5)
    valid = np.stack([rng.random((64, 80)) < 0.8, rng.random((64, 80)) < 0.3, rng.random((64, 80)) < 0.97])
    pts = rng.standard_normal((3, 64, 80, 3)).astype(np.float32)
    img = rng.random((3, 64, 80, 3), dtype=np.float32)
    return dict(valid=valid, pts=pts, img=img, ref=MR.faces_ref(valid), ref_fwd=MR.faces_ref(valid, both_windings=False))


def _check_mesh(m, g, case):
    for k in ("vertices", "faces", "face_colors"):
        ref = g[case + "_" + k]
        got = m[k].cpu().numpy()
        assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref), (case, k)


@pytest.mark.parametrize("case", CASES_1)
def test_pts3d_to_mesh_equals_the_reference(golden, case):
    m = M.pts3d_to_mesh(_t(golden[case + "_img"]), _t(golden[case + "_pts"]), _t(golden[case + "_valid"]))
    _check_mesh(m, golden, case)


def test_pts3d_to_mesh_without_a_mask(golden):
    m = M.pts3d_to_mesh(_t(golden["c5x7_img"]), _t(golden["c5x7_pts"]))
    faces, colour, _ = MR.faces_ref(np.ones((1, 5, 7), bool))
    assert np.array_equal(m["faces"].cpu().numpy(), faces)
    assert np.array_equal(m["face_colors"].cpu().numpy(), golden["c5x7_img"].reshape(-1, 3)[colour])


def test_cat_meshes_equals_the_reference(golden):
    g = golden
    meshes = [M.pts3d_to_mesh(_t(g["c9x13x3_img"][i]), _t(g["c9x13x3_pts"][i]), _t(g["c9x13x3_valid"][i])) for i in range(3)]
    before = [m["faces"].clone() for m in meshes]
    _check_mesh(M.cat_meshes(meshes), g, "c9x13x3")
    assert all(torch.equal(a, m["faces"]) for a, m in zip(before, meshes))
    # the same three frames in one call of the kernel: the global indices cat_meshes produces
    faces, colour, counts = M.build_faces(3, 9, 13, "cuda", valid=_t(g["c9x13x3_valid"].astype(np.uint8)))
    assert np.array_equal(faces.cpu().numpy(), g["c9x13x3_faces"]) and counts == MR.faces_ref(g["c9x13x3_valid"])[2]
    assert np.array_equal(g["c9x13x3_img"].reshape(-1, 3)[colour.cpu().numpy()], g["c9x13x3_face_colors"])


def test_faces_many_tiles_windings_conf_and_determinism(big):
    valid = _t(big["valid"].astype(np.uint8))
    ref_f, ref_c, ref_n = big["ref"]
    faces, colour, counts = M.build_faces(3, 64, 80, "cuda", valid=valid)
    assert counts == ref_n and np.array_equal(faces.cpu().numpy(), ref_f) and np.array_equal(colour.cpu().numpy(), ref_c)
    again = M.build_faces(3, 64, 80, "cuda", valid=valid)
    assert torch.equal(again[0], faces) and torch.equal(again[1], colour) and again[2] == counts
    # forward windings only = blocks 0 and 2 of every frame of the full list
    fwd, col_fwd, n_fwd = M.build_faces(3, 64, 80, "cuda", valid=valid, both_windings=False)
    starts = np.cumsum([0] + ref_n[1:])
    rows = np.concatenate([np.arange(starts[4 * f + b], starts[4 * f + b + 1]) for f in range(3) for b in (0, 2)])
    assert np.array_equal(fwd.cpu().numpy(), ref_f[rows]) and np.array_equal(col_fwd.cpu().numpy(), ref_c[rows])
    assert n_fwd == big["ref_fwd"][2] and np.array_equal(fwd.cpu().numpy(), big["ref_fwd"][0])
    # conf + threshold in the kernel = the same call with the mask computed by torch; confidences include 1 (0 > t fails), NaN, inf
    rng = np.random.default_rng(6)
    conf = (1 + rng.random((3, 64, 80)) * 0.01).astype(np.float32)
    conf.reshape(-1)[:5] = (1.0, np.nan, np.inf, 0.0, -1.0)
    c = _t(conf)
    mask = ((c - 1) / c > 3e-3).to(torch.uint8)
    assert 0.2 < float(mask.float().mean()) < 0.8
    a = M.build_faces(3, 64, 80, "cuda", conf=c, conf_thresh=3e-3)
    b = M.build_faces(3, 64, 80, "cuda", valid=mask)
    assert a[2] == b[2] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2] == MR.faces_ref(MR.conf_valid(conf, 3e-3))[2]
    # pts adds the finiteness test
    pts = big["pts"].copy()
    pts[1, 5, 7, 2], pts[2, 63, 79, 0] = np.nan, np.inf
    ok = big["valid"].copy()
    ok[1, 5, 7] = ok[2, 63, 79] = False
    assert big["valid"][2, 63, 79] and M.build_faces(3, 64, 80, "cuda", valid=valid, pts=_t(pts))[2] == MR.faces_ref(ok)[2]


def test_degenerate_grids():
    for t, h, w in ((1, 1, 5), (2, 4, 1), (1, 2, 2)):
        faces, colour, counts = M.build_faces(t, h, w, "cuda")
        assert counts == MR.faces_ref(np.ones((t, h, w), bool))[2] and faces.shape == (counts[0], 3)


# ------------------------------------------------------------------------------------------------ vertex compaction
XF = np.array([[0.5, -2.0, 0.25, 1.0], [0.0, 1.5, -1.0, -3.0], [2.0, 0.125, 1.0, 0.5], [0, 0, 0, 1]])


@pytest.mark.parametrize("which", ["c5x7", "big"])
def test_compact_vertices_mesh(golden, big, which):
    if which == "c5x7":
        valid, pts = golden["c5x7_valid"][None], golden["c5x7_pts"][None]
    else:
        valid, pts = big["valid"], big["pts"]
    pts = pts.copy()
    pts.reshape(-1, 3)[np.flatnonzero(~valid.ravel())[::3]] = np.nan            # non-finite points under the mask must never appear
    t, h, w = valid.shape
    ref_faces = MR.faces_ref(valid, both_windings=False)[0]
    faces, _, _ = M.build_faces(t, h, w, "cuda", valid=_t(valid.astype(np.uint8)), pts=_t(pts), both_windings=False)
    rgba = torch.arange(t * h * w, dtype=torch.int32, device="cuda") * 7 + 1
    pos, col, bounds = M.compact_vertices(_t(pts).reshape(-1, 3), rgba, faces=faces, scale=10.0, transform=XF)
    rpos, kept, rfaces, rbounds = MR.compact_ref(pts, ref_faces, scale=10.0, transform=XF)
    assert len(kept) > 0 and len(kept) < t * h * w
    assert np.array_equal(pos.cpu().numpy(), rpos) and np.isfinite(pos.cpu().numpy()).all()
    assert np.array_equal(col.cpu().numpy(), kept * 7 + 1)
    assert np.array_equal(faces.cpu().numpy(), rfaces) and np.array_equal(bounds, rbounds)


@pytest.mark.parametrize("which", ["c5x7", "big"])
def test_compact_vertices_cloud(golden, big, which):
    if which == "c5x7":
        valid, pts = golden["c5x7_valid"][None], golden["c5x7_pts"][None]
    else:
        valid, pts = big["valid"], big["pts"]
    pts = pts.copy()
    pts.reshape(-1, 3)[::11, 1] = np.inf                                        # valid or not: a non-finite point is never kept
    keep = valid.ravel() & np.isfinite(pts.reshape(-1, 3)).all(1)
    rgba = torch.arange(keep.size, dtype=torch.int32, device="cuda")
    pos, col, bounds = M.compact_vertices(_t(pts).reshape(-1, 3), rgba, valid=_t(valid.astype(np.uint8)), scale=10.0, transform=M.TRANSFORM)
    rpos, kept, _, rbounds = MR.compact_ref(pts, keep=keep, scale=10.0, transform=M.TRANSFORM)
    assert np.array_equal(pos.cpu().numpy(), rpos) and np.array_equal(col.cpu().numpy(), kept) and np.array_equal(bounds, rbounds)
    assert np.array_equal(rpos, pts.reshape(-1, 3)[kept] * np.float32(10) * np.float32([-1, -1, 1]))
    none = M.compact_vertices(_t(pts).reshape(-1, 3), rgba, valid=torch.zeros(keep.size, dtype=torch.uint8, device="cuda"))
    assert none[0].shape == (0, 3) and np.array_equal(none[2], [[np.inf] * 3, [-np.inf] * 3])


# ------------------------------------------------------------------------------------------------ rasteriser
def _rot(deg, axis=(0.3, 1.0, 0.2)):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


CAM = RR.Cam(np.eye(3), np.zeros(3), 16.0, 16.0, 24.0, 16.0, W, H, 0.0, 1)
CAM_NEAR = RR.Cam(np.eye(3), np.zeros(3), 16.0, 16.0, 24.0, 16.0, W, H, 1.0, 1)
CAM_POSE = RR.Cam(_rot(20.0), np.array([0.3, -0.2, 0.5]), 17.0, 18.5, 23.25, 15.625, W, H, 0.0, 1)


def _verts(cam, uvz):
    """fp32 world points that project to the screen coordinates u, v (pixels) at depth z"""
    uvz = np.asarray(uvz, np.float64).reshape(-1, 3)
    u, v, z = uvz[:, 0], uvz[:, 1], uvz[:, 2]
    Xc = np.stack(((u - cam.cx) * z / cam.fx, (v - cam.cy) * z / cam.fy, z), 1)
    return ((Xc - cam.t) @ cam.R).astype(np.float32)


QUAD = [(8, 4, 2.0), (24, 4, 3.0), (8, 20, 3.0), (24, 20, 4.0)]      # corners on pixel centres; the diagonal 1-2 passes through 15 more


def raster_cases():
    """name -> (pts fp32 [n, 3], faces [F, 3], colour_px or None, cam, max_bbox_px).  Screen coordinates are multiples of 1/16 pixel
    (CAM) or sit within 0.2 / 16 of one (CAM_POSE), so fp32 and float64 snap alike; test_raster_inputs_are_safe verifies it."""
    rng = np.random.default_rng(3)
    tri = [(5, 3.5, 2.0), (30.25, 6, 3.0), (12, 25.0625, 5.0)]
    cases = {
        "front": (_verts(CAM, tri), [[0, 1, 2]], None, CAM, 4096),
        "back": (_verts(CAM, tri), [[0, 2, 1]], None, CAM, 4096),
        "quad": (_verts(CAM, QUAD), [[0, 1, 2], [1, 3, 2]], [0, 3], CAM, 4096),
        "quad_a": (_verts(CAM, QUAD), [[0, 1, 2]], [0], CAM, 4096),
        "quad_b": (_verts(CAM, QUAD), [[1, 3, 2]], [3], CAM, 4096),
        "zero_area": (_verts(CAM, [(4, 4, 2.0), (12, 12, 3.0), (20, 20, 2.0), (6, 6, 2.0)]), [[0, 1, 2], [3, 3, 3], [0, 0, 1]], None, CAM, 4096),
        "behind_near": (_verts(CAM_NEAR, [(5, 3, 2.0), (30, 6, 0.5), (12, 25, 5.0), (40, 28, 1.5)]), [[0, 1, 2], [0, 2, 3]], None, CAM_NEAR, 4096),
        "bbox_over": (_verts(CAM, [(5, 3, 2.0), (25, 3, 2.0), (5, 23, 3.0)]), [[0, 1, 2]], None, CAM, 440),       # 21 x 21 pixels in its box
        "bbox_at": (_verts(CAM, [(5, 3, 2.0), (25, 3, 2.0), (5, 23, 3.0)]), [[0, 1, 2]], None, CAM, 441),
        "half_outside": (_verts(CAM, [(-10, 5, 2.0), (30, 10, 3.0), (-10.5, 28, 2.5), (40, 20, 2.0), (60, 44, 3.0), (30, 45.25, 4.0)]),
                         [[0, 1, 2], [3, 4, 5]], None, CAM, 4096),
        "outside": (_verts(CAM, [(-30, 5, 2.0), (-5, 10, 3.0), (-10, 28, 2.5), (5, -9, 2.0), (40, -0.0625, 2.0), (20, -20, 2.0)]),
                    [[0, 1, 2], [3, 4, 5]], None, CAM, 4096),
    }
    # overlapping and crossing triangles under a general pose, vertices shared, colour pixel = any vertex
    uv = rng.integers(0, [16 * W, 16 * H], (24, 2)) / 16.0 + rng.uniform(-0.2, 0.2, (24, 2)) / 16.0
    uvz = np.c_[uv, rng.uniform(2.0, 4.0, 24)]
    faces = np.stack([rng.permutation(24)[:3] for _ in range(40)])
    cases["soup"] = (_verts(CAM_POSE, uvz), faces, rng.integers(0, 24, 40), CAM_POSE, 600)
    return {k: (p, np.asarray(f, np.int32), None if c is None else np.asarray(c, np.int32), cam, mb) for k, (p, f, c, cam, mb) in cases.items()}


def _render_cam(cam):
    from spann3r_amd import lib as L
    return L.RenderCam((ctypes.c_float * 9)(*cam.R.reshape(-1)), (ctypes.c_float * 3)(*cam.t), cam.fx, cam.fy, cam.cx, cam.cy, cam.width,
                       cam.height, cam.z_near, cam.point_size)


class Buffer:
    """a key buffer driven through the library directly"""

    def __init__(self, cam):
        from spann3r_amd import lib as L
        self.L, self.lib, self.cam, self.rc = L, L.load(), cam, _render_cam(cam)
        self.keys = torch.empty(cam.width * cam.height, dtype=torch.int64, device="cuda")
        self.culled = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.L.check(self.lib.sp3_render_clear(self.keys.data_ptr(), self.keys.numel(), L.stream_ptr()), "sp3_render_clear")

    def tris(self, pts, faces, colour_px, max_bbox_px, index_base=0, rows=None):
        p, f = _t(pts), _t(faces if rows is None else faces[rows])
        c = None if colour_px is None else _t(colour_px if rows is None else colour_px[rows])
        self.L.check(self.lib.sp3_render_tris(p.data_ptr(), len(pts), f.data_ptr(), self.L.ptr(c), len(f), None, index_base, ctypes.byref(self.rc),
                                              max_bbox_px, self.keys.data_ptr(), self.culled.data_ptr(), self.L.stream_ptr()), "sp3_render_tris")
        torch.cuda.synchronize()
        return self

    def points(self, pts, index_base=0):
        p = _t(pts)
        self.L.check(self.lib.sp3_render_splat(p.data_ptr(), None, 0.0, len(pts), index_base, ctypes.byref(self.rc), self.keys.data_ptr(),
                                               self.L.stream_ptr()), "sp3_render_splat")
        torch.cuda.synchronize()
        return self

    def image(self, ncolours):
        h, w = self.cam.height, self.cam.width
        rgb = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
        depth, index = torch.empty((h, w), dtype=torch.float32, device="cuda"), torch.empty((h, w), dtype=torch.int32, device="cuda")
        rgba = torch.zeros(max(ncolours, 1), dtype=torch.int32, device="cuda")
        self.L.check(self.lib.sp3_render_resolve(self.keys.data_ptr(), rgba.data_ptr(), ctypes.byref(self.rc), 0, rgb.data_ptr(), depth.data_ptr(),
                                                 index.data_ptr(), self.L.stream_ptr()), "sp3_render_resolve")
        return index.cpu().numpy().astype(np.int64), depth.cpu().numpy(), int(self.culled.item())


def _assert_same(got, ref):
    (gi, gd, gc), (ri, rd, rc) = got, ref
    assert np.array_equal(gi, ri), "coverage or winner differ at %s" % (np.argwhere(gi != ri)[:8].tolist(),)
    assert gc == rc
    m = ri >= 0
    assert np.isinf(gd[~m]).all() and (m.sum() == 0 or np.abs(gd[m] / rd[m] - 1).max() <= DEPTH_RTOL)


def _snapped(pts, cam, dt):
    u, v, _, ok = MR.project(pts, cam, dt)
    return MR.snap(u, v, ok)


def test_raster_inputs_are_safe():
    """every projected vertex stays at least a quarter of a snapping step from a snapping boundary, and fp32 snaps as float64 does"""
    for name, (pts, faces, col, cam, mb) in raster_cases().items():
        d = MR.snap_boundary_distance(pts, cam)
        assert d[np.isfinite(d)].min() >= 0.25, name
        a, b = _snapped(pts, cam, np.float32), _snapped(pts, cam, np.float64)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
        # ... and no pixel's winner hangs on the last bits of a depth: the rule in fp32 picks what it picks in float64
        assert np.array_equal(MR.raster(pts, faces, col, cam, mb, dtype=np.float32)[0], MR.raster(pts, faces, col, cam, mb)[0]), name


@pytest.mark.parametrize("name", ["front", "back", "quad", "zero_area", "behind_near", "bbox_over", "bbox_at", "half_outside", "outside", "soup"])
def test_raster_equals_the_restatement(name):
    """coverage, winner and the count of culled triangles exact; depth within DEPTH_RTOL = 1e-6 relative, where the rule rounded to
    fp32 differs from float64 by DEPTH_MEASURED = 1.8e-7 at most on these inputs (measured on the CPU, see the top of the file)"""
    pts, faces, col, cam, mb = raster_cases()[name]
    ref = MR.raster(pts, faces, col, cam, mb)
    _assert_same(Buffer(cam).tris(pts, faces, col, mb).image(len(pts)), ref)
    covered = int((ref[0] >= 0).sum())
    expect = {"zero_area": 0, "behind_near": None, "bbox_over": 0, "outside": 0, "quad": 256}.get(name, None)
    assert expect is None or covered == expect
    if name == "behind_near":          # the face with the vertex at z = 0.5 <= z_near is gone, the other is drawn
        assert covered > 0 and set(np.unique(ref[0])) == {-1, 0}
        assert np.array_equal(ref[0], MR.raster(pts, faces[1:], None, cam, mb)[0])
    if name in ("bbox_over", "bbox_at"):
        assert ref[2] == (1 if name == "bbox_over" else 0) and (covered > 0) == (name == "bbox_at")
    if name in ("front", "half_outside", "soup"):
        assert covered > 50


def test_both_orientations_cover_alike():
    c = raster_cases()
    a = Buffer(CAM).tris(*c["front"][:3], 4096).image(3)
    b = Buffer(CAM).tris(*c["back"][:3], 4096).image(3)
    assert np.array_equal(a[0], b[0]) and (a[0] >= 0).sum() > 50
    assert np.abs(a[1][a[0] >= 0] / b[1][a[0] >= 0] - 1).max() <= DEPTH_RTOL


def test_shared_edge_pixels_are_drawn_exactly_once():
    """the two triangles of a quad whose corners and diagonal lie on pixel centres: drawn alone their coverages are disjoint, together
    they are the 16 x 16 pixels the top-left rule gives the quad (left and top edge in, right and bottom edge out)"""
    c = raster_cases()
    a = Buffer(CAM).tris(*c["quad_a"][:3], 4096).image(4)[0] >= 0
    b = Buffer(CAM).tris(*c["quad_b"][:3], 4096).image(4)[0] >= 0
    both = Buffer(CAM).tris(*c["quad"][:3], 4096).image(4)[0] >= 0
    want = np.zeros((H, W), bool)
    want[4:20, 8:24] = True
    assert not (a & b).any() and np.array_equal(a | b, want) and np.array_equal(both, want)
    diag = [(4 + k, 24 - k) for k in range(1, 16)]                              # pixel centres exactly on the shared edge
    assert all(a[y, x] != b[y, x] for y, x in diag)
    assert a.sum() + b.sum() == 256


def test_arrival_order_does_not_matter():
    pts, faces, col, cam, mb = raster_cases()["soup"]
    n = len(faces)
    one = Buffer(cam).tris(pts, faces, col, mb)
    ab = Buffer(cam).tris(pts, faces, col, mb, rows=np.arange(n // 2)).tris(pts, faces, col, mb, rows=np.arange(n // 2, n))
    ba = Buffer(cam).tris(pts, faces, col, mb, rows=np.arange(n // 2, n)).tris(pts, faces, col, mb, rows=np.arange(n // 2))
    rev = Buffer(cam).tris(pts, faces, col, mb, rows=np.arange(n)[::-1].copy())
    assert torch.equal(ab.keys, ba.keys) and torch.equal(ab.keys, one.keys) and torch.equal(rev.keys, one.keys)
    assert (one.keys != -1).sum() > 50


def test_points_and_triangles_share_one_buffer():
    pts, faces, col, cam, mb = raster_cases()["soup"]
    rng = np.random.default_rng(8)
    n = 300
    uvz = np.c_[rng.integers(0, W, n) + rng.uniform(-0.25, 0.25, n), rng.integers(0, H, n) + rng.uniform(-0.25, 0.25, n),
                rng.choice([1.25, 2.25, 2.75, 3.5, 6.0], n) * 1.0005 ** rng.permutation(n)]      # in front of, between and behind the
    # triangles; all distinct by 5e-4 relative, so two points on one pixel never tie within fp32's rounding of the pose
    cloud = _verts(cam, uvz)
    assert RR.boundary_distance(cloud, cam).min() >= 0.2
    got = Buffer(cam).points(cloud, 0).tris(pts, faces, col, mb, index_base=n).image(n + len(pts))
    other = Buffer(cam).tris(pts, faces, col, mb, index_base=n).points(cloud, 0).image(n + len(pts))
    ti, td, tc = MR.raster(pts, faces, col, cam, mb, index_base=n)
    pi, pd = RR.render(cloud, cam)
    ri, rd = MR.merge([(pi, pd), (ti, td)])
    _assert_same(got, (ri, rd, tc))
    _assert_same(other, (ri, rd, tc))
    assert ((ri >= 0) & (ri < n)).sum() > 30 and (ri >= n).sum() > 30 and ((pi >= 0) & (ri >= n)).sum() > 0


def test_render_frames_surface_is_solid():
    """a 12 x 16 planar pointmap seen head-on, 2.5 pixels between neighbours: the splat leaves holes inside the silhouette, the mesh none"""
    from spann3r_amd import vis
    u, v = 4.3 + 2.5 * np.arange(16), 2.3 + 2.5 * np.arange(12)
    uvz = np.stack(np.broadcast_arrays(u[None, :], v[:, None], 2.0), -1).reshape(-1, 3)
    pts = _t(_verts(CAM, uvz).reshape(1, 12, 16, 3))
    img = torch.ones_like(pts)
    cam = vis.Camera([[CAM.fx, 0, CAM.cx], [0, CAM.fy, CAM.cy], [0, 0, 1]], np.eye(4), W, H)
    inside = np.zeros((H, W), bool)
    inside[3:30, 5:42] = True                                                   # pixel centres strictly inside 4.3..41.8 x 2.3..29.8
    dots = vis.render_frames(pts, img, cam)[0].cpu().numpy()
    solid = vis.render_frames(pts, img, cam, surface=True)[0].cpu().numpy()
    again = vis.render_frames(pts, img, cam, surface=True, max_bbox_px=4096)[0].cpu().numpy()
    assert (dots[inside] == 0).any() and (dots == 255).any()
    assert (solid[inside] == 255).all() and (solid[~inside] == 0).all() and np.array_equal(solid, again)
    # max_bbox_px below the 2 x 2 pixels every cell's box holds at least: nothing is surface; a mask and a confidence map cut the same hole
    assert (vis.render_frames(pts, img, cam, surface=True, max_bbox_px=3).cpu().numpy() == 0).all()
    mask = torch.ones((1, 12, 16), dtype=torch.bool, device="cuda")
    mask[0, 5, 7] = False
    conf = torch.where(mask, 2.0, 1.0)
    holed = vis.render_frames(pts, img, cam, surface=True, mask=mask)[0].cpu().numpy()
    assert np.array_equal(holed, vis.render_frames(pts, img, cam, surface=True, conf_all=conf, conf_thresh=0.1)[0].cpu().numpy())
    assert (holed[inside] == 0).any() and (holed != solid).sum() > 0


def test_add_mesh_equals_the_restatement_and_mixes_with_points():
    from spann3r_amd import vis
    rng = np.random.default_rng(9)
    h, w = 7, 9
    uv = np.stack(np.broadcast_arrays(3.125 + 4.25 * np.arange(w)[None, :], 2.0 + 4.0 * np.arange(h)[:, None]), -1).reshape(-1, 2)
    uv = np.round(uv * 16) / 16 + rng.uniform(-0.2, 0.2, uv.shape) / 16
    pm = _verts(CAM_POSE, np.c_[uv, rng.uniform(2.0, 3.0, h * w)])
    assert MR.snap_boundary_distance(pm, CAM_POSE).min() >= 0.25 and RR.boundary_distance(pm, CAM_POSE).min() >= 0.1
    pm[10] = np.nan
    valid = rng.random((h, w)) < 0.9
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = CAM_POSE.R, CAM_POSE.t
    r = vis.PointRenderer(camera=vis.Camera([[CAM_POSE.fx, 0, CAM_POSE.cx], [0, CAM_POSE.fy, CAM_POSE.cy], [0, 0, 1]], E, W, H))
    cols = rng.integers(0, 256, (h * w, 3)).astype(np.float32) / 255
    r.add(_t(pm), _t(cols))
    r.add_mesh(_t(pm.reshape(h, w, 3)), _t(cols.reshape(h, w, 3)), valid=_t(valid), max_bbox_px=20)
    rgb, depth, index = (x.cpu().numpy() for x in r.image(return_depth=True, return_index=True))
    ok = valid & np.isfinite(pm).all(1).reshape(h, w)
    faces, colour, _ = MR.faces_ref(ok[None], both_windings=False)
    safe = np.where(np.isfinite(pm), pm, 0)
    ti, td, tc = MR.raster(safe, faces, colour, CAM_POSE, 20, index_base=h * w)
    assert 0 < tc < len(faces) // 2
    pi, pd = RR.render(pm, CAM_POSE)
    ri, rd = MR.merge([(pi, pd), (ti, td)])
    _assert_same((index.astype(np.int64), depth, int(r.mesh_stats[1].item())), (ri, rd, tc))
    assert int(r.mesh_stats[0].item()) == len(faces) and (ri >= h * w).sum() > 100
    assert np.array_equal(rgb, RR.resolve(np.where(ri >= h * w, ri - h * w, ri), cols))
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.add_mesh(torch.zeros(h, w, 3), torch.zeros(h, w, 3))
    with pytest.raises(RuntimeError, match="not both"):
        r.add_mesh(_t(pm.reshape(h, w, 3)), _t(cols.reshape(h, w, 3)), conf=_t(np.ones((h, w), np.float32)), valid=_t(valid))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("as_pointcloud", [False, True])
def test_scene_mesh_and_write_glb(tmp_path, as_pointcloud):
    rng = np.random.default_rng(11)
    t, h, w = 3, 12, 16
    pts = rng.standard_normal((t, h, w, 3)).astype(np.float32)
    img = rng.random((t, h, w, 3), dtype=np.float32)
    conf = (1 + rng.random((t, h, w)) * 0.01).astype(np.float32)
    pts[1, 3, 4, 0] = np.nan
    conf[1, 3, 4] = 5.0
    ok = MR.conf_valid(conf, 3e-3) & np.isfinite(pts).all(-1)
    scene = M.scene_mesh(_t(pts), _t(img), _t(conf), 3e-3, as_pointcloud=as_pointcloud)
    path = str(tmp_path / "scene.glb")
    M.write_glb(path, scene["vertices"], scene["colors"], scene["faces"], bounds=scene["bounds"])
    g = read_glb(path)
    if as_pointcloud:
        rpos, kept, rfaces, rbounds = MR.compact_ref(pts, keep=ok, scale=10.0, transform=M.TRANSFORM)
        assert g["indices"] is None and g["mode"] == 0
    else:
        rpos, kept, rfaces, rbounds = MR.compact_ref(pts, MR.faces_ref(ok, both_windings=False)[0], scale=10.0, transform=M.TRANSFORM)
        assert g["mode"] == 4 and np.array_equal(g["indices"], rfaces) and len(rfaces) > 100
    assert len(kept) > 100 and g["positions"].shape == rpos.shape and np.array_equal(g["positions"], rpos)
    assert np.array_equal(rpos, pts.reshape(-1, 3)[kept] * np.float32(10) * np.float32([-1, -1, 1]))
    assert np.array_equal(g["colors"][:, :3], RR.pack_rgba8(img.reshape(-1, 3)[kept])) and (g["colors"][:, 3] == 255).all()
    assert np.array_equal(scene["bounds"], rbounds)


def test_export_glb_takes_forward_outputs(tmp_path):
    rng = np.random.default_rng(12)
    preds, batch = [], []
    for j in range(2):
        p = {"conf": _t((1 + rng.random((1, 12, 16))).astype(np.float32)),
             "pts3d" if j == 0 else "pts3d_in_other_view": _t(rng.standard_normal((1, 12, 16, 3)).astype(np.float32))}
        preds.append(p)
        batch.append({"img": _t((rng.random((1, 3, 12, 16)) * 2 - 1).astype(np.float32))})
    info = M.export_glb(str(tmp_path / "x.glb"), preds, batch, conf_thresh=0.2)
    g = read_glb(str(tmp_path / "x.glb"))
    assert info == dict(vertices=len(g["positions"]), faces=len(g["indices"]), bytes=g["length"]) and info["faces"] > 50
    with pytest.raises(RuntimeError, match="nothing passes"):
        M.export_glb(str(tmp_path / "y.glb"), preds, batch, conf_thresh=0.99)


if __name__ == "__main__":
    # the fp32-vs-float64 depth difference DEPTH_MEASURED is taken from (CPU only)
    worst = 0.0
    for name, (pts, faces, col, cam, mb) in raster_cases().items():
        i32, d32, _ = MR.raster(pts, faces, col, cam, mb, dtype=np.float32)
        i64, d64, _ = MR.raster(pts, faces, col, cam, mb)
        assert np.array_equal(i32, i64), name
        m = i64 >= 0
        if m.any():
            worst = max(worst, float(np.abs(d32[m].astype(np.float64) / d64[m] - 1).max()))
            print("%-14s %5d pixels, depth fp32 vs float64: %.3g" % (name, m.sum(), np.abs(d32[m].astype(np.float64) / d64[m] - 1).max()))
    print("worst %.3g" % worst)
