"""spann3r_amd.vis: the headless point rasteriser (csrc/render.hip) and the colourisers of vis_pred_and_imgs.

The pin of the rasteriser is tests/render_ref.py, a float64 restatement of its rule (Open3D, whose window the reference draws in, is
not available anywhere: parity with it is unpinned).  The colour maps are pinned to the installed matplotlib through
tests/golden/vis_colormaps.npz (tests/golden/make_golden_vis.py).

Boundary-safe inputs: points are made from integer pixel targets plus a jitter of at most 0.25 px, x = (u - cx) z / fx, so fp32 and
float64 round to the same pixel with a margin (0.25 px) three orders above the fp32 projection error (about 1e-4 px at these image
sizes); every test asserts on the CPU that the float64 projection of each of its points stays at least 0.2 px from a rounding
boundary, so no point is excluded from a comparison.  Tolerances: index and rgb are compared exactly; depth exactly for the identity
pose (Xc.z = z, no rounding) and within 4 * 2^-24 * (|R||X| + |t|) of float64 for a general pose (three rounded products and three
rounded sums of the z row)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import render_ref as RR
from conftest import REPO

gpu = pytest.mark.gpu
DEPTHS = (1.0, 1.5, 2.0, 3.0)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "vis_colormaps.npz")))


def _rot(deg, axis=(0.3, 1.0, 0.2)):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _cam(W, H, R=None, t=None, point_size=1, f=None):
    f = f if f is not None else 0.8 * W
    return RR.Cam(np.eye(3) if R is None else R, np.zeros(3) if t is None else t, f, f * 1.05, (W - 1) / 2.0 + 0.25, (H - 1) / 2.0 - 0.125, W, H,
                  0.0, point_size)


def _safe_points(rng, cam, n, depths=None, bad=0.05, targets=None, k0=0):
    """fp32 world points [n, 3] whose projections sit within 0.25 px of integer pixels; `bad` of them culled one way or another
    (z <= 0, a NaN, outside the image).  depths: values to draw from, or None for distinct depths 1.002^k, k = k0 .. k0 + n - 1."""
    if targets is None:
        tu, tv = rng.integers(0, cam.width, n), rng.integers(0, cam.height, n)
    else:
        tu, tv = targets
    u = tu + rng.uniform(-0.25, 0.25, n)
    v = tv + rng.uniform(-0.25, 0.25, n)
    z = rng.choice(depths, n) if depths is not None else 1.002 ** (k0 + rng.permutation(n))
    kind = np.where(rng.random(n) < bad, rng.integers(1, 5, n), 0)
    z = np.where(kind == 1, -z, z)                                                  # behind the camera
    if depths is not None:                                                          # (identity-pose tests: Xc.z = z exactly)
        z = np.where((kind == 1) & (rng.random(n) < 0.3), 0.0, z)                   # ... or exactly on its plane
    u = np.where(kind == 2, cam.width + 4 + tu % 7, u)                              # right of the image
    v = np.where(kind == 3, -3.0 - tv % 5, v)                                       # above it
    Xc = np.stack(((u - cam.cx) * z / cam.fx, (v - cam.cy) * z / cam.fy, z), 1)
    X = (Xc - cam.t) @ cam.R                                                        # R^T (Xc - t), row-wise
    X[kind == 4, rng.integers(0, 3)] = np.nan
    return X.astype(np.float32)


def _colors(rng, n):
    return (rng.integers(0, 256, (n, 3)) / 255.0).astype(np.float32)                # exact levels: packing has no rounding case


def _assert_safe(pts, cam):
    d = RR.boundary_distance(pts, cam)
    assert np.all(d >= 0.2), "a point's float64 projection is %.3f px from a rounding boundary" % d.min()


def _vis_camera(cam):
    from spann3r_amd import vis
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = cam.R, cam.t
    return vis.Camera([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], E, cam.width, cam.height)


def _renderer(cam, **kw):
    from spann3r_amd import vis
    return vis.PointRenderer(camera=_vis_camera(cam), point_size=cam.point_size, **kw)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _image(r):
    rgb, depth, index = r.image(return_depth=True, return_index=True)
    return rgb.cpu().numpy(), depth.cpu().numpy(), index.cpu().numpy()


def _frames(seed, cam, shapes, depths, bad=0.05):
    rng = np.random.default_rng(seed)
    pts = [_safe_points(rng, cam, n, depths, bad, k0=sum(shapes[:i])) for i, n in enumerate(shapes)]
    cols = [_colors(rng, n) for n in shapes]
    _assert_safe(np.concatenate(pts), cam)
    return pts, cols


# ------------------------------------------------------------------------------------------------ CPU
def test_restatement_gives_the_hand_computed_picture():
    """6 points into 4 x 3 pixels (fx = fy = 1, cx = cy = 0, identity pose): two on pixel (1, 0) at depths 2 and 1 (the nearer, later one
    wins), two on pixel (2, 1) at the same depth (the earlier one wins), one behind the camera, one outside the image."""
    cam = RR.Cam(np.eye(3), np.zeros(3), 1, 1, 0, 0, 4, 3)
    pts = np.array([[2.0, 0.0, 2.0],        # 0: pixel (1, 0), depth 2
                    [1.0, 0.0, 1.0],        # 1: pixel (1, 0), depth 1 -> wins
                    [4.0, 2.0, 2.0],        # 2: pixel (2, 1), depth 2 -> wins the tie
                    [4.2, 1.8, 2.0],        # 3: pixel (2, 1), depth 2 (u = 2.1, v = 0.9)
                    [0.0, 0.0, -1.0],       # 4: behind the camera
                    [9.0, 0.0, 1.0]])       # 5: pixel (9, 0), outside
    cols = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 1, 1], [0, 1, 1]], np.float64) * (200 / 255)
    index, depth = RR.render(pts, cam)
    want_i = np.array([[-1, 1, -1, -1], [-1, -1, 2, -1], [-1, -1, -1, -1]])
    want_d = np.full((3, 4), np.inf)
    want_d[0, 1], want_d[1, 2] = 1.0, 2.0
    assert np.array_equal(index, want_i) and np.array_equal(depth, want_d)
    rgb = RR.resolve(index, cols, background=(0, 0, 0.5))
    want = np.zeros((3, 4, 3), np.uint8)
    want[..., 2] = 128                       # floor(0.5 * 255 + 0.5)
    want[0, 1], want[1, 2] = (0, 200, 0), (0, 0, 200)
    assert np.array_equal(rgb, want)
    # the same through a 3-wide footprint, clipped at the top edge: point 1 covers x 0..2 of rows 0..1
    index3, _ = RR.render(pts[:2], RR.Cam(np.eye(3), np.zeros(3), 1, 1, 0, 0, 4, 3, point_size=3))
    assert np.array_equal(index3, np.array([[1, 1, 1, -1], [1, 1, 1, -1], [-1, -1, -1, -1]]))


def test_jet_table_equals_matplotlib(fx):
    from spann3r_amd import vis
    lut = vis.jet_lut()
    assert lut.dtype == np.uint8 and lut.shape == (256, 4) and np.array_equal(lut, fx["jet_lut"])


def test_fixture_mask_is_small(fx):
    """the near-integer allowance of the hsv comparison covers under 1 % of the entries: it cannot hide a wrong formula"""
    f64 = fx["hsv_f64"]
    near = np.abs(255 * f64 - np.rint(255 * f64)) <= 255 * 8 * 2.0 ** -24
    assert np.array_equal(near, fx["hsv_near"]) and near.mean() < 0.01
    x = fx["hsv_x"]
    assert x.dtype == np.float32 and x.min() == 0.0 and x.max() == 1.0
    for k in range(7):
        assert np.any(x[:, 0] == np.float32(1.0 - k / 6.0))


def test_camera_json_round_trip_and_open3d_layout(tmp_path):
    from spann3r_amd import vis
    rng = np.random.default_rng(5)
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = _rot(37.0), rng.normal(0, 1, 3) / 3.0
    K = np.array([[935.307436087194, 0, 959.5], [0, 935.307436087194 / 3, 539.5], [0, 0, 1]])
    cam = vis.Camera(K, E, 1920, 1080)
    p = str(tmp_path / "camera.json")
    vis.save_camera(p, cam)
    back = vis.load_camera(p)
    assert back.intrinsic.tobytes() == cam.intrinsic.tobytes() and back.extrinsic.tobytes() == cam.extrinsic.tobytes()
    assert (back.width, back.height) == (1920, 1080)
    # a file as Open3D writes it: column-major matrices
    q = str(tmp_path / "o3d.json")
    with open(q, "w") as f:
        f.write('{\n\t"class_name" : "PinholeCameraParameters",\n\t"extrinsic" : \n\t[\n\t\t0.0, 1.0, 0.0, 0.0,\n\t\t-1.0, 0.0, 0.0, 0.0,\n'
                '\t\t0.0, 0.0, 1.0, 0.0,\n\t\t0.5, -0.25, 2.0, 1.0\n\t],\n\t"intrinsic" : \n\t{\n\t\t"height" : 480,\n\t\t"intrinsic_matrix" : \n'
                '\t\t[\n\t\t\t500.0, 0.0, 0.0,\n\t\t\t0.0, 510.0, 0.0,\n\t\t\t319.5, 239.5, 1.0\n\t\t],\n\t\t"width" : 640\n\t},\n'
                '\t"version_major" : 1,\n\t"version_minor" : 0\n}')
    o = vis.load_camera(q)
    assert np.array_equal(o.extrinsic, np.array([[0, -1, 0, 0.5], [1, 0, 0, -0.25], [0, 0, 1, 2.0], [0, 0, 0, 1.0]]))
    assert np.array_equal(o.intrinsic, np.array([[500.0, 0, 319.5], [0, 510.0, 239.5], [0, 0, 1]]))
    assert (o.width, o.height) == (640, 480)
    import json
    d = json.load(open(p))
    assert sorted(d) == ["class_name", "extrinsic", "intrinsic", "version_major", "version_minor"]
    assert sorted(d["intrinsic"]) == ["height", "intrinsic_matrix", "width"] and d["extrinsic"][12:15] == list(E[:3, 3])


def test_fit_camera_box():
    """the box +-[1.0, 0.5, 0.25] around (0, 0, 3) seen from the identity pose: every corner inside the image, one within 5 % of a border
    (the fit makes the binding corner touch it: a property of the fit, not a measurement)"""
    from spann3r_amd import vis
    lo, hi = np.array([-1.0, -0.5, 2.75]), np.array([1.0, 0.5, 3.25])
    for W, H in ((1920, 1080), (640, 480), (300, 900)):
        cam = vis.camera_for_box(lo, hi, W, H, 60.0)
        assert np.array_equal(cam.extrinsic[:3, :3], np.eye(3)) and (cam.width, cam.height) == (W, H)
        ref = RR.Cam(cam.extrinsic[:3, :3], cam.extrinsic[:3, 3], cam.intrinsic[0, 0], cam.intrinsic[1, 1], cam.intrinsic[0, 2],
                     cam.intrinsic[1, 2], W, H)
        corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        u, v, z, ok = RR.project(corners, ref)
        assert ok.all() and np.all(u >= 0) and np.all(u <= W - 1) and np.all(v >= 0) and np.all(v <= H - 1)
        border = np.minimum(np.minimum(u, W - 1 - u) / W, np.minimum(v, H - 1 - v) / H)
        assert border.min() <= 0.05
        assert abs(cam.intrinsic[1, 1] - 0.5 * H / np.tan(np.radians(30.0))) < 1e-9


def test_render_cam_struct_matches_the_header():
    from spann3r_amd import lib
    fields = [f[0] for f in lib.RenderCam._fields_]
    src = ['#include "%s"' % os.path.join(REPO, "include", "spann3r_hip.h"), "#include <stdio.h>", "#include <stddef.h>", "int main(){",
           'printf("%zu\\n", sizeof(sp3_render_cam));'] + ['printf("%%zu\\n", offsetof(sp3_render_cam, %s));' % f for f in fields] + ["return 0;}"]
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(c, "w").write("\n".join(src) + "\n")
        subprocess.check_call(["gcc", c, "-o", exe])
        vals = [int(x) for x in subprocess.check_output([exe]).split()]
    assert vals == [ctypes.sizeof(lib.RenderCam)] + [getattr(lib.RenderCam, f).offset for f in fields]


# ------------------------------------------------------------------------------------------------ GPU
def _check_exact(r, pts, cols, cam, keep=None, depth_exact=True, background=(0, 0, 0)):
    """the renderer's picture against render_ref on the concatenated frames"""
    allp, allc = np.concatenate(pts), np.concatenate(cols)
    index, depth = RR.render(allp, cam, keep)
    rgb_d, depth_d, index_d = _image(r)
    assert rgb_d.shape == (cam.height, cam.width, 3) and rgb_d.dtype == np.uint8
    assert np.array_equal(index_d, index)
    assert np.array_equal(rgb_d, RR.resolve(index, allc, background))
    assert np.array_equal(np.isinf(depth_d), index < 0)
    if depth_exact:
        assert np.array_equal(depth_d.astype(np.float64), depth)
    else:
        m = index >= 0
        X = allp[index[m]].astype(np.float64)
        bound = 4 * 2.0 ** -24 * (np.abs(cam.R[2]) @ np.abs(X).T + abs(cam.t[2]))
        err = np.abs(depth_d[m].astype(np.float64) - depth[m])
        print("worst depth error / bound = %.3f" % float((err / bound).max()))
        assert np.all(err <= bound)
    return index


@gpu
def test_exact_picture_identity_pose():
    cam = _cam(61, 47)
    pts, cols = _frames(11, cam, [16 * 20] * 3, DEPTHS)
    index, _ = RR.render(np.concatenate(pts), cam)
    ranks = np.unique(index[index >= 0] // 320)
    assert len(ranks) == 3, "every frame should win pixels"
    r = _renderer(cam, background=(0.25, 0.5, 1.0))
    for p, c in zip(pts, cols):
        r.add(_t(p), _t(c))
    _check_exact(r, pts, cols, cam, background=(0.25, 0.5, 1.0))
    # pixels that several points reach, and exact depth ties among them, do occur in this input
    u, v, z, ok = RR.project(np.concatenate(pts), cam)
    pix = (np.floor(v[ok] + 0.5) * 61 + np.floor(u[ok] + 0.5)).astype(np.int64)
    inside = (np.floor(u[ok] + 0.5) >= 0) & (np.floor(u[ok] + 0.5) < 61) & (np.floor(v[ok] + 0.5) >= 0) & (np.floor(v[ok] + 0.5) < 47)
    pz = np.stack((pix[inside], z[ok][inside]), 1)
    assert len(np.unique(pix[inside])) < inside.sum() * 0.9 and len(np.unique(pz, axis=0)) < inside.sum()


@gpu
def test_general_pose():
    R = _rot(30.0)
    cam = _cam(61, 47, R, np.array([0.3, -0.2, 0.5]))
    pts, cols = _frames(12, cam, [16 * 20] * 3, None)
    _, _, z, ok = RR.project(np.concatenate(pts), cam)
    zs = np.sort(z[ok])
    assert np.all(zs[1:] / zs[:-1] - 1 >= 1e-3), "depths must be separated by 1e-3 relative"
    r = _renderer(cam)
    for p, c in zip(pts, cols):
        r.add(_t(p), _t(c))
    _check_exact(r, pts, cols, cam, depth_exact=False)


@gpu
def test_growing_equals_one_shot_and_dynamic_equals_fresh():
    import torch
    cam = _cam(61, 47)
    pts, cols = _frames(13, cam, [16 * 20] * 3, DEPTHS)
    grow, dyn = _renderer(cam), _renderer(cam, dynamic=True)
    for i in range(3):
        grow.add(_t(pts[i]), _t(cols[i]))
        dyn.add(_t(pts[i]), _t(cols[i]))
        shot = _renderer(cam)
        shot.add(_t(np.concatenate(pts[:i + 1])), _t(np.concatenate(cols[:i + 1])))
        fresh = _renderer(cam)
        fresh.add(_t(pts[i]), _t(cols[i]))
        for a, b in ((grow, shot), (dyn, fresh)):
            for x, y in zip(a.image(True, True), b.image(True, True)):
                assert torch.equal(x, y)
        _check_exact(dyn, [pts[i]], [cols[i]], cam)
    assert grow.count == 960 and dyn.count == 320


@gpu
def test_in_kernel_confidence_mask():
    cam = _cam(61, 47)
    pts, cols = _frames(14, cam, [16 * 20] * 2, DEPTHS)
    rng = np.random.default_rng(15)
    thresh = np.float32(0.5)
    confs = [rng.uniform(1.0, 4.0, 320).astype(np.float32) for _ in range(2)]
    confs[0][:4] = (2.0, 1.0, np.nextafter(np.float32(2.0), np.float32(3.0)), 1.0)       # (2 - 1) / 2 = 0.5 exactly: NOT above; conf = 1 -> 0
    keeps = [(c.astype(np.float32) - np.float32(1)) / c > thresh for c in confs]
    assert not keeps[0][0] and not keeps[0][1] and keeps[0][2] and 0.2 < np.mean(keeps[0]) < 0.8
    masked = _renderer(cam, conf_thresh=float(thresh))
    filtered = _renderer(cam)
    for p, c, cf, k in zip(pts, cols, confs, keeps):
        masked.add(_t(p), _t(c), _t(cf))
        filtered.add(_t(p[k]), _t(c[k]))
    index = _check_exact(masked, pts, cols, cam, keep=np.concatenate(keeps))
    rgb_m, depth_m, index_m = _image(masked)
    rgb_f, depth_f, index_f = _image(filtered)
    fmap = np.flatnonzero(np.concatenate(keeps))                                       # filtered index -> original index
    assert np.array_equal(np.where(index_f >= 0, fmap[np.maximum(index_f, 0)], -1), index_m)
    assert np.array_equal(rgb_m, rgb_f) and np.array_equal(depth_m, depth_f)
    assert masked.count == 640 and filtered.count == int(np.concatenate(keeps).sum())


@gpu
@pytest.mark.parametrize("ps", [3, 4])
def test_point_size_clipped_footprints_and_guards(ps):
    import torch
    W, H = 29, 23
    cam = _cam(W, H, point_size=ps)
    rng = np.random.default_rng(16 + ps)
    edge = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2), (1, 1), (W - 2, H - 2)]
    inner = [(int(a), int(b)) for a, b in zip(rng.integers(0, W, 40), rng.integers(0, H, 40))]
    tu, tv = np.array(edge + inner).T
    # just outside the image too: a footprint that reaches back in must draw its inside part (bad = 0: no culled points here)
    tu, tv = np.concatenate((tu, [-1, W, 5, 7])), np.concatenate((tv, [3, 4, -1, H]))
    pts = _safe_points(rng, cam, len(tu), DEPTHS, bad=0.0, targets=(tu, tv))
    cols = _colors(rng, len(tu))
    _assert_safe(pts, cam)
    r = _renderer(cam)
    pad, sentinel = 256, 0x0123456789abcdef
    guard = torch.full((2 * pad + W * H,), sentinel, dtype=torch.int64, device="cuda")
    r.keys = guard[pad:pad + W * H]
    r.clear()
    r.add(_t(pts), _t(cols))
    index = _check_exact(r, [pts], [cols], cam)
    assert (index >= 0).sum() > len(inner), "footprints should cover more pixels than there are points"
    assert bool((guard[:pad] == sentinel).all()) and bool((guard[pad + W * H:] == sentinel).all())


@gpu
@pytest.mark.parametrize("n", [1, 321, 0])
def test_awkward_counts(n):
    cam = _cam(61, 47)
    pts, cols = _frames(20 + n, cam, [n], DEPTHS, bad=0.0)
    r = _renderer(cam)
    r.add(_t(pts[0]), _t(cols[0]))
    index = _check_exact(r, pts, cols, cam)
    assert (index >= 0).any() == (n > 0) and r.count == n


@gpu
def test_full_size_resolve():
    cam = _cam(1920, 1080)
    pts, cols = _frames(30, cam, [224 * 224] * 4, DEPTHS)
    r = _renderer(cam)
    for p, c in zip(pts, cols):
        r.add(_t(p), _t(c))
    index = _check_exact(r, pts, cols, cam)
    assert (index >= 0).sum() > 150000


@gpu
def test_determinism_and_arrival_order():
    import torch
    cam = _cam(61, 47)
    pts, cols = _frames(17, cam, [16 * 20] * 3, DEPTHS)

    def run(ps, cs):
        r = _renderer(cam)
        for p, c in zip(ps, cs):
            r.add(_t(p), _t(c))
        return r.image(True, True)
    a, b = run(pts, cols), run(pts, cols)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    rev = run([p[::-1] for p in pts], [c[::-1] for c in cols])
    assert torch.equal(a[1], rev[1])                                   # depth: identical everywhere
    fwd_i, _ = RR.render(np.concatenate(pts), cam)
    rev_i, _ = RR.render(np.concatenate([p[::-1] for p in pts]), cam)
    back = np.concatenate([np.arange(320)[::-1] + 320 * i for i in range(3)])      # reversed-order index -> original index
    same = np.where(rev_i >= 0, back[np.maximum(rev_i, 0)], -1) == fwd_i             # the same point wins: away from ties
    assert 0.5 < same.mean() < 1.0
    assert np.array_equal(a[0].cpu().numpy()[same], rev[0].cpu().numpy()[same])


@gpu
def test_colorize_lut(fx):
    import torch
    from spann3r_amd import vis
    rng = np.random.default_rng(18)
    x = np.concatenate((rng.random(4096, dtype=np.float32), np.array([0.0, 1.0 - 2.0 ** -24, 1.0, -0.1], np.float32)))
    lut = fx["jet_lut"]
    want = lut[np.minimum(np.maximum((x * np.float32(256)).astype(np.int64), 0), 255)]
    assert np.array_equal(want[-4:], lut[[0, 255, 255, 0]])
    got = vis.colorize_lut(_t(x), _t(lut)).cpu().numpy()
    assert got.shape == (4100, 4) and np.array_equal(got, want)


@gpu
def test_colorize_hsv(fx):
    from spann3r_amd import vis
    got = vis.colorize_hsv(_t(fx["hsv_x"])).cpu().numpy().astype(np.int64)
    diff = np.abs(got - fx["hsv_rgb"].astype(np.int64))
    print("entries off the fixture: %d (mask holds %d)" % ((diff > 0).sum(), fx["hsv_near"].sum()))
    assert diff.max() <= 1 and not np.any((diff > 0) & ~fx["hsv_near"])


@gpu
def test_end_to_end_tiny(tmp_path, tiny_sd):
    import torch
    from PIL import Image
    from spann3r_amd import Spann3R, TINY, vis
    from spann3r_amd.weights import synth_frames
    m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False)
    m.load_state_dict(tiny_sd, strict=True)
    m = m.to("cuda:0").eval()
    frames = synth_frames(3, 64, 80)
    preds, _ = m([{"img": f["img"].to("cuda:0")} for f in frames])
    pts_all = torch.cat([p["pts3d" if j == 0 else "pts3d_in_other_view"] for j, p in enumerate(preds)]).float()
    conf_all = torch.cat([p["conf"] for p in preds]).float()
    images_all = (torch.cat([f["img"] for f in frames]).permute(0, 2, 3, 1).cuda() + 1.0) / 2.0
    images_all = torch.round(images_all * 255) / 255             # exact levels: packing has no rounding case
    conf_sig = (conf_all - 1) / conf_all
    cam = vis.fit_camera(pts_all, 320, 200)
    out = str(tmp_path)
    pics = vis.render_frames(pts_all, images_all, cam, out)
    maps = vis.vis_pred_and_imgs(pts_all, out, images_all=images_all, conf_all=conf_sig)
    assert pics.shape == (3, 200, 320, 3) and pics.dtype == torch.uint8 and pics.is_cuda
    for i in range(3):
        for name, want in (("render_frames/frame_%03d.png" % i, pics[i]), ("pts/pts_%04d.png" % i, maps["pts"][i]),
                           ("imgs/img_%04d.png" % i, maps["imgs"][i]), ("confs/conf_%04d.png" % i, maps["confs"][i])):
            assert np.array_equal(np.asarray(Image.open(os.path.join(out, name))), want.cpu().numpy()), name
    back = vis.load_camera(os.path.join(out, "render_frames", "camera.json"))
    assert back.extrinsic.tobytes() == cam.extrinsic.tobytes() and back.intrinsic.tobytes() == cam.intrinsic.tobytes()
    assert maps["pts"].shape == (3, 64, 80, 3) and maps["confs"].shape == (3, 64, 80, 4)
    # the pictures against the restatement on the same predictions, general-pose comparison; pixels that a point within 1e-3 px of a
    # rounding boundary could reach are skipped, and stay under 1 % of the picture
    ref = RR.Cam(cam.extrinsic[:3, :3], cam.extrinsic[:3, 3], cam.intrinsic[0, 0], cam.intrinsic[1, 1], cam.intrinsic[0, 2], cam.intrinsic[1, 2], 320, 200)
    P, Cc = pts_all.cpu().numpy().reshape(3, -1, 3), images_all.cpu().numpy().reshape(3, -1, 3)
    for i in range(3):
        allp, allc = P[:i + 1].reshape(-1, 3), Cc[:i + 1].reshape(-1, 3)
        index, _ = RR.render(allp, ref)
        u, v, _, ok = RR.project(allp, ref)
        near = np.flatnonzero(RR.boundary_distance(allp, ref) < 1e-3)
        skip = np.zeros((200, 320), bool)
        for k in near:                       # the pixels on either side of the boundary
            xs = {int(np.floor(u[k] + 0.5 + e)) for e in (-1e-3, 1e-3)}
            ys = {int(np.floor(v[k] + 0.5 + e)) for e in (-1e-3, 1e-3)}
            for x in xs:
                for y in ys:
                    if 0 <= x < 320 and 0 <= y < 200:
                        skip[y, x] = True
        assert skip.mean() < 0.01
        assert (index >= 0).sum() > 100, "the fitted camera should see the cloud"
        assert np.array_equal(pics[i].cpu().numpy()[~skip], RR.resolve(index, allc)[~skip])


@gpu
def test_errors_are_named():
    import torch
    from spann3r_amd import lib, vis
    cam = _cam(16, 8)
    r = _renderer(cam)
    good_p, good_c = torch.zeros(5, 3, device="cuda"), torch.zeros(5, 3, device="cuda")
    with pytest.raises(RuntimeError, match="PointRenderer.add: pts.*no CPU path"):
        r.add(torch.zeros(5, 3), good_c)
    with pytest.raises(RuntimeError, match="PointRenderer.add: mismatched lengths: 5 points, 4 colours"):
        r.add(good_p, good_c[:4])
    with pytest.raises(RuntimeError, match="mismatched lengths: 5 points, 3 confidences"):
        _renderer(cam, conf_thresh=0.1).add(good_p, good_c, torch.ones(3, device="cuda"))
    for ps in (0, 9):
        with pytest.raises(RuntimeError, match="sp3_render_splat failed.*point_size %d outside 1..8" % ps):
            vis.PointRenderer(camera=_vis_camera(cam), point_size=ps)
    l = lib.load()
    keys = torch.empty(16 * 8, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="sp3_render_splat failed.*index overflow"):
        lib.check(l.sp3_render_splat(good_p.data_ptr(), 0, 0.0, 1, 2 ** 32 - 2, ctypes.byref(r.cam), keys.data_ptr(), lib.stream_ptr()), "sp3_render_splat")
    assert l.sp3_render_splat(good_p.data_ptr(), 0, 0.0, 1, 2 ** 32 - 3, ctypes.byref(r.cam), keys.data_ptr(), lib.stream_ptr()) == 0
    with pytest.raises(RuntimeError, match="render_frames: pts_all"):
        vis.render_frames(torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2, 3), _vis_camera(cam))
    torch.cuda.synchronize()
