"""RGB-D views on the device (spann3r_amd/views.py, csrc/views.hip): build_views against what the reference's own data-set path
produced (tests/golden/views_rgbd.npz), the kernel's launch shapes against the numpy restatement (tests/views_ref.py), the views
as input of the training criterion, and the launch count under a side stream."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from spann3r_amd import views as V

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import views_ref as VR  # noqa: E402
from test_views_cpu import case_inputs, fixture_cases, sanitising  # noqa: E402

pytestmark = pytest.mark.gpu


def build_case(g, name, **kw):
    cfg, raws, Ks, poses = case_inputs(g, name)
    rgbs = [VR.seeded_image(r.shape[0], r.shape[1], int(s)) for r, s in zip(raws, g[name + "_rgb_seed"])]
    return V.build_views(rgbs, raws, Ks, list(poses), resolution=tuple(cfg["resolution"]), rng=np.random.default_rng(cfg["seed"]),
                         aug_crop=cfg["aug_crop"], **sanitising(cfg), **kw)


def check_world(pts, xcam, pose, where):
    exact, unit = VR.world_bound(xcam, pose)
    units = float((np.abs(pts.astype(np.float64) - exact) / unit).max())
    print("%s: world error %.2f units of 2^-24 (sum |R||X| + |t|), bound 4" % (where, units))
    assert units <= 4.0, (where, units)


def test_build_views_equals_the_reference_on_every_fixture_case():
    g, names = fixture_cases()
    for name in names:
        views = build_case(g, name, debug_xcam=True)
        assert len(views) == len(g[name + "_pose"])
        for i, v in enumerate(views):
            where = "%s[%d]" % (name, i)
            for k in ("img", "depthmap", "valid_mask", "camera_intrinsics", "camera_pose", "pts3d"):
                assert v[k].is_cuda and v[k].shape == (1,) + g["%s_%s" % (name, k)][i].shape, (where, k)
            assert v["true_shape"].dtype == torch.int32 and not v["true_shape"].is_cuda
            assert v["valid_mask"].dtype == torch.bool and v["img"].shape[2] <= v["img"].shape[3]
            for k in ("depthmap", "camera_intrinsics", "camera_pose", "img", "true_shape"):          # bit-equal
                assert v[k][0].cpu().numpy().tobytes() == g["%s_%s" % (name, k)][i].tobytes(), (where, k)
            mask = g[name + "_valid_mask"][i]
            assert np.array_equal(v["valid_mask"][0].cpu().numpy(), mask), where
            xcam = v["pts3d_cam"][0].cpu().numpy()
            ref_xcam = g[name + "_xcam"][i]
            assert xcam[mask].tobytes() == ref_xcam[mask].tobytes() and np.array_equal(xcam, ref_xcam), where
            check_world(v["pts3d"][0].cpu().numpy(), ref_xcam, g[name + "_pose"][i], where)
            assert (v["idx"], v["instance"], v["label"], v["dataset"]) == (i, str(i), str(i), "rgbd")


def _frame(h, w, seed, kind="f32", fx=70.0):
    rng = np.random.default_rng(seed)
    K = np.array([[fx, 0, w / 2 - 0.3], [0, fx + 1, h / 2 + 0.4], [0, 0, 1]], np.float32)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = q, rng.uniform(-2, 2, 3)
    if kind == "u16":
        d = rng.integers(0, 6000, (h, w)).astype(np.uint16)
        d[rng.random((h, w)) < 0.1] = 65535
    else:
        d = rng.uniform(0.0, 5.0, (h, w)).astype(np.float32)
        d[rng.random((h, w)) < 0.1] = 0
    return VR.seeded_image(h, w, seed), d, K, T


def _against_ref(frames, resolution, **kw):
    """build_views on seeded frames == views_ref with the same plans (depth, mask, camera points and world points EXACTLY: the
    restatement rounds every fp32 operation as the kernel does)"""
    views = V.build_views(*[list(x) for x in zip(*frames)], resolution=resolution, debug_xcam=True, **kw)
    assert len(views) == len(frames)
    for i, ((rgb, d, K, T), v) in enumerate(zip(frames, views)):
        p = V.plan_rgbd_view(d.shape[0], d.shape[1], K, resolution)
        z, xcam, pts, mask = VR.view_depth_ref(d, p, T, **kw)
        assert v["depthmap"][0].cpu().numpy().tobytes() == z.tobytes(), i
        assert np.array_equal(v["valid_mask"][0].cpu().numpy(), mask), i
        assert np.array_equal(v["pts3d_cam"][0].cpu().numpy(), xcam), i
        assert np.array_equal(v["pts3d"][0].cpu().numpy(), pts), i
        check_world(v["pts3d"][0].cpu().numpy(), xcam, T, "view %d" % i)
        assert v["camera_intrinsics"][0].cpu().numpy().tobytes() == p["camera_intrinsics"].tobytes()
    return views


def test_one_view_of_one_pixel():
    views = _against_ref([_frame(9, 11, 1)], (1, 1))
    assert views[0]["pts3d"].shape == (1, 1, 1, 3)


def test_width_no_multiple_of_the_pixel_tile():
    """29 x 21 = 609 pixels: odd, so the one-pixel-per-lane kernel, three blocks, a ragged last one; 30 x 22 = 660 pixels: the
    four-pixel kernel with groups that straddle rows (30 is no multiple of 4) and a last wave that is partly idle"""
    _against_ref([_frame(50, 66, 2), _frame(47, 61, 3)], (29, 21))
    _against_ref([_frame(50, 66, 4), _frame(80, 58, 5)], (30, 22))            # the second view is a portrait: transposed stores


def test_mixed_sizes_and_dtypes_in_one_call():
    frames = [_frame(48, 64, 6, "u16"), _frame(60, 44, 7, "f32"), _frame(37, 53, 8, "u16"), _frame(52, 52, 9, "f32")]
    before = V.LAUNCHES["sp3_view_depth"]
    _against_ref(frames, (32, 24), depth_div=1000.0, raw_invalid=65535, min_depth=1e-3, max_depth=4.5)
    assert V.LAUNCHES["sp3_view_depth"] == before + 1


def test_seventeen_views():
    _against_ref([_frame(40 + s, 56 + (s % 3), 10 + s, "u16" if s % 2 else "f32") for s in range(17)], (16, 12), depth_div=2.0)


def test_all_zero_depth_gives_an_empty_mask_and_finite_points():
    rgb, d, K, T = _frame(48, 64, 30)
    views = _against_ref([(rgb, np.zeros_like(d), K, T), (rgb, d, K, T)], (32, 24))
    assert not views[0]["valid_mask"].any() and torch.isfinite(views[0]["pts3d"]).all()
    assert torch.equal(views[0]["pts3d"][0, 0, 0].cpu(), torch.from_numpy(T[:3, 3]))
    assert views[1]["valid_mask"].any()


def test_bad_inputs_raise():
    rgb, d, K, T = _frame(48, 64, 31)
    with pytest.raises(TypeError):
        V.build_views([rgb], [d.astype(np.float64)], [K], [T], resolution=(32, 24))
    with pytest.raises(ValueError):
        V.build_views([rgb], [d[:-1]], [K], [T], resolution=(32, 24))
    with pytest.raises(ValueError):
        V.build_views([rgb, rgb], [d], [K], [T], resolution=(32, 24))
    Tn = T.copy(); Tn[0, 3] = np.nan
    with pytest.raises(ValueError):
        V.build_views([rgb], [d], [K], [Tn], resolution=(32, 24))


def test_stacked_sequences_feed_the_training_criterion():
    """two built sequences, stacked to B = 2, give the loss that the reference's own views give"""
    from spann3r_amd.loss import ConfLoss_t, Regr3D_t, L21
    g, _ = fixture_cases()
    names = ("landscape", "uint16")
    built = V.stack_sequences([build_case(g, n) for n in names])
    assert len(built) == 3 and built[0]["pts3d"].shape == (2, 24, 32, 3) and built[1]["label"] == ["1", "1"]
    ref = [{k: torch.from_numpy(np.stack([g["%s_%s" % (n, k)][i] for n in names])).cuda() for k in ("pts3d", "valid_mask", "camera_pose")}
           for i in range(3)]
    gen = torch.Generator().manual_seed(0)
    preds_all = []
    for i in range(2):
        pair = []
        for key, j in (("pts3d", i), ("pts3d_in_other_view", i + 1)):
            pts = ref[j]["pts3d"].cpu() + 0.05 * torch.randn(2, 24, 32, 3, generator=gen)
            pair.append({key: pts.cuda(), "conf": (1 + torch.rand(2, 24, 32, generator=gen)).cuda()})
        preds_all.append(tuple(pair))
    crit = ConfLoss_t(Regr3D_t(L21, norm_mode="avg_dis", fix_first=False), alpha=0.4)
    a = crit.compute_frame_loss(built, preds_all)
    b = crit.compute_frame_loss(ref, preds_all)
    # masks, poses and depths are equal; the world points differ from the reference's by roundings of its einsum (<= 4 units of
    # 2^-24), so the two losses agree to the tolerances tests/test_loss.py holds this criterion to against the reference
    print("loss from built views %.9g, from the reference's views %.9g" % (float(a[0]), float(b[0])))
    assert math.isfinite(float(a[0])) and abs(float(a[0]) - float(b[0])) < 1e-5 * abs(float(b[0]))
    assert abs(float(a[2]) - float(b[2])) < 1e-6 + 1e-5 * abs(float(b[2]))
    for k, v in b[1].items():
        assert abs(a[1][k] - v) < 2e-5 * max(1.0, abs(v)), k


def test_one_depth_launch_per_call_on_a_side_stream():
    g, _ = fixture_cases()
    torch.cuda.synchronize()
    want = build_case(g, "offcentre")
    s = torch.cuda.Stream()
    before = V.LAUNCHES["sp3_view_depth"]
    calls = []
    real = torch.cuda.synchronize
    torch.cuda.synchronize = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        with torch.cuda.stream(s):
            got = build_case(g, "offcentre")
    finally:
        torch.cuda.synchronize = real
    assert V.LAUNCHES["sp3_view_depth"] == before + 1 and not calls
    s.synchronize()
    for a, b in zip(want, got):
        for k in ("img", "depthmap", "pts3d", "valid_mask"):
            assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ evaluation from views
def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rel(got, want, scale, where):
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) / scale
    print("%s: %.3g of max |gt|" % (where, err))
    return err


@pytest.fixture(scope="module")
def align_cases():
    from test_views_cpu import eval_align_fixture
    g, meta = eval_align_fixture()
    out = []
    for tag, m in meta.items():
        case = VR.eval_align_case(m["seed"])
        assert VR.eval_align_digest(case) == m["digest"]
        out.append((tag, m, case, VR.eval_align_batch(case, _cuda)))
    return g, out


def test_get_all_pts3d_t_equals_the_reference(align_cases):
    from spann3r_amd.loss import L21, Regr3D_t_ScaleShiftInv
    g, cases = align_cases
    crit = Regr3D_t_ScaleShiftInv(L21, norm_mode=False, gt_scale=True)
    for tag, m, case, (views, preds, preds_all) in cases:
        gt_pts, (pred_l, pred_r), gt_factor, pr_factor, masks, monitoring = crit.get_all_pts3d_t(views, preds_all)
        assert gt_factor is None and pr_factor is None and len(gt_pts) == 4 and len(pred_l) == len(pred_r) == 3
        valid = case["masks"]
        assert all(torch.equal(a.cpu(), torch.from_numpy(b[None])) for a, b in zip(masks, valid))
        print("D = %.3g" % m["D"])
        for k, want in zip(m["monitoring"], g[tag + "_monitoring"]):
            print(k, float(monitoring[k]), float(want))
            assert abs(float(monitoring[k]) - want) < 2e-5 * max(1.0, abs(want)), (tag, k)
        for k, got, frames in (("gt_pts", gt_pts, slice(0, 4)), ("pred_l", pred_l, slice(0, 3)), ("pred_r", pred_r, slice(1, 4))):
            got = torch.cat(got).cpu().numpy()
            assert got.shape == g["%s_%s" % (tag, k)].shape and np.isfinite(got).all()
            err = _rel(got[valid[frames]], g["%s_%s" % (tag, k)][valid[frames]], m["max_abs_gt"], tag + " " + k)
            assert err <= 4 * m["D"], (tag, k, err, m["D"])
    with pytest.raises(NotImplementedError):
        Regr3D_t_ScaleShiftInv(L21, gt_scale=True).get_all_pts3d_t(views, preds_all)
    with pytest.raises(NotImplementedError):
        crit.compute_frame_loss(views, preds_all)


def test_align_to_ground_truth_equals_the_reference(align_cases):
    from spann3r_amd.evaluate import align_to_ground_truth
    g, cases = align_cases
    for tag, m, case, (views, preds, preds_all) in cases:
        a = align_to_ground_truth(views, preds, preds_all)
        valid = case["masks"]
        assert all(v.is_cuda for v in a.values())
        assert np.array_equal(a["masks_all"].cpu().numpy(), valid) and a["masks_all"].dtype == torch.bool
        assert np.array_equal(a["conf_all"].cpu().numpy(), case["conf"])
        assert np.array_equal(a["images_all"].cpu().numpy(), (case["img"].transpose(0, 2, 3, 1) + np.float32(1.0)) / np.float32(2.0))
        for k in ("pts_all", "pts_gt_all"):
            got = a[k].cpu().numpy()
            assert got.shape == (4, 24, 32, 3) and np.isfinite(got).all()
            err = _rel(got[valid], g["%s_%s" % (tag, k)][valid], m["max_abs_gt"], tag + " " + k)
            assert err <= 4 * m["D"], (tag, k, err, m["D"])
    two = [dict(v, pts3d=torch.cat([v["pts3d"]] * 2), valid_mask=torch.cat([v["valid_mask"]] * 2), camera_pose=torch.cat([v["camera_pose"]] * 2))
           for v in views]
    both = [tuple({k: torch.cat([x] * 2) for k, x in r.items()} for r in pair) for pair in preds_all]
    with pytest.raises(ValueError, match="batch size 1"):
        align_to_ground_truth(two, preds, both)


def test_evaluate_sequence(align_cases):
    from spann3r_amd.evaluate import evaluate_reconstruction, evaluate_sequence
    g, cases = align_cases
    tag, m, case, (views, preds, preds_all) = cases[0]
    valid = case["masks"]
    r = evaluate_sequence(views, preds, preds_all, threshold=0.1)
    # lengths and order of the compaction: exact
    assert np.array_equal(r["cloud_index"].cpu().numpy(), np.flatnonzero(valid.ravel()))
    assert r["pred_cloud"].shape == r["gt_cloud"].shape == r["cloud_colors"].shape == (int(valid.sum()), 3)
    for k, ref in (("pred_cloud", g[tag + "_pts_all"][valid]), ("gt_cloud", g[tag + "_pts_gt_all"][valid])):
        assert _rel(r[k].cpu().numpy(), ref, m["max_abs_gt"], tag + " " + k) <= 4 * m["D"]
    assert np.array_equal(r["cloud_colors"].cpu().numpy(), ((case["img"].transpose(0, 2, 3, 1) + np.float32(1.0)) / np.float32(2.0))[valid])
    again = evaluate_reconstruction(r["pred_cloud"], r["gt_cloud"], 0.1)
    for k, v in again.items():
        assert np.array_equal(np.asarray(r[k]), np.asarray(v)), k
    assert math.isfinite(r["acc"]) and math.isfinite(r["comp"]) and 0.0 <= r["nc1"] <= 1.0
    print({k: r[k] for k in ("acc", "comp", "nc1", "nc2")})
    empty = [dict(v, valid_mask=torch.zeros_like(v["valid_mask"])) for v in views]
    with pytest.raises(ValueError, match="no valid pixel"):
        evaluate_sequence(empty, preds, preds_all)
