"""RGB-D views, host side (spann3r_amd/views.py): the crop plan for real intrinsics and the frame sampling against what the
reference's own functions produced (tests/golden/views_rgbd.npz, views_sampling.json; make_golden_views.py), and the numpy
restatement of the kernel's rules (tests/views_ref.py) against the same fixture."""
import json
import os
import sys

import numpy as np
import pytest

from spann3r_amd import preprocess as PP
from spann3r_amd import views as V

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import views_ref as VR  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_cases():
    g = np.load(os.path.join(GOLDEN, "views_rgbd.npz"))
    return g, [str(n) for n in g["names"]]


def case_inputs(g, name):
    cfg = json.loads(str(g[name + "_cfg"]))
    n = len(g[name + "_pose"])
    raws = [g["%s_raw%d" % (name, i)] for i in range(n)]
    Ks = [g["%s_K%d" % (name, i)] for i in range(n)]
    return cfg, raws, Ks, g[name + "_pose"]


def case_plans(g, name):
    """the plans of one fixture case, drawn from one generator in view order as the data set does"""
    cfg, raws, Ks, _ = case_inputs(g, name)
    rng = np.random.default_rng(cfg["seed"])
    return [V.plan_rgbd_view(r.shape[0], r.shape[1], K, tuple(cfg["resolution"]), rng, cfg["aug_crop"]) for r, K in zip(raws, Ks)]


def sanitising(cfg):
    return {k: cfg[k] for k in ("depth_div", "raw_invalid", "min_depth", "max_depth")}


def test_plan_equals_the_references_own_calls():
    g, names = fixture_cases()
    assert len(names) >= 8
    portraits = coins = 0
    for name in names:
        plans = case_plans(g, name)
        for i, p in enumerate(plans):
            want = g[name + "_plan"][i].tolist()
            assert list(p["crop0"]) + list(p["resize"]) + list(p["crop1"]) == want, (name, i, p)
            h, w = g[name + "_true_shape"][i].tolist()
            assert p["out"] == (w, h) and p["transpose"] == (h > w)
            K = p["camera_intrinsics"]
            assert K.dtype == np.float32 and K.tobytes() == g[name + "_camera_intrinsics"][i].tobytes(), (name, i)
            portraits += h > w
        coins += name.startswith("square") and len({p["transpose"] for p in plans}) == 2
    assert portraits >= 4 and coins >= 1          # permuted K rows and both outcomes of the coin are in the fixture


def test_bad_principal_point():
    K = np.array([[50.0, 0, 10.0], [0, 50.0, 24.0], [0, 0, 1]], np.float32)
    with pytest.raises(ValueError, match="Bad principal point: column"):
        V.plan_rgbd_view(48, 64, K, (32, 24))
    K = np.array([[50.0, 0, 32.0], [0, 50.0, 40.0], [0, 0, 1]], np.float32)
    with pytest.raises(ValueError, match="Bad principal point: row"):
        V.plan_rgbd_view(48, 64, K, (32, 24))
    with pytest.raises(ValueError):
        V.plan_rgbd_view(48, 64, np.eye(3), (24, 32))
    with pytest.raises(ValueError):
        V.plan_rgbd_view(48, 64, np.array([[50.0, 0, 32], [0, 50, 24], [0, 0, 1]]), (32, 24), aug_crop=8)


def test_centred_intrinsics_give_the_demo_plan():
    g = np.load(os.path.join(GOLDEN, "crop_plan.npz"))
    tags = sorted({k.rsplit("_", 1)[0] for k in g.files if k.endswith("_hw")})
    assert len({t.split("_s")[0] for t in tags}) == 12
    for t in tags:
        H, W = (int(v) for v in g[t + "_hw"])
        res = tuple(int(v) for v in g[t + "_res"])
        seed = int(t.split("_s")[1])
        K = np.array([[1.0, 0, W // 2], [0, 1.0, H // 2], [0, 0, 1]], dtype=np.float32)
        a = V.plan_rgbd_view(H, W, K, res, np.random.default_rng(seed))
        b = PP.plan_view(H, W, res, np.random.default_rng(seed))
        assert {k: a[k] for k in b} == b, t
        assert a["K_crop"].tobytes() == g[t + "_K"].tobytes(), t


def test_sampling_draw_for_draw():
    rows = json.load(open(os.path.join(GOLDEN, "views_sampling.json")))
    assert len(rows) >= 30
    for r in rows:
        names = ["%06d" % i for i in range(r["length"])]
        args = (r["num_frames"], r["min_thresh"], r["max_thresh"], r["train_ratio"])
        rng = np.random.default_rng(r["seed"])
        assert V.sample_frame_idx(names, rng, *args) == r["picked"], r
        assert int(rng.integers(1 << 30)) == r["next_draw"], r             # consumed exactly the reference's draws
        idx = V.sample_frames(r["length"], *args, np.random.default_rng(r["seed"]))
        assert [names[i] for i in idx] == r["picked"] and all(type(i) is int for i in idx)
        assert V.sample_frame_idx(names, None, *args, full_video=True, kf_every=r["kf_every"]) == r["full_video"]


def test_views_ref_equals_the_reference():
    g, names = fixture_cases()
    worst = 0.0
    for name in names:
        cfg, raws, _, poses = case_inputs(g, name)
        for i, p in enumerate(case_plans(g, name)):
            z, xcam, pts, mask = VR.view_depth_ref(raws[i], p, poses[i], **sanitising(cfg))
            assert z.tobytes() == g[name + "_depthmap"][i].tobytes(), (name, i)
            assert np.array_equal(mask, g[name + "_valid_mask"][i]), (name, i)
            ref_xcam = g[name + "_xcam"][i]
            assert np.array_equal(xcam[mask], ref_xcam[mask]) and np.array_equal(xcam, ref_xcam), (name, i)
            exact, unit = VR.world_bound(ref_xcam, poses[i])
            for got in (pts, g[name + "_pts3d"][i]):
                units = float((np.abs(got.astype(np.float64) - exact) / unit).max())
                worst = max(worst, units)
                assert units <= 4.0, (name, i, units)
    print("worst world error: %.2f units of 2^-24 (sum |R||X| + |t|)" % worst)


def test_the_fixture_tells_the_two_index_rules_apart():
    """floor(x * src / dst), the rule of the stub in make_golden.py, must FAIL on the fixture in at least two cases"""
    g, names = fixture_cases()

    def other(dst, src):
        return (np.arange(dst) * src / dst).astype(int).clip(0, src - 1)
    told = 0
    real = VR.nearest_index
    try:
        VR.nearest_index = other
        for name in names:
            cfg, raws, _, poses = case_inputs(g, name)
            got = np.stack([VR.view_depth_ref(raws[i], p, poses[i], **sanitising(cfg))[0] for i, p in enumerate(case_plans(g, name))])
            told += not np.array_equal(got, g[name + "_depthmap"])
    finally:
        VR.nearest_index = real
    assert told >= 2, told


def eval_align_fixture():
    g = np.load(os.path.join(GOLDEN, "views_eval_align.npz"))
    return g, json.loads(str(g["meta"]))


def test_alignment_restatement_equals_the_reference():
    """tests/views_ref.py eval_align_ref in float64 against the reference's float32 chain: within the fixture's own float32 error D
    (held to the 4 D of the device check), medians to the tolerance of tests/test_loss.py, clouds in the reference's order"""
    g, meta = eval_align_fixture()
    assert len(meta) == 2
    for tag, m in meta.items():
        case = VR.eval_align_case(m["seed"])
        assert VR.eval_align_digest(case) == m["digest"], "the seeded inputs changed: regenerate the fixture"
        r = VR.eval_align_ref(case)
        valid = case["masks"]
        for k in ("pts_all", "pts_gt_all", "gt_pts"):
            err = float(np.abs(r[k][valid] - g["%s_%s" % (tag, k)][valid]).max()) / m["max_abs_gt"]
            assert err <= 4 * m["D"], (tag, k, err, m["D"])
        for k, frames in (("pred_l", slice(0, 3)), ("pred_r", slice(1, 4))):
            err = float(np.abs(r[k][valid[frames]] - g["%s_%s" % (tag, k)][valid[frames]]).max()) / m["max_abs_gt"]
            assert err <= 4 * m["D"], (tag, k, err, m["D"])
        for k, want in zip(m["monitoring"], g[tag + "_monitoring"]):
            assert abs(r["monitoring"][k] - want) < 2e-5 * max(1.0, abs(want)), (tag, k)
        assert np.array_equal(r["cloud_index"], np.flatnonzero(valid.ravel())) and len(r["pred_cloud"]) == int(valid.sum())
        assert float(np.abs(r["pred_cloud"] - g[tag + "_pts_all"][valid]).max()) / m["max_abs_gt"] <= 4 * m["D"]
