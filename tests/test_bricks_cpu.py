"""The numpy restatement of the brick volume (tests/bricks_ref.py) checked against itself and against the dense restatement, and the
argument checks of spann3r_amd.fusion.BrickTSDFVolume that need no device.  No GPU."""
import numpy as np
import pytest
import torch

import bricks_ref as BR
import fusion_ref as FR
import raycast_ref as RC

S = BR.SCENE


@pytest.fixture(scope="module")
def frames():
    return BR.scene_frames("pts")


@pytest.fixture(scope="module")
def marked(frames):
    return BR.mark(frames, S["dims"], S["origin"], S["voxel"], S["band"], return_span=True)


@pytest.fixture(scope="module")
def fused(frames):
    """(the brick state after one integrate call of the six frames, the dense restatement of the same call on the full grid)"""
    state, grown = BR.integrate(BR.empty(S["dims"], 4096), frames, S["origin"], S["voxel"], S["trunc"], S["band"])
    assert grown == 0
    dense = FR.integrate_ref(*FR.empty_volume(S["dims"]), frames, np.float32(S["origin"]), np.float32(S["voxel"]), np.float32(S["trunc"]), np.float32)
    return state, dense


def test_scene_is_neither_empty_nor_full(marked, fused):
    flags, span = marked
    n = int(flags.sum())
    print("bricks", n, "of", flags.size, "span", span)
    assert flags.size == 11 * 9 * 6 and n <= 0.75 * flags.size and n >= 0.25 * flags.size          # at least 25 % absent
    assert span == 2                                                                              # no point spans more than 2 bricks per axis
    assert fused[0]["count"] == n


def test_mark_depth_path_matches_pts_path_up_to_rounding(marked):
    """the depth path rebuilds P from depth and pose in fp32: the same bricks except where a band face falls within that rounding"""
    flags_d = BR.mark(BR.scene_frames("depth"), S["dims"], S["origin"], S["voxel"], S["band"])
    differ = int((flags_d != marked[0]).sum())
    print("bricks that differ between the paths:", differ)
    assert differ <= 2 and flags_d.sum() > 0


def test_mark_skips_what_the_integrate_rule_skips():
    fr = dict(BR.scene_frames("pts")[0])
    P, ok = BR.frame_points(fr)
    assert ok.sum() > 100
    bad = dict(fr, pts=fr["pts"].copy(), valid=fr["valid"].copy(), pixel_weight=np.ones(ok.shape, np.float32))
    ys, xs = np.nonzero(ok)
    bad["pts"][ys[0], xs[0]] = np.nan                   # a non-finite point
    bad["valid"][ys[1], xs[1]] = 0
    bad["pixel_weight"][ys[2], xs[2]] = 0.0
    bad["pixel_weight"][ys[3], xs[3]] = np.inf
    bad["pts"][ys[4], xs[4]] = bad["pts"][ys[4], xs[4]] - 100.0 * np.asarray(fr["cam2world"])[:3, 2].astype(np.float32)      # behind the camera
    _, ok2 = BR.frame_points(bad)
    assert ok.sum() - ok2.sum() == 5
    far = dict(fr, pts=(fr["pts"] + np.float32(100.0)))      # every box misses the grid
    far["w2c"] = fr["w2c"].copy()
    far["w2c"][[3, 7, 11]] -= fr["w2c"].reshape(3, 4)[:, :3] @ np.full(3, 100.0, np.float32)
    assert BR.frame_points(far)[1].sum() == ok.sum()
    assert BR.mark([far], S["dims"], S["origin"], S["voxel"], S["band"]).sum() == 0


def test_allocation_order_is_the_sorted_marked_set(marked, fused):
    flags, _ = marked
    state = fused[0]
    want = sorted(int(b) for b in np.flatnonzero(flags))                                          # brute force
    assert state["slot_brick"][:state["count"]].tolist() == want
    assert (state["table"][want] == np.arange(len(want))).all() and (state["table"] >= 0).sum() == len(want)
    # a second round: new bricks go behind the old ones, again in brick order, and old ones keep their slots
    half = flags.copy()
    half[::2] = 0
    s1, f1, (c1, n1) = BR.alloc(BR.empty(S["dims"], 4096), half)
    s2, f2, (c2, n2) = BR.alloc(s1, flags)
    assert c1 == n1 == int(half.sum()) and c2 == n2 == len(want) and not f1.any() and not f2.any()
    assert s2["slot_brick"][:c1].tolist() == sorted(np.flatnonzero(half).tolist())
    assert s2["slot_brick"][c1:c2].tolist() == sorted(set(want) - set(np.flatnonzero(half).tolist()))


def test_alloc_is_all_or_nothing(marked):
    flags, _ = marked
    need = int(flags.sum())
    s0 = BR.empty(S["dims"], need - 1)
    s0["tsdf"][:] = 7.0                                                                           # (what a stale pool may hold)
    s1, f1, (count, n) = BR.alloc(s0, flags)
    assert (count, n) == (0, need) and np.array_equal(f1, flags)
    for k in ("table", "slot_brick", "tsdf", "weight", "rgb"):
        assert np.array_equal(s1[k], s0[k])
    s2, f2, (count, n) = BR.alloc(BR.grow(s1, 2 * (need - 1)), f1)                                # the caller grows and calls again
    assert (count, n) == (need, need) and not f2.any() and (s2["tsdf"][:need] == 1).all() and (s2["tsdf"][need:] == 0).all()


def test_masked_dense_identity(fused):
    """after ONE call every allocated voxel holds what the dense rule gives it on the full grid; absent voxels read (1, 0, 0)"""
    state, dense = fused
    D, W, col = BR.to_dense(state)
    slot, _ = BR._voxel_slots(state)
    ok = slot >= 0
    assert 0.25 < ok.mean() < 0.75
    for got, ref in ((D, dense[0]), (W, dense[1]), (col, dense[2])):
        assert np.array_equal(got[ok].view(np.uint32), ref[ok].view(np.uint32))
    assert (D[~ok] == 1).all() and (W[~ok] == 0).all() and (col[~ok] == 0).all()
    # the band covers the truncation: every voxel the dense call touched, less those whose brick no point came near, is allocated
    missed = (dense[1] > 0) & ~ok
    print("dense-observed voxels in absent bricks:", int(missed.sum()), "of", int((dense[1] > 0).sum()))
    sub = BR.to_dense(state, ((5, 3, 9), (30, 21, 17)))
    assert sub[0].shape == (17, 21, 30) and np.array_equal(sub[0], D[9:26, 3:24, 5:35]) and np.array_equal(sub[2], col[9:26, 3:24, 5:35])


def test_late_born_bricks_differ_from_the_dense_volume(frames):
    """two calls: a brick born in the second holds nothing of the first call's frames -- the restatement, not the dense volume, pins it"""
    state = BR.empty(S["dims"], 64)
    state, g1 = BR.integrate(state, frames[:3], S["origin"], S["voxel"], S["trunc"], S["band"])
    first = state["count"]
    state, g2 = BR.integrate(state, frames[3:], S["origin"], S["voxel"], S["trunc"], S["band"])
    assert g1 >= 1 and state["count"] > first
    dense = FR.integrate_ref(*FR.empty_volume(S["dims"]), frames, np.float32(S["origin"]), np.float32(S["voxel"]), np.float32(S["trunc"]), np.float32)
    slot, _ = BR._voxel_slots(state)
    D, W, _ = BR.to_dense(state)
    old, late = (slot >= 0) & (slot < first), slot >= first
    assert np.array_equal(W[old], dense[1][old]) and np.array_equal(D[old].view(np.uint32), dense[0][old].view(np.uint32))
    assert (W[late] != dense[1][late]).sum() > 0


def test_raycast_of_the_brick_volume_equals_the_dense_one(frames, fused):
    """the main view (frame 2): the band keeps everything the ray-caster can reach, so masking the bricks changes no pixel"""
    state, dense = fused
    view = BR.scene_view(frames[2])
    a = RC.raycast_ref(*BR.to_dense(state), np.float32(S["origin"]), np.float32(S["voxel"]), view, 1.0, None, np.float32)
    b = RC.raycast_ref(*dense, np.float32(S["origin"]), np.float32(S["voxel"]), view, 1.0, None, np.float32)
    print("hit", float(a["hit"].mean()))
    assert a["hit"].mean() >= 0.5
    assert np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))


def test_argument_errors_without_a_device():
    from spann3r_amd import fusion as F
    with pytest.raises(ValueError, match="three sizes"):
        F.BrickTSDFVolume((0, 0, 0), 0.1, (8, 8))
    with pytest.raises(ValueError, match="voxel_size"):
        F.BrickTSDFVolume((0, 0, 0), 0.0, (8, 8, 8))
    with pytest.raises(ValueError, match="trunc"):
        F.BrickTSDFVolume((0, 0, 0), 0.1, (8, 8, 8), trunc=-1.0)
    with pytest.raises(ValueError, match="band"):
        F.BrickTSDFVolume((0, 0, 0), 0.1, (8, 8, 8), band=0.9)                                    # over 8 voxels
    with pytest.raises(ValueError, match="band"):
        F.BrickTSDFVolume((0, 0, 0), 0.1, (8, 8, 8), band=0.0)
    with pytest.raises(ValueError, match="capacity"):
        F.BrickTSDFVolume((0, 0, 0), 0.1, (8, 8, 8), capacity=0)
    with pytest.raises(ValueError, match="origin"):
        F.BrickTSDFVolume((0, np.nan, 0), 0.1, (8, 8, 8))
    with pytest.raises(ValueError, match="index limit"):
        F.BrickTSDFVolume((0, 0, 0), 0.1, (2 ** 14, 2 ** 14, 2 ** 14))
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.BrickTSDFVolume((0, 0, 0), 0.1, (8, 8, 8), device="cpu")
    with pytest.raises(ValueError, match="extent"):
        F.brick_volume_for_extent(((0, 0, 0), (1, -1, 1)), 0.1)
    with pytest.raises(ValueError, match="voxel_size"):
        F.brick_volume_for_extent(((0, 0, 0), (1, 1, 1)), None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.FusionSession(0.1, ((0, 0, 0), (1, 1, 1)), device="cpu")
    pts, valid = torch.zeros(1, 4, 4, 3), torch.ones(1, 4, 4, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.fuse_pointmaps(pts, np.eye(3), np.eye(4)[None], valid, bricks=True, voxel_size=0.1)
