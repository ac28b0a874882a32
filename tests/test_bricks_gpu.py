"""spann3r_amd.fusion.BrickTSDFVolume and FusionSession on the device (csrc/bricks.hip; include/spann3r_hip.h "Brick TSDF volume").

Every comparison is bit for bit.  The anchors: tests/bricks_ref.py (mark, alloc, integrate, to_dense restated in numpy) for the
allocation and for what late-born bricks hold; the dense kernels -- TSDFVolume.integrate on the same grid, TSDFVolume.raycast and
track_frame on to_dense() of the full grid -- for the per-voxel rule and the ray-caster, which must not change a bit by going
through bricks or by passing over samples.  The scene is bricks_ref.SCENE: 376 of its 594 bricks exist and the main view hits on
72.9 % of its pixels (asserted from the restatement in tests/test_bricks_cpu.py and again below), so no comparison passes on an
empty or a full volume."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import bricks_ref as BR
import fusion_ref as FR
import raycast_ref as RC

pytestmark = pytest.mark.gpu

S = BR.SCENE
FULL = ((0, 0, 0), S["dims"])
SIZE = (S["h"], S["w"])


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _brick(capacity=4096, color=True, dims=None, origin=None):
    from spann3r_amd import fusion as F
    return F.BrickTSDFVolume(S["origin"] if origin is None else origin, S["voxel"], S["dims"] if dims is None else dims, trunc=S["trunc"],
                             band=S["band"], color=color, capacity=capacity)


def _args(frs, path="pts", images=True):
    kw = dict(intrinsics=[f["K"] for f in frs], cam2world=[f["cam2world"] for f in frs], valid=[_t(f["valid"]) for f in frs])
    kw[path] = [_t(f[path]) for f in frs]
    if images:
        kw["images"] = [_t(f["images"]) for f in frs]
    return kw


def _assert_state(vol, ref):
    """the device's table, slot_brick, count and pool against a restatement state"""
    n = ref["count"]
    assert vol.n_bricks == n and int(vol.count.cpu()) == n
    assert np.array_equal(vol.table.cpu().numpy(), ref["table"])
    assert np.array_equal(vol.slot_brick[:n].cpu().numpy(), ref["slot_brick"][:n])
    for name in ("tsdf", "weight", "rgb"):
        if ref[name] is not None:
            assert _bits(getattr(vol, name)[:n].cpu().numpy(), ref[name][:n]), name


def _same_pool(a, b):
    n = a.n_bricks
    return (b.n_bricks == n and torch.equal(a.table, b.table) and torch.equal(a.slot_brick[:n], b.slot_brick[:n]) and
            all(torch.equal(getattr(a, k)[:n].view(torch.int32), getattr(b, k)[:n].view(torch.int32)) for k in ("tsdf", "weight", "rgb")))


@pytest.fixture(scope="module")
def frames():
    return RC.scene_frames()


@pytest.fixture(scope="module")
def ref_one(frames):
    """the restatement after ONE integrate call of the six frames (pts)"""
    state, _ = BR.integrate(BR.empty(S["dims"], 4096), FR.as_path(frames, "pts"), S["origin"], S["voxel"], S["trunc"], S["band"])
    assert 0.25 * state["table"].size <= (state["table"] < 0).sum()                              # at least 25 % of the bricks absent
    return state


@pytest.fixture(scope="module")
def fused(frames):
    """(the brick volume after one call of the six frames, to_dense of the full grid)"""
    vol = _brick().integrate(**_args(frames))
    return vol, vol.to_dense(FULL)


# ------------------------------------------------------------------------------------------------ mark and alloc
@pytest.mark.parametrize("path", ["pts", "depth"])
def test_mark_and_alloc_equal_the_restatement(frames, path):
    frs = FR.as_path(frames, path)
    flags = BR.mark(frs, S["dims"], S["origin"], S["voxel"], S["band"])
    ref, f2, counts = BR.alloc(BR.empty(S["dims"], 4096), flags)
    vol = _brick().allocate(**_args(frames, path, images=False))
    print(path, "bricks", vol.n_bricks, "of", vol.table.numel())
    assert counts == (376, 376) and vol.launches == 0
    _assert_state(vol, ref)                                                                       # (the slots are initialised: 1, 0, 0)
    assert not vol.flags.any()
    assert vol._counts.cpu().tolist() == [376, 376]


def test_alloc_reports_need_and_writes_nothing_when_the_pool_is_short(frames, ref_one):
    """capacity exhaustion shows in the reported `need`; table, slots, pool, count and flags stay as they were"""
    from spann3r_amd import lib as L
    vol = _brick(capacity=375)
    tbl = vol.frame_table([_t(f["pts"]) for f in frames], False, [f["K"] for f in frames], [f["cam2world"] for f in frames],
                          [_t(f["valid"]) for f in frames], None, [_t(f["images"]) for f in frames])
    lib, st = L.load(), L.stream_ptr()
    nx, ny, nz = vol.dims
    L.check(lib.sp3_tsdf_brick_mark(tbl[0], tbl[1].data_ptr(), tbl[4].data_ptr(), tbl[2], nx, ny, nz, vol._origin_c, vol.voxel_size, vol.band,
                                    vol.flags.data_ptr(), st), "mark")
    flags = vol.flags.clone()
    vol.tsdf.fill_(7.0)
    vol.slot_brick.fill_(-5)
    L.check(lib.sp3_tsdf_brick_alloc(vol.flags.data_ptr(), nx, ny, nz, vol.table.data_ptr(), vol.slot_brick.data_ptr(), vol.count.data_ptr(),
                                     vol.capacity, vol.tsdf.data_ptr(), vol.weight.data_ptr(), L.ptr(vol.rgb), vol._ws.data_ptr(),
                                     vol._counts.data_ptr(), st), "alloc")
    assert vol._counts.cpu().tolist() == [0, 376] and int(vol.count.cpu()) == 0
    assert torch.equal(vol.flags, flags) and int(flags.sum()) == 376
    assert (vol.table == -1).all() and (vol.slot_brick == -5).all() and (vol.tsdf == 7.0).all()
    vol.allocate_table(tbl)                                                                       # marks again (the same flags), grows, allocates
    assert vol.grown == 1 and vol.capacity >= 376
    assert np.array_equal(vol.table.cpu().numpy(), ref_one["table"])


# ------------------------------------------------------------------------------------------------ integrate
def test_one_call_equals_the_dense_integrate_on_every_allocated_voxel(frames, fused, ref_one):
    from spann3r_amd import fusion as F
    vol, dense_of_bricks = fused
    assert vol.launches == 1 and vol.n_bricks == 376 and vol.grown == 0
    _assert_state(vol, ref_one)
    dense = F.TSDFVolume(S["origin"], S["voxel"], S["dims"], trunc=S["trunc"]).integrate(**_args(frames))
    slot, _ = BR._voxel_slots(ref_one)
    ok = slot >= 0
    for name in ("tsdf", "weight", "rgb"):
        a, b = getattr(dense_of_bricks, name).cpu().numpy(), getattr(dense, name).cpu().numpy()
        assert _bits(a[ok], b[ok]), name
        assert (a[~ok] == (1.0 if name == "tsdf" else 0.0)).all()
    assert (dense.weight.cpu().numpy()[ok] > 0).sum() > 50000


def test_depth_path_equals_the_dense_integrate(frames):
    from spann3r_amd import fusion as F
    vol = _brick(color=False).integrate(**_args(frames, "depth", images=False))
    dense = F.TSDFVolume(S["origin"], S["voxel"], S["dims"], trunc=S["trunc"], color=False).integrate(**_args(frames, "depth", images=False))
    got = vol.to_dense(FULL)
    ok = (vol.table.cpu().numpy() >= 0)
    slot, _ = BR._voxel_slots(dict(dims=S["dims"], bricks=vol.bricks, table=vol.table.cpu().numpy()))
    ok = slot >= 0
    assert vol.n_bricks == 376 and got.rgb is None
    assert _bits(got.tsdf.cpu().numpy()[ok], dense.tsdf.cpu().numpy()[ok]) and _bits(got.weight.cpu().numpy()[ok], dense.weight.cpu().numpy()[ok])


def test_two_calls_equal_the_restatement_and_late_bricks_differ_from_dense(frames):
    from spann3r_amd import fusion as F
    frs = FR.as_path(frames, "pts")
    ref, _ = BR.integrate(BR.empty(S["dims"], 4096), frs[:3], S["origin"], S["voxel"], S["trunc"], S["band"])
    first = ref["count"]
    ref, _ = BR.integrate(ref, frs[3:], S["origin"], S["voxel"], S["trunc"], S["band"])
    vol = _brick().integrate(**_args(frames[:3]))
    assert vol.n_bricks == first
    vol.integrate(**_args(frames[3:]))
    assert vol.launches == 2 and vol.n_bricks > first
    _assert_state(vol, ref)
    dense = F.TSDFVolume(S["origin"], S["voxel"], S["dims"], trunc=S["trunc"]).integrate(**_args(frames))
    slot, _ = BR._voxel_slots(ref)
    got, W = vol.to_dense(FULL).weight.cpu().numpy(), dense.weight.cpu().numpy()
    old, late = (slot >= 0) & (slot < first), slot >= first
    assert np.array_equal(got[old], W[old])
    print("voxels of late-born bricks that differ from the dense volume:", int((got[late] != W[late]).sum()))
    assert (got[late] != W[late]).sum() > 0                                                       # the restatement pins this case


def test_growth_from_a_small_pool_gives_the_same_state(frames, fused):
    vol = _brick(capacity=64).integrate(**_args(frames))
    assert vol.grown >= 1 and vol.capacity >= 376 and fused[0].grown == 0
    assert _same_pool(vol, fused[0])
    big = _brick().integrate(**_args(frames[:3]))
    two = _brick(capacity=big.n_bricks).integrate(**_args(frames[:3]))                            # a pool that is exactly full ...
    assert two.grown == 0 and two.capacity == two.n_bricks
    two.integrate(**_args(frames[3:]))                                                            # ... grows with every slot in use
    big.integrate(**_args(frames[3:]))
    assert two.grown == 1 and big.grown == 0 and two.n_bricks > two.capacity // 2 and _same_pool(two, big)


# ------------------------------------------------------------------------------------------------ ray-casting
def _assert_same_maps(vol, dense, K, P, **kw):
    """raycast of the brick volume against the dense ray-caster on to_dense(full grid): all four maps, bit for bit -> the hit share"""
    a, b = vol.raycast(K, P, SIZE, **kw), dense.raycast(K, P, SIZE, **kw)
    assert sorted(a) == ["colors", "depth", "normals", "vertices"]
    for k in a:
        x, y = a[k].contiguous(), b[k].contiguous()
        assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k
    return float((a["depth"] != 0).float().mean())


def test_raycast_six_views_in_one_launch(frames, fused):
    vol, dense = fused
    before = vol.raycasts
    hit = _assert_same_maps(vol, dense, [f["K"] for f in frames], [f["cam2world"] for f in frames], min_weight=1.0)
    main = float((vol.raycast(frames[2]["K"], frames[2]["cam2world"], SIZE)["depth"] != 0).float().mean())
    print("hit share: six views", hit, "main view", main)
    assert vol.raycasts == before + 2 and main >= 0.5


def test_raycast_from_inside_the_grid(frames, fused):
    P = FR.look_at((0.55, -0.45, 0.6), (-0.3, 0.2, 0.0))
    hit = _assert_same_maps(*fused, frames[0]["K"], P[None])
    print("hit share", hit)
    assert hit > 0.3


def test_raycast_that_misses_the_grid(frames, fused):
    P = FR.look_at((0.95, -1.25, 0.85), (3.0, -3.0, 2.0))
    assert _assert_same_maps(*fused, frames[0]["K"], P[None]) == 0.0


def test_raycast_axis_aligned_with_the_eye_on_a_brick_face(frames, fused):
    """looking straight down: the central column has dir_x == 0 exactly and eye.x = origin.x + 8 k voxel lies on a brick face"""
    eye_x = float(np.float32(S["origin"][0]) + np.float32(8 * 5) * np.float32(S["voxel"]))
    P = np.eye(4)
    P[:3, :3] = [[1, 0, 0], [0, -1, 0], [0, 0, -1]]
    P[:3, 3] = (eye_x, 0.0, 1.2)
    K = np.array([[40.0, 0, 32.0], [0, 39.0, 23.0], [0, 0, 1]])
    out = fused[0].raycast(K, P[None], SIZE)
    assert (out["vertices"][0, :, 32, 0][out["depth"][0, :, 32] != 0] == eye_x).all()             # the column never leaves the face
    hit = _assert_same_maps(*fused, K, P[None])
    print("hit share", hit)
    assert hit > 0.3


def test_raycast_with_near_inside_a_band_and_a_finite_far(frames, fused):
    fr = frames[2]
    z = float(fr["depth"][24, 32])
    full = _assert_same_maps(*fused, fr["K"], fr["cam2world"][None])
    hit = _assert_same_maps(*fused, fr["K"], fr["cam2world"][None], near=z - 0.03, far=z + 0.4)   # starts inside the surface's band
    print("hit share", hit, "of", full)
    assert 0.05 < hit < full


def test_raycast_step_and_min_weight(frames, fused):
    for kw in (dict(step_voxels=0.25), dict(step_voxels=2.5), dict(min_weight=2.0)):
        assert _assert_same_maps(*fused, frames[4]["K"], frames[4]["cam2world"][None], **kw) > 0.2


def test_raycast_of_a_colourless_volume_equals_the_dense_raycaster(frames):
    """k_brick_raycast<false> against k_tsdf_raycast<false> directly: depth, vertices and normals of one scene camera, bit for bit"""
    vol = _brick(color=False).integrate(**_args(frames, images=False))
    dense = vol.to_dense(FULL)
    assert vol.rgb is None and dense.rgb is None and vol.n_bricks == 376
    fr = frames[2]
    a, b = vol.raycast(fr["K"], fr["cam2world"][None], SIZE), dense.raycast(fr["K"], fr["cam2world"][None], SIZE)
    assert sorted(a) == sorted(b) == ["depth", "normals", "vertices"]
    for k in a:
        x, y = a[k].contiguous(), b[k].contiguous()
        assert x.shape == y.shape and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), k
    hit = float((a["depth"] != 0).float().mean())
    print("hit share", hit)
    assert hit >= 0.5                                                                             # (the main view: 72.9 % with colours)


def test_track_frame_on_bricks_equals_track_frame_on_the_dense_volume(frames):
    from spann3r_amd import fusion as F
    vol = _brick(color=False).integrate(**_args(frames[:3], images=False))
    dense = vol.to_dense(FULL)
    moved = RC.perturbed_frames(frames, RC.perturbations(7))[3]
    pts, valid = _t(moved["pts"]), _t(moved["valid"])
    Ta, ia = F.track_frame(vol, pts, valid, moved["K"], moved["cam2world"])
    Tb, ib = F.track_frame(dense, pts, valid, moved["K"], moved["cam2world"])
    print(ia)
    assert ia["tracked"] and ia["pairs"] > 500 and ia == ib and np.array_equal(Ta, Tb)
    assert RC.motion_size(Ta)[0] > 0.5                                                            # a real correction, not the identity


# ------------------------------------------------------------------------------------------------ to_dense and extraction
def test_to_dense_of_a_box_that_cuts_bricks(fused, ref_one):
    vol, _ = fused
    box = ((5, 3, 9), (30, 21, 17))
    got = vol.to_dense(box)
    ref = BR.to_dense(ref_one, box)
    assert got.dims == (30, 21, 17)
    assert _bits(got.tsdf.cpu().numpy(), ref[0]) and _bits(got.weight.cpu().numpy(), ref[1]) and _bits(got.rgb.cpu().numpy(), ref[2])
    assert (ref[1] > 0).any() and (ref[1] == 0).any()
    want = np.float32(S["origin"]) + np.float32(box[0]) * np.float32(S["voxel"])
    assert np.array_equal(got.origin, want)
    lo, size = vol.brick_box()
    assert all(l % 8 == 0 and s % 8 == 0 for l, s in zip(lo, size)) and vol.to_dense().dims == size
    with pytest.raises(ValueError, match="dims_limit"):
        vol.to_dense(FULL, dims_limit=64)
    with pytest.raises(ValueError, match="inside the grid"):
        vol.to_dense(((80, 0, 0), (16, 8, 8)))


def test_extract_mesh_equals_the_dense_extraction(fused):
    vol, _ = fused
    a, b = vol.extract_mesh(), vol.to_dense().extract_mesh()
    assert a["faces"].shape[0] > 5000 and a["vertices"].shape[0] > 2500
    for k in ("vertices", "colors", "faces"):
        assert torch.equal(a[k], b[k]), k
    assert np.array_equal(a["bounds"], b["bounds"])


# ------------------------------------------------------------------------------------------------ a 512^3 virtual grid
def test_the_scene_in_a_512_cubed_virtual_grid(frames):
    """The same scene mid-grid in 512^3 voxels (a dense volume of that size: 2.7 GB).  The scene's floor and walls run on past the
    88 x 72 x 48 grid, and a larger grid holds them too: fed all pixels it allocates 645 bricks against 376 and 4453 of the 18432
    pixels of the six scene views hit where the small grid has nothing (measured on the MI355X).  "The same scene" is therefore the
    pixels whose band box lies inside the small grid by a voxel; both volumes get those.  The origin moves by whole bricks, so the
    brick sets can differ only where a band face falls within fp32 rounding of a brick face (bound: 4 bricks).  The views start inside
    both grids: a ray that enters a lattice box from outside starts sampling at the box, so its samples sit at another phase in
    another box and a grazing pixel may legitimately flip; from inside both marches start at `near` and sample the same points."""
    lo = np.float64(np.float32(S["origin"])) + S["band"] + S["voxel"]
    hi = np.float64(np.float32(S["origin"])) + (np.asarray(S["dims"]) - 2) * S["voxel"] - S["band"]
    inner = [dict(f, valid=(f["valid"] != 0) & ((f["pts"] >= lo) & (f["pts"] <= hi)).all(-1)) for f in frames]
    kept = np.mean([f["valid"].mean() for f in inner])
    small = _brick().integrate(**_args(inner))
    shift = np.array([208, 216, 232])
    origin = np.float32(S["origin"]) - shift.astype(np.float32) * np.float32(S["voxel"])
    vol = _brick(dims=(512, 512, 512), origin=origin).integrate(**_args(inner))
    flags = BR.mark(FR.as_path(inner, "pts"), (512, 512, 512), origin, S["voxel"], S["band"])
    table = vol.table.cpu().numpy()
    assert np.array_equal(table >= 0, flags != 0) and vol.n_bricks == int(flags.sum())             # the restatement, bit for bit
    b = shift // 8
    region = (table.reshape(64, 64, 64) >= 0)[b[2]:b[2] + 6, b[1]:b[1] + 9, b[0]:b[0] + 11]
    differ = int((region != (small.table.cpu().numpy().reshape(6, 9, 11) >= 0)).sum())
    print("pixels kept %.3f; bricks: small grid %d, 512^3 grid %d, %d differ inside the small grid's region; %d bytes"
          % (kept, small.n_bricks, vol.n_bricks, differ, vol.memory_bytes))
    assert kept > 0.5 and small.n_bricks > 200 and 0.25 * 594 <= 594 - small.n_bricks
    assert abs(vol.n_bricks - small.n_bricks) <= 4 and differ <= 4 and vol.grown == 0
    assert vol.memory_bytes < 64 * 2 ** 20
    P = np.stack([FR.look_at((0.55, -0.45, 0.6), (-0.3, 0.2, 0.0)), FR.look_at((0.3, -0.5, 0.5), (-0.3, 0.3, 0.1))])
    assert ((P[:, :3, 3] > np.float32(S["origin"])) & (P[:, :3, 3] < hi)).all()                   # both eyes inside the small grid
    a, c = vol.raycast(frames[0]["K"], P, SIZE)["depth"] != 0, small.raycast(frames[0]["K"], P, SIZE)["depth"] != 0
    print("pixels whose hit differs:", int((a != c).sum()), "of", a.numel(), "hit", float(a.float().mean()))
    assert torch.equal(a, c) and a.float().mean() > 0.3
    K6, P6 = [f["K"] for f in frames], [f["cam2world"] for f in frames]                            # for the record: rays from outside
    a6, c6 = vol.raycast(K6, P6, SIZE)["depth"] != 0, small.raycast(K6, P6, SIZE)["depth"] != 0
    print("the six scene views (eyes outside the small grid): hit differs on", int((a6 != c6).sum()), "of", a6.numel(), "pixels")


# ------------------------------------------------------------------------------------------------ the session
EXTENT = ((-0.8, -0.7, -0.1), (0.85, 0.65, 0.8))


def test_session_without_tracking_equals_six_integrate_calls(frames):
    from spann3r_amd import fusion as F
    ses = F.FusionSession(S["voxel"], EXTENT, track=False)
    vol = F.brick_volume_for_extent(EXTENT, S["voxel"])
    for f in frames:
        pose, info = ses.push(_t(f["pts"]), f["K"], f["cam2world"], _t(f["valid"]), _t(f["images"]))
        assert np.array_equal(pose, f["cam2world"]) and info == dict(tracked=False)
        vol.integrate(**_args([f]))
    assert ses.frames == 6 and ses.volume.launches == 6 and ses.volume.n_bricks > 300 and _same_pool(ses.volume, vol)
    out = ses.raycast(frames[2]["K"], frames[2]["cam2world"][None], SIZE)
    assert float((out["depth"] != 0).float().mean()) > 0.5
    assert ses.mesh()["faces"].shape[0] > 5000


def test_session_with_tracking_equals_fuse_pointmaps_on_bricks(frames):
    from spann3r_amd import fusion as F
    moved = RC.perturbed_frames(frames, RC.perturbations(3))
    ses = F.FusionSession(S["voxel"], EXTENT, track=True)
    for f in moved:
        ses.push(_t(f["pts"]), f["K"], f["cam2world"], _t(f["valid"]), _t(f["images"]))
    pts = torch.stack([_t(f["pts"]) for f in moved])
    mesh, vol = F.fuse_pointmaps(pts, np.stack([f["K"] for f in moved]), np.stack([f["cam2world"] for f in moved]),
                                 torch.stack([_t(f["valid"]) for f in moved]).bool(), torch.stack([_t(f["images"]) for f in moved]),
                                 voxel_size=S["voxel"], track=True, bricks=True, extent=EXTENT, return_volume=True, return_poses=True)
    print("tracked", ses.tracked)
    assert ses.tracked == mesh["tracked"] and sum(ses.tracked) >= 5
    assert np.array_equal(np.stack(ses.poses), mesh["poses"]) and np.array_equal(np.stack(ses.corrections), mesh["corrections"])
    assert _same_pool(ses.volume, vol)
    got = ses.mesh()
    assert torch.equal(got["faces"], mesh["faces"]) and torch.equal(got["vertices"], mesh["vertices"])
    # and with the default extent (the valid points' box) the bricks=True path still fuses
    auto = F.fuse_pointmaps(pts[:2], moved[0]["K"], np.stack([f["cam2world"] for f in moved[:2]]),
                            torch.stack([_t(f["valid"]) for f in moved[:2]]).bool(), voxel_size=S["voxel"], bricks=True)
    assert auto["faces"].shape[0] > 1000
    with pytest.raises(ValueError, match="voxel_size"):
        F.fuse_pointmaps(pts[:2], moved[0]["K"], np.stack([f["cam2world"] for f in moved[:2]]), torch.stack([_t(f["valid"]) for f in moved[:2]]).bool(),
                         bricks=True)


# ------------------------------------------------------------------------------------------------ errors and no-ops
def test_errors_and_no_ops(frames, fused):
    from spann3r_amd import fusion as F
    from spann3r_amd import lib as L
    lib = L.load()
    o = (C.c_float * 3)(0, 0, 0)
    vol, _ = fused
    # no-ops: T = 0 and n_bricks = 0 need no pointer
    assert lib.sp3_tsdf_brick_mark(None, None, None, 0, 8, 8, 8, o, 0.1, 0.3, None, None) == 0
    assert lib.sp3_tsdf_brick_integrate(None, None, 0, 8, 8, 8, o, 0.1, 0.3, None, 1, None, None, None, None) == 0
    assert lib.sp3_tsdf_brick_raycast(None, None, 0, 8, 8, 8, o, 0.1, None, None, None, None, 1.0, 0.1, None) == 0
    tbl = vol.frame_table([_t(frames[0]["pts"])], False, frames[0]["K"], frames[0]["cam2world"][None], None, None, [_t(frames[0]["images"])])
    assert lib.sp3_tsdf_brick_integrate(tbl[0], tbl[1].data_ptr(), 1, 8, 8, 8, o, 0.1, 0.3, None, 0, None, None, None, None) == 0
    # a dimension that is not a multiple of 8
    assert lib.sp3_tsdf_brick_mark(None, None, None, 0, 8, 12, 8, o, 0.1, 0.3, None, None) != 0
    assert b"multiples of 8" in lib.sp3_last_error()
    assert lib.sp3_tsdf_brick_raycast(None, None, 0, 8, 8, 7, o, 0.1, None, None, None, None, 1.0, 0.1, None) != 0
    # band outside (0, 8 voxel]
    for band in (0.0, 0.81, math.nan):
        assert lib.sp3_tsdf_brick_mark(None, None, None, 0, 8, 8, 8, o, 0.1, band, None, None) != 0
        assert b"band" in lib.sp3_last_error()
    # the index limit
    assert lib.sp3_tsdf_brick_alloc(None, 2 ** 14, 2 ** 14, 2 ** 14, None, None, None, 16, None, None, None, None, None, None) != 0
    assert b"index limit" in lib.sp3_last_error()
    assert lib.sp3_tsdf_brick_alloc(None, 8, 8, 8, None, None, None, 2 ** 31 - 1, None, None, None, None, None, None) != 0
    assert b"index limit" in lib.sp3_last_error()
    # a frame with both, or neither, of depth and pts
    nx, ny, nz = vol.dims
    for both in (True, False):
        bad = (L.TsdfFrame * 1)()
        C.memmove(bad, tbl[0], C.sizeof(L.TsdfFrame))
        bad[0].depth = bad[0].pts if both else None
        bad[0].pts = bad[0].pts if both else None
        assert lib.sp3_tsdf_brick_mark(bad, tbl[1].data_ptr(), tbl[4].data_ptr(), 1, nx, ny, nz, vol._origin_c, vol.voxel_size, vol.band,
                                       vol.flags.data_ptr(), None) != 0
        assert b"exactly one" in lib.sp3_last_error()
    # rgba views on a pool without colours
    plain = _brick(color=False)
    with pytest.raises(ValueError, match="without colours"):
        plain.raycast(frames[0]["K"], frames[0]["cam2world"][None], SIZE, colors=True)
    vt = vol.view_table(frames[0]["K"], frames[0]["cam2world"][None], SIZE)
    assert lib.sp3_tsdf_brick_raycast(vt[0], vt[1].data_ptr(), 1, nx, ny, nz, vol._origin_c, vol.voxel_size, vol.table.data_ptr(),
                                      vol.tsdf.data_ptr(), vol.weight.data_ptr(), None, 1.0, 0.02, None) != 0
    assert b"no colours" in lib.sp3_last_error()
    with pytest.raises(ValueError, match="has colours"):
        _brick().integrate(pts=[_t(frames[0]["pts"])], intrinsics=frames[0]["K"], cam2world=frames[0]["cam2world"][None])
    with pytest.raises(RuntimeError, match="no CPU path"):
        _brick().integrate(pts=[torch.zeros(4, 4, 3)], intrinsics=frames[0]["K"], cam2world=frames[0]["cam2world"][None])
    # an empty volume: nothing allocated, every ray misses, nothing to extract
    assert plain.n_bricks == 0 and plain.brick_box() == ((0, 0, 0), (0, 0, 0)) and plain.to_dense().dims == (0, 0, 0)
    assert not plain.raycast(frames[0]["K"], frames[0]["cam2world"][None], SIZE)["depth"].any()
    vol2 = _brick().integrate(**_args(frames[:1]))
    assert vol2.n_bricks > 0
    vol2.reset()
    assert vol2.n_bricks == 0 and (vol2.table == -1).all() and int(vol2.count.cpu()) == 0
