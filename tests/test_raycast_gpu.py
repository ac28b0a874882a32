"""The ray-caster and the frame-to-model tracking of spann3r_amd.fusion on the device against the numpy restatement of the header's
rules (tests/raycast_ref.py).

Every fp32 operation of the ray-caster is specified (order, one rounding per operation, IEEE division and square root), so depth,
vertex, normal and rgba are compared bit for bit with the restatement evaluated in fp32; no tolerance is used for them.  For the
record, what the number format alone costs on the scene used here (fp32 against float64 of the restatement, measured on the CPU by
tests/test_raycast_cpu.py::test_float32_against_float64): depth 1.7e-6, vertex 1.8e-6, normal 1.5e-5; 4 x those would be the
fallback bound had a map not been bit-equal, with the hit mask equal in every case.  The ray-caster is fed the device's own
volume, downloaded, so the integration (pinned by tests/test_fusion_gpu.py) and the ray-caster are tested apart.

The accumulation is a reordered fp64 sum: every entry is held to n_pairs * 2^-52 * (the sum of the absolute values of its terms),
the pair count to equality, at the iterates of the restatement's own run."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import fusion_ref as FR
import mesh_ref as MR
import raycast_ref as RC
import render_ref as RR

pytestmark = pytest.mark.gpu

S = RC.SCENE
MAPS = (("depth", "depth"), ("vertices", "vertex"), ("normals", "normal"))


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _volume(color=True, dims=None):
    from spann3r_amd import fusion as F
    return F.TSDFVolume(S["origin"], S["voxel"], S["dims"] if dims is None else dims, trunc=S["trunc"], color=color)


def _state(vol):
    return vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), None if vol.rgb is None else vol.rgb.cpu().numpy()


def _ref(state, fr, step_voxels=1.0, min_weight=1.0, **kw):
    step = np.float32(np.float32(step_voxels) * np.float32(S["voxel"]))
    return RC.raycast_ref(*state, np.float32(S["origin"]), np.float32(S["voxel"]), RC.scene_view(fr, **kw), min_weight, step, np.float32)


def _assert_equal(got, ref, i=None, colors=True):
    """the maps of view i of a raycast() dict against one restatement dict, bit for bit"""
    pick = (lambda x: x) if i is None else (lambda x: x[i])
    depth = pick(got["depth"]).cpu().numpy()
    assert np.array_equal(depth != 0, ref["hit"])
    for name, rname in MAPS:
        g = pick(got[name]).cpu().numpy()
        assert _bits(g, ref[rname]), (name, float(np.abs(g - ref[rname]).max()))
    if colors:
        assert np.array_equal(pick(got["colors"]).cpu().numpy().view(np.uint32)[..., 0], ref["rgba"])


@pytest.fixture(scope="module")
def frames():
    return RC.scene_frames()


@pytest.fixture(scope="module")
def fused(frames):
    """SCENE fused on the device through `pts` with colours; (volume, its downloaded state)"""
    vol = _volume()
    vol.integrate(pts=[_t(f["pts"]) for f in frames], intrinsics=[f["K"] for f in frames], cam2world=[f["cam2world"] for f in frames],
                  valid=[_t(f["valid"]) for f in frames], images=[_t(f["images"]) for f in frames])
    return vol, _state(vol)


@pytest.fixture(scope="module")
def refs(frames, fused):
    """the six scene views by the restatement in fp32, computed once"""
    return [_ref(fused[1], fr) for fr in frames]


def _cast(vol, frs, **kw):
    return vol.raycast([f["K"] for f in frs], [f["cam2world"] for f in frs], (S["h"], S["w"]), **kw)


# ------------------------------------------------------------------------------------------------ ray-casting
def test_raycast_equals_the_restatement_bit_for_bit(frames, fused, refs):
    vol, _ = fused
    before = vol.raycasts
    one = _cast(vol, frames)                                                                     # six views, one launch
    assert vol.raycasts == before + 1
    assert one["depth"].shape == (6, S["h"], S["w"]) and one["colors"].shape == (6, S["h"], S["w"], 4) and one["colors"].dtype == torch.uint8
    for i, ref in enumerate(refs):
        hit = ref["hit"].mean()
        print("view", i, "hit", float(hit))
        assert 0.4 <= hit <= 0.76                                                                # both outcomes in every view
        _assert_equal(one, ref, i)
        single = _cast(vol, frames[i:i + 1])                                                     # and as six launches
        for k in one:
            assert torch.equal(single[k][0], one[k][i])
    assert vol.raycasts == before + 7
    n = one["normals"].cpu().numpy().astype(np.float64)
    m = one["depth"].cpu().numpy() != 0
    assert np.abs(np.linalg.norm(n[m], axis=-1) - 1).max() < 1e-6 and (n[~m] == 0).all()


def test_raycast_maps_are_optional_and_T0_is_a_no_op(frames, fused, refs):
    vol, _ = fused
    got = _cast(vol, frames[2:3], vertices=False, normals=False, colors=False)
    assert sorted(got) == ["depth"] and _bits(got["depth"][0].cpu().numpy(), refs[2]["depth"])
    before = vol.raycasts
    none = vol.raycast(frames[0]["K"], np.zeros((0, 4, 4)), (S["h"], S["w"]))
    assert none["depth"].shape == (0, S["h"], S["w"]) and none["normals"].shape == (0, S["h"], S["w"], 3) and vol.raycasts == before
    from spann3r_amd import lib as L
    o = (C.c_float * 3)(0, 0, 0)
    assert L.load().sp3_tsdf_raycast(None, None, 0, 8, 8, 8, o, 0.1, None, None, None, 1.0, 0.1, None) == 0          # T = 0
    assert L.load().sp3_tsdf_raycast(None, None, 0, 8, 8, 8, o, 0.1, None, None, None, 1.0, 1e-9, None) != 0         # cap over 2^24
    assert b"2^24" in L.load().sp3_last_error()


def _raw_view(e, maps, w, h, stride, fr, near=0.0, far=math.inf):
    e.depth, e.vertex, e.normal, e.rgba = (None if m is None else m.data_ptr() for m in maps)
    e.row_stride, e.w, e.h = stride, w, h
    e.fu, e.fv, e.cu, e.cv = fr["fu"], fr["fv"], fr["cu"], fr["cv"]
    e.c2w[:] = np.asarray(fr["cam2world"])[:3].reshape(12).astype(np.float32).tolist()
    e.near, e.far = near, far


def _raw_raycast(vol, table, min_weight=1.0, step=None):
    from spann3r_amd import lib as L
    table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    nx, ny, nz = vol.dims
    step = float(np.float32(vol.voxel_size)) if step is None else step
    rc = L.load().sp3_tsdf_raycast(table, table_d.data_ptr(), len(table), nx, ny, nz, vol._origin_c, vol.voxel_size, vol.tsdf.data_ptr(),
                                   vol.weight.data_ptr(), L.ptr(vol.rgb), min_weight, step, L.stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_raycast_odd_view_with_a_row_stride_leaves_the_padding_alone(frames, fused):
    from spann3r_amd import lib as L
    vol, state = fused
    h, w, stride = 19, 37, 40
    fr = dict(frames[3], fu=23.0, fv=22.5, cu=18.25, cv=9.0)
    depth = torch.full((h, stride), -7.0, device="cuda")
    vertex, normal = torch.full((h, stride, 3), -7.0, device="cuda"), torch.full((h, stride, 3), -7.0, device="cuda")
    rgba = torch.full((h, stride), 12345, dtype=torch.int32, device="cuda")
    table = (L.TsdfView * 1)()
    _raw_view(table[0], (depth, vertex, normal, rgba), w, h, stride, fr)
    assert _raw_raycast(vol, table) == 0
    ref = RC.raycast_ref(*state, np.float32(S["origin"]), np.float32(S["voxel"]), dict(RC.scene_view(fr), w=w, h=h), 1.0, None, np.float32)
    assert 0.2 < ref["hit"].mean() < 0.9
    assert _bits(depth[:, :w].cpu().numpy(), ref["depth"]) and _bits(vertex[:, :w].cpu().numpy(), ref["vertex"])
    assert _bits(normal[:, :w].cpu().numpy(), ref["normal"]) and np.array_equal(rgba[:, :w].cpu().numpy().view(np.uint32), ref["rgba"])
    assert (depth[:, w:] == -7.0).all() and (vertex[:, w:] == -7.0).all() and (normal[:, w:] == -7.0).all() and (rgba[:, w:] == 12345).all()


def test_raycast_views_of_different_sizes_in_one_launch(frames, fused, refs):
    """the grid is sized by the largest view; a smaller view's blocks beyond its own size write nothing"""
    from spann3r_amd import lib as L
    vol, state = fused
    small = dict(frames[1], fu=20.0, fv=20.0, cu=9.5, cv=7.0)
    d0, d1 = torch.full((S["h"], S["w"]), -7.0, device="cuda"), torch.full((33, 32), -7.0, device="cuda")
    table = (L.TsdfView * 2)()
    _raw_view(table[0], (d0, None, None, None), S["w"], S["h"], S["w"], frames[0])
    _raw_view(table[1], (d1, None, None, None), 21, 17, 32, small)
    assert _raw_raycast(vol, table) == 0
    ref = RC.raycast_ref(*state, np.float32(S["origin"]), np.float32(S["voxel"]), dict(RC.scene_view(small), w=21, h=17), 1.0, None, np.float32)
    assert _bits(d0.cpu().numpy(), refs[0]["depth"]) and _bits(d1[:17, :21].cpu().numpy(), ref["depth"]) and ref["hit"].any()
    assert (d1[17:] == -7.0).all() and (d1[:, 21:] == -7.0).all()


def test_raycast_eye_inside_looking_away_near_and_far(frames, fused, refs):
    vol, state = fused
    h, w = S["h"], S["w"]
    K = frames[0]["K"]
    inside = dict(frames[0], cam2world=FR.look_at((0.5, -0.55, 0.5), (0.0, 0.0, 0.4)))           # an eye inside the volume
    got = vol.raycast(K, inside["cam2world"], (h, w))
    ref = _ref(state, inside)
    assert 0.3 < ref["hit"].mean() < 1.0
    _assert_equal(got, ref, 0)
    away = dict(frames[0], cam2world=FR.look_at((0.95, -1.25, 0.85), (2.0, -3.0, 1.5)))          # looking away: nothing
    got = vol.raycast(K, away["cam2world"], (h, w))
    assert all(float(v.abs().max()) == 0.0 for v in got.values())
    assert not _ref(state, away)["hit"].any()
    # far cuts the big sphere, near lies beyond it
    d0 = refs[0]["depth"]
    ball = np.linalg.norm(refs[0]["vertex"].astype(np.float64) - np.asarray(S["spheres"][0][0]), axis=-1) < 0.5
    ball &= refs[0]["hit"]
    far = float(np.float32(np.median(d0[ball])))
    got = vol.raycast(K, frames[0]["cam2world"], (h, w), far=far)
    ref = _ref(state, frames[0], far=far)
    _assert_equal(got, ref, 0)
    assert ref["hit"].any() and ref["depth"].max() <= far + S["voxel"] and (refs[0]["hit"] & ~ref["hit"] & ball).any()
    near = float(np.float32(d0[ball].max() + 2 * S["voxel"]))
    got = vol.raycast(K, frames[0]["cam2world"], (h, w), near=near)
    ref = _ref(state, frames[0], near=near)
    _assert_equal(got, ref, 0)
    assert (ref["depth"][ref["hit"]] >= near - S["voxel"]).all() and not (ref["hit"] & ball).all()


@pytest.mark.parametrize("step_voxels", [0.5, 2.0])
def test_raycast_step(frames, fused, refs, step_voxels):
    vol, state = fused
    got = _cast(vol, frames[4:5], step_voxels=step_voxels)
    ref = _ref(state, frames[4], step_voxels=step_voxels)
    _assert_equal(got, ref, 0)
    both = ref["hit"] & refs[4]["hit"]
    assert both.mean() > 0.6 and np.median(np.abs(ref["depth"] - refs[4]["depth"])[both]) < S["voxel"] / 4


def test_raycast_min_weight(frames, fused, refs):
    vol, state = fused
    got = _cast(vol, frames[1:2], min_weight=2.0)
    ref = _ref(state, frames[1], min_weight=2.0)
    _assert_equal(got, ref, 0)
    assert 0 < ref["hit"].sum() < refs[1]["hit"].sum()


def test_raycast_without_colours_and_a_flat_volume(frames, fused):
    from spann3r_amd import lib as L
    vol, state = fused
    plain = _volume(color=False)
    plain.tsdf.copy_(vol.tsdf)
    plain.weight.copy_(vol.weight)
    got = _cast(plain, frames[5:6])
    assert "colors" not in got
    _assert_equal(got, _ref((state[0], state[1], None), frames[5]), 0, colors=False)
    with pytest.raises(ValueError, match="without colours"):
        _cast(plain, frames[5:6], colors=True)
    depth = torch.full((S["h"], S["w"]), -7.0, device="cuda")
    rgba = torch.zeros((S["h"], S["w"]), dtype=torch.int32, device="cuda")
    table = (L.TsdfView * 1)()
    _raw_view(table[0], (depth, None, None, rgba), S["w"], S["h"], S["w"], frames[5])
    assert _raw_raycast(plain, table) != 0 and b"no colours" in L.load().sp3_last_error()         # the error code of the raw entry
    assert (depth == -7.0).all()
    flat = _volume(color=False, dims=(1, S["dims"][1], S["dims"][2]))                             # nx = 1: no cell, every ray misses
    flat.tsdf.fill_(-0.5)
    flat.weight.fill_(1.0)
    flat.tsdf[:, : S["dims"][1] // 2] = 0.5
    got = _cast(flat, frames[:2])
    assert all(float(v.abs().max()) == 0.0 for v in got.values())


def test_raycast_depth_against_the_rasterised_mesh(frames, fused, refs):
    """Two independent routes to the same level set: the ray-cast depth and the z-buffer of the marching-tetrahedra mesh of the same
    volume (extract_mesh + add_triangles), at the pixels both hit.  The difference is discretisation (a trilinear level set against
    flat triangles on the Kuhn cut, pixel-centre rays against the 1/16-pixel snapping of the rasteriser), not arithmetic; it is held
    to 2 x the same difference between the two CPU restatements.  Measured on this view between the restatements: median 8.7e-4, 90 % below
    3.8e-3 (0.09 voxel), maximum 0.63 at a silhouette, where the two routes see different surfaces."""
    from spann3r_amd import vis
    vol, state = fused
    fr, w, h = frames[2], S["w"], S["h"]
    K, E = fr["K"], np.linalg.inv(fr["cam2world"])
    mesh = vol.extract_mesh()
    r = vis.PointRenderer(camera=vis.Camera(K, E, w, h))
    r.add_triangles(mesh["vertices"], mesh["faces"], mesh["colors"])
    _, zbuf = (x.cpu().numpy() for x in r.image(return_depth=True))
    cast = _cast(vol, [fr])["depth"][0].cpu().numpy()
    rv, _, rf = FR.extract_ref(*state, np.float32(S["origin"]), np.float32(S["voxel"]), 1.0, np.float32)
    cam = r.camera
    ref_cam = RR.Cam(cam.extrinsic[:3, :3], cam.extrinsic[:3, 3], K[0, 0], K[1, 1], K[0, 2], K[1, 2], w, h)
    _, rz, _ = MR.raster(rv, rf, None, ref_cam, 4096, dtype=np.float32)

    def diff(a, z):
        both = (a != 0) & np.isfinite(z)
        assert both.sum() > 1500
        d = np.abs(a.astype(np.float64) - z.astype(np.float64))[both]
        return float(np.median(d)), float(np.quantile(d, 0.9)), float(d.max())

    got, ref = diff(cast, zbuf), diff(refs[2]["depth"], rz)
    print("ray-cast against rasterised depth (median, p90, max): device", got, "restatements", ref)
    assert all(g <= 2 * r_ for g, r_ in zip(got, ref))
    assert ref[0] < S["voxel"] / 4


# ------------------------------------------------------------------------------------------------ tracking
@pytest.fixture(scope="module")
def moved(frames):
    return RC.perturbed_frames(frames, RC.perturbations(1))


def _accum(pts, valid, T, model, w2c, dist_max, maps=None):
    from spann3r_amd import lib as L
    from spann3r_amd.fusion import _rt12
    lib = L.load()
    p = _t(np.ascontiguousarray(pts, np.float32).reshape(-1, 3))
    n = p.shape[0]
    v = None if valid is None else _t(np.ascontiguousarray(valid, np.uint8).reshape(-1))
    maps = maps or tuple(_t(np.ascontiguousarray(model[k], np.float32)) for k in ("vertex", "normal", "depth"))
    h, w = model["depth"].shape
    ws = torch.empty(max(int(lib.sp3_tsdf_track_accum_ws_bytes(n)), 16), dtype=torch.uint8, device="cuda")
    out = torch.full((29,), -1.0, dtype=torch.float64, device="cuda")
    T_d, w2c_d = _t(_rt12(T)), _t(_rt12(w2c))                                                   # (held until the result is read)
    L.check(lib.sp3_tsdf_track_accum(p.data_ptr(), L.ptr(v), n, T_d.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(),
                                     w, h, w, model["fu"], model["fv"], model["cu"], model["cv"], w2c_d.data_ptr(), dist_max, ws.data_ptr(),
                                     out.data_ptr(), L.stream_ptr()), "sp3_tsdf_track_accum")
    return out.cpu().numpy()


def _assert_accum(got, ref, ab):
    assert got[28] == ref[28]
    bound = ref[28] * 2.0 ** -52 * ab
    assert (np.abs(got - ref) <= bound).all(), (np.abs(got - ref) / np.maximum(bound, 1e-300)).max()


def test_track_accum_at_every_iterate_of_the_restatement(frames, moved):
    """T comes from the restatement's run (fp32 ray-casts, as on the device), so no difference is amplified by the iteration"""
    origin, voxel, trunc = np.float32(S["origin"]), np.float32(S["voxel"]), np.float32(S["trunc"])
    state = RC.fuse_ref(frames[:1], color=False)
    fr = moved[1]
    trace = []
    T, info = RC.track_frame_ref(state, origin, voxel, trunc, fr["pts"], fr["valid"], fr["K"], fr["cam2world"], dtype=np.float32, trace=trace)
    assert info["tracked"] and len(trace) == info["iterations"] >= 4 and len({id(t["model"]) for t in trace}) == 2
    maps = {}
    for it in trace:
        m = it["model"]
        if id(m) not in maps:
            maps[id(m)] = tuple(_t(np.ascontiguousarray(m[k], np.float32)) for k in ("vertex", "normal", "depth"))
        got = _accum(fr["pts"], fr["valid"], it["T"], m, it["w2c"], float(trunc), maps[id(m)])
        assert it["out29"][28] > 1000
        _assert_accum(got, it["out29"], it["abs29"])
    # valid null; a NaN point, a point behind the camera and one projecting outside the map are skipped
    it = trace[-1]
    m = it["model"]
    pts = fr["pts"].copy()
    pts[10, 10] = np.nan
    pts[11, 11, 1] = np.inf
    eye, fwd = fr["cam2world"][:3, 3], fr["cam2world"][:3, 2]
    pts[12, 12] = eye - 0.5 * fwd                                                                # behind the camera
    pts[13, 13] = eye + 0.5 * fwd + 5.0 * fr["cam2world"][:3, 0]                                 # far off to the right: outside the map
    ref, ab = RC.track_accum_ref(pts, None, it["T"], m, it["w2c"], float(trunc), return_abs=True)
    full, _ = RC.track_accum_ref(fr["pts"], None, it["T"], m, it["w2c"], float(trunc), return_abs=True)
    assert full[28] - 4 <= ref[28] < full[28]
    _assert_accum(_accum(pts, None, it["T"], m, it["w2c"], float(trunc), maps[id(m)]), ref, ab)
    none = _accum(pts, np.zeros(pts.shape[:2], np.uint8), it["T"], m, it["w2c"], float(trunc), maps[id(m)])
    assert (none == 0).all()


def test_track_frame_and_tracked_fusion_recover_the_motion(frames, moved):
    """fuse_pointmaps(track=True) on the frames moved by 2 degrees and a voxel each (seed 1): every frame is tracked and its leftover
    rotation and translation are at most half of what it started with; without track the poses stay as given and one launch runs"""
    from spann3r_amd import fusion as F
    motions = RC.perturbations(1)
    pts = _t(np.stack([f["pts"] for f in moved]))
    valid = _t(np.stack([f["valid"] for f in moved]))
    K = np.stack([f["K"] for f in moved])
    poses = np.stack([f["cam2world"] for f in moved])
    mesh, vol = F.fuse_pointmaps(pts, K, poses, valid, voxel_size=S["voxel"], return_volume=True, track=True, return_poses=True)
    assert vol.launches == len(moved) and vol.raycasts == 2 * (len(moved) - 1) and all(mesh["tracked"]) and mesh["faces"].shape[0] > 0
    assert np.array_equal(mesh["corrections"][0], np.eye(4))
    for i in range(1, len(moved)):
        (r0, t0), (r1, t1) = RC.motion_size(motions[i]), RC.motion_size(mesh["corrections"][i] @ motions[i])
        print("frame", i, "start %.2f deg %.4f" % (r0, t0), "end %.3f deg %.4f" % (r1, t1))
        assert r1 <= 0.5 * r0 and t1 <= 0.5 * t0
        assert np.allclose(mesh["poses"][i], mesh["corrections"][i] @ poses[i], rtol=0, atol=1e-12)
    plain, vol0 = F.fuse_pointmaps(pts, K, poses, valid, voxel_size=S["voxel"], return_volume=True, return_poses=True)
    assert vol0.launches == 1 and vol0.raycasts == 0 and not any(plain["tracked"]) and np.array_equal(plain["poses"], poses)
    assert np.array_equal(plain["corrections"], np.stack([np.eye(4)] * len(moved)))
    again = F.fuse_pointmaps(pts, K, poses, valid, voxel_size=S["voxel"])
    assert "poses" not in again and torch.equal(again["vertices"], plain["vertices"]) and torch.equal(again["faces"], plain["faces"])


def test_track_frame_that_cannot_be_registered(frames, fused):
    from spann3r_amd import fusion as F
    vol, _ = fused
    fr = frames[1]
    T, info = F.track_frame(vol, _t(fr["pts"]), _t(np.zeros_like(fr["valid"])), fr["K"], fr["cam2world"])
    assert np.array_equal(T, np.eye(4)) and info["tracked"] is False and info["pairs"] == 0
    T, info = F.track_frame(_volume(color=False), _t(fr["pts"]), None, fr["K"], fr["cam2world"])  # a model with no hit
    assert np.array_equal(T, np.eye(4)) and info["tracked"] is False and info["pairs"] == 0
    T, info = F.track_frame(vol, _t(fr["pts"]), _t(fr["valid"]), fr["K"], fr["cam2world"])       # the unmoved frame stays where it is
    r, t = RC.motion_size(T)
    assert info["tracked"] and info["pairs"] > 1000 and r < 0.5 and t < 0.01


def test_argument_errors_never_launch(frames, fused):
    from spann3r_amd import fusion as F
    vol, _ = fused
    fr = frames[0]
    before = (vol.raycasts, vol.launches)
    size = (S["h"], S["w"])
    skew = fr["K"].copy()
    skew[0, 1] = 0.5
    nan_pose = fr["cam2world"].copy()
    nan_pose[1, 3] = np.nan
    with pytest.raises(ValueError, match="skew"):
        vol.raycast(skew, fr["cam2world"], size)
    with pytest.raises(ValueError, match="finite"):
        vol.raycast(fr["K"], nan_pose, size)
    with pytest.raises(ValueError, match="singular"):
        vol.raycast(fr["K"], np.zeros((4, 4)), size)
    with pytest.raises(ValueError, match="step_voxels"):
        vol.raycast(fr["K"], fr["cam2world"], size, step_voxels=0.2)
    with pytest.raises(ValueError, match="near"):
        vol.raycast(fr["K"], fr["cam2world"], size, near=2.0, far=1.0)
    with pytest.raises(ValueError, match="min_weight"):
        vol.raycast(fr["K"], fr["cam2world"], size, min_weight=0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.track_frame(vol, torch.from_numpy(fr["pts"]), None, fr["K"], fr["cam2world"])
    with pytest.raises(ValueError, match="skew"):
        F.track_frame(vol, _t(fr["pts"]), None, skew, fr["cam2world"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.fuse_pointmaps(torch.from_numpy(fr["pts"][None]), fr["K"], fr["cam2world"][None], torch.ones(1, *size, dtype=torch.bool), track=True)
    assert (vol.raycasts, vol.launches) == before
    from spann3r_amd import lib as L
    lib = L.load()
    table = (L.TsdfView * 1)()
    depth = torch.full(size, -7.0, device="cuda")
    _raw_view(table[0], (depth, None, None, None), S["w"], S["h"], S["w"], fr, near=2.0, far=1.0)
    assert _raw_raycast(vol, table) != 0 and b"near" in lib.sp3_last_error()
    _raw_view(table[0], (depth, None, None, None), S["w"], S["h"], S["w"] - 1, fr)
    assert _raw_raycast(vol, table) != 0 and b"geometry" in lib.sp3_last_error()
    _raw_view(table[0], (depth, None, None, None), S["w"], S["h"], S["w"], fr)
    assert _raw_raycast(vol, table, min_weight=0.0) != 0 and _raw_raycast(vol, table, step=0.0) != 0
    assert (depth == -7.0).all()
    assert lib.sp3_tsdf_track_accum(None, None, 4, None, None, None, None, 8, 8, 8, 1.0, 1.0, 0.0, 0.0, None, 0.1, None, None, None) != 0
    assert b"null" in lib.sp3_last_error()
