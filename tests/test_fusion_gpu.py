"""spann3r_amd.fusion on the device against the numpy restatement of the header's rules (tests/fusion_ref.py) evaluated in fp32.

Every operation of both stages is specified (order, one rounding per operation, IEEE division), so the comparisons are bit for bit:
weight, tsdf and rgb of the integration; V, F, faces, vertices and colours of the extraction.  No tolerance is used for them.  For
the record, what the number format alone costs on the scene used here (fp32 against float64 of the restatement, measured on the
CPU by tests/test_fusion_cpu.py::test_fused_scene_float32_against_float64): tsdf 7.9e-7 absolute through `depth`, 9.2e-7 through
`pts`; a bound of 4 x that (3.7e-6) would be the fallback had a stage not been bit-equal.  The two stages are tested apart: the
extraction is fed the device's own volume, downloaded, so that no sign at a near-zero voxel can differ between the two sides.
The rasteriser check reuses tests/mesh_ref.py and the DEPTH_RTOL of tests/test_mesh_gpu.py.

The kernel reads its frame table straight from memory, frame by frame (no chunks), so there is no chunk + 1 case."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
import fusion_ref as FR
import mesh_ref as MR
import render_ref as RR
from test_mesh_cpu import read_glb
from test_mesh_gpu import DEPTH_RTOL

pytestmark = pytest.mark.gpu

S = FR.SCENE


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _volume(color=True, dims=None, origin=None, voxel=None, trunc=None):
    from spann3r_amd import fusion as F
    return F.TSDFVolume(S["origin"] if origin is None else origin, S["voxel"] if voxel is None else voxel, S["dims"] if dims is None else dims,
                        trunc=S["trunc"] if trunc is None else trunc, color=color)


def _integrate(vol, frames, path):
    kw = dict(intrinsics=[f["K"] for f in frames], cam2world=[f["cam2world"] for f in frames], valid=[_t(f["valid"]) for f in frames],
              weight=[None if f["pixel_weight"] is None else _t(f["pixel_weight"]) for f in frames])
    if vol.rgb is not None:
        kw["images"] = [_t(f["images"]) for f in frames]
    kw[path] = [_t(f[path]) for f in frames]
    return vol.integrate(**kw)


def _state(vol):
    return vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), None if vol.rgb is None else vol.rgb.cpu().numpy()


def _ref_args(vol):
    return vol.origin, np.float32(vol.voxel_size), np.float32(vol.trunc), np.float32


@pytest.fixture(scope="module")
def frames():
    from spann3r_amd import fusion as F
    fr = FR.scene_frames()
    _, w2c = F.camera_tables([f["K"] for f in fr], [f["cam2world"] for f in fr], len(fr))      # the matrices the kernel is given
    for f, m in zip(fr, w2c):
        f["w2c"] = m
    return fr


@pytest.fixture(scope="module")
def fused(frames):
    """the 21 x 18 x 13 scene fused on the device through `depth`, downloaded"""
    vol = _integrate(_volume(), frames, "depth")
    return vol, _state(vol)


# ------------------------------------------------------------------------------------------------ integrate
@pytest.mark.parametrize("path", ["depth", "pts"])
def test_integrate_equals_the_restatement_bit_for_bit(frames, path):
    vol = _volume()
    assert vol.integrate(**{path: [], "intrinsics": [], "cam2world": []}) is vol and vol.launches == 0                 # T = 0
    assert float(vol.tsdf.min()) == 1.0 and float(vol.weight.max()) == 0.0
    _integrate(vol, frames[:3], path)
    assert vol.launches == 1
    ref3 = FR.integrate_ref(*FR.empty_volume(S["dims"]), FR.as_path(frames[:3], path), *_ref_args(vol))
    got3 = _state(vol)
    print(path, "3 frames: weight differs at", int((got3[1] != ref3[1]).sum()), "tsdf max abs", float(np.abs(got3[0] - ref3[0]).max()),
          "rgb max abs", float(np.abs(got3[2] - ref3[2]).max()))
    assert _bits(got3[1], ref3[1]) and _bits(got3[0], ref3[0]) and _bits(got3[2], ref3[2])
    assert (got3[1] > 0).mean() > 0.3 and (got3[1] == 0).any() and (got3[0] < 0).any() and got3[1].max() > 3.0
    _integrate(vol, frames[3:], path)                                                            # 2 more frames: a second call
    assert vol.launches == 2
    one = _integrate(_volume(), frames, path)                                                    # all 5 in one call
    assert one.launches == 1
    ref5 = FR.integrate_ref(*FR.empty_volume(S["dims"]), FR.as_path(frames, path), *_ref_args(vol))
    for a, b, r in zip(_state(vol), _state(one), ref5):
        assert _bits(a, b) and _bits(a, r)


def test_integrate_without_colours_and_raw_no_ops(frames):
    from spann3r_amd import lib as L
    vol = _integrate(_volume(color=False), frames, "depth")
    ref = FR.integrate_ref(*FR.empty_volume(S["dims"], color=False), FR.as_path(frames, "depth"), *_ref_args(vol))
    got = _state(vol)
    assert got[2] is None and _bits(got[0], ref[0]) and _bits(got[1], ref[1])
    lib = L.load()
    o = (C.c_float * 3)(0, 0, 0)
    assert lib.sp3_tsdf_integrate(None, None, 0, 8, 8, 8, o, 0.1, 0.3, None, None, None, None) == 0                    # T = 0
    assert lib.sp3_tsdf_integrate(None, None, 3, 8, 0, 8, o, 0.1, 0.3, None, None, None, None) == 0                    # empty volume
    assert lib.sp3_tsdf_extract(None, None, None, 0, 4, 4, o, 0.1, 1.0, None, 0, 0, None, None, None, None, None) == 0
    assert lib.sp3_tsdf_integrate(None, None, 1, 8, 8, 8, o, 0.1, -1.0, None, None, None, None) != 0
    assert b"trunc" in lib.sp3_last_error()
    assert lib.sp3_tsdf_integrate(None, None, 1, 1024, 1024, 512, o, 0.1, 0.3, None, None, None, None) != 0
    assert b"index limit" in lib.sp3_last_error()
    with pytest.raises(ValueError, match="colours"):
        _volume().integrate(depth=[_t(frames[0]["depth"])], intrinsics=frames[0]["K"], cam2world=[frames[0]["cam2world"]])
    with pytest.raises(RuntimeError, match="mismatched shapes"):
        _volume(color=False).integrate(depth=[_t(frames[0]["depth"])], intrinsics=frames[0]["K"], cam2world=[frames[0]["cam2world"]],
                                       valid=[_t(frames[0]["valid"][:, :-1])])
    with pytest.raises(RuntimeError, match="mismatched lengths"):
        _volume(color=False).integrate(depth=[_t(frames[0]["depth"])], intrinsics=frames[0]["K"], cam2world=[frames[0]["cam2world"]],
                                       valid=[_t(f["valid"]) for f in frames[:2]])
    with pytest.raises(RuntimeError, match="no CPU path"):
        _volume(color=False).integrate(depth=[torch.zeros(4, 4)], intrinsics=frames[0]["K"], cam2world=[frames[0]["cam2world"]])


# ------------------------------------------------------------------------------------------------ extract
def _extract(vol, min_weight=1.0):
    v, c, f, counts = vol.extract_raw(min_weight, 7 * vol.tsdf.numel(), 12 * vol.tsdf.numel())
    nv, nf = counts.cpu().tolist()
    return v[:nv].cpu().numpy(), c[:nv].cpu().numpy().view(np.uint32), f[:nf].cpu().numpy(), nv, nf


def _assert_extract_equals_ref(vol, min_weight=1.0):
    tsdf, weight, rgb = _state(vol)
    rv, rc, rf = FR.extract_ref(tsdf, weight, rgb, vol.origin, np.float32(vol.voxel_size), min_weight, np.float32)
    gv, gc, gf, nv, nf = _extract(vol, min_weight)
    assert (nv, nf) == (len(rv), len(rf))
    assert np.array_equal(gf, rf)
    assert _bits(gv, rv), float(np.abs(gv - rv).max())
    assert np.array_equal(gc, rc)
    return gv, gc, gf


def _load(vol, tsdf, weight):
    vol.tsdf.copy_(_t(tsdf))
    vol.weight.copy_(_t(weight))
    return vol


def test_extract_fused_scene_equals_the_restatement(fused):
    vol, _ = fused
    v, c, f = _assert_extract_equals_ref(vol)
    assert len(f) > 300 and len(np.unique(c)) > 50 and FR.manifold_report(f)["bad"] == 0
    v2, c2, f2 = _assert_extract_equals_ref(vol, min_weight=2.5)                                 # fewer observed voxels, fewer live cells
    assert 0 < len(f2) < len(f)


def test_extract_sphere_is_a_closed_manifold():
    n, h, centre, radius = 24, 0.05, (0.011, -0.017, 0.006), 0.43
    origin = (-0.58, -0.57, -0.59)
    tsdf, weight = FR.sphere_volume((n, n, n), origin, h, centre, radius, 3 * h)
    vol = _load(_volume(False, (n, n, n), origin, h, 3 * h), tsdf, weight)
    v, c, f = _assert_extract_equals_ref(vol)
    rep = FR.manifold_report(f)
    assert len(f) > 1000 and rep["closed"] and rep["euler"] == 2 and len(np.unique(f)) == len(v)
    assert (c == 0xffffffff).all()
    L_ = np.sqrt(3) * h                                                                          # (the bound derived in test_fusion_cpu.py, plus fp32 positions)
    err = np.abs(np.linalg.norm(v.astype(np.float64) - np.asarray(centre), axis=1) - radius)
    assert err.max() <= L_ * L_ / (8 * (radius - L_)) + 2.0 ** -24 * 3 * h + 4 * 2.0 ** -24
    a, b, d = (v[f[:, k]].astype(np.float64) - np.asarray(centre) for k in range(3))
    assert np.einsum("ij,ij->i", a, np.cross(b, d)).sum() > 0                                    # outward


def test_extract_more_than_1024_scan_tiles():
    dims, h = (65, 64, 64), 0.02
    assert (dims[0] * dims[1] * dims[2] + 255) // 256 > 1024
    origin = (-0.64, -0.63, -0.65)
    tsdf, weight = FR.sphere_volume(dims, origin, h, (0.01, 0.0, -0.02), 0.55, 3 * h)
    weight[:, :, 40:] = 0                                                                        # a cut: vertices without faces exist too
    weight[10:20, 5:9, 3:30] = 0
    vol = _load(_volume(False, dims, origin, h, 3 * h), tsdf, weight)
    v, c, f = _assert_extract_equals_ref(vol)
    assert len(f) > 20000 and len(FR.manifold_report(f)["boundary"]) > 0


def test_extract_nothing_observed():
    vol = _volume()
    v, c, f, nv, nf = _extract(vol)
    assert nv == 0 and nf == 0
    m = vol.extract_mesh()
    assert m["vertices"].shape == (0, 3) and m["faces"].shape == (0, 3) and m["colors"].shape == (0, 4)
    vol.weight.fill_(1.0)                                                                        # observed, all positive
    assert _extract(vol)[3:] == (0, 0)


def test_extract_capacity_and_retry():
    from spann3r_amd import lib as L
    rng = np.random.default_rng(5)
    dims = (16, 15, 14)
    tsdf = rng.uniform(-1, 1, dims[::-1]).astype(np.float32)
    weight = (rng.random(dims[::-1]) < 0.95).astype(np.float32)
    vol = _load(_volume(False, dims), tsdf, weight)
    v, c, f = _assert_extract_equals_ref(vol)
    nv, nf, n = len(v), len(f), tsdf.size
    assert nv > max(4096, n // 4)                                                                # over extract_mesh's first guess
    cap_v, cap_f, room_v, room_f = nv // 2, nf // 3, nv + 64, nf + 64
    lib = L.load()
    bv = torch.full((room_v, 3), -7.0, device="cuda")
    bc = torch.full((room_v,), 12345, dtype=torch.int32, device="cuda")
    bf = torch.full((room_f, 3), -9, dtype=torch.int32, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.sp3_tsdf_extract_ws_bytes(*dims)), dtype=torch.uint8, device="cuda")
    L.check(lib.sp3_tsdf_extract(vol.tsdf.data_ptr(), vol.weight.data_ptr(), None, *dims, vol._origin_c, vol.voxel_size, 1.0, ws.data_ptr(),
                                 cap_v, cap_f, bv.data_ptr(), bc.data_ptr(), bf.data_ptr(), counts.data_ptr(), L.stream_ptr()), "sp3_tsdf_extract")
    assert counts.cpu().tolist() == [nv, nf]                                                     # the need, not the capacity
    assert _bits(bv[:cap_v].cpu().numpy(), v[:cap_v]) and np.array_equal(bf[:cap_f].cpu().numpy(), f[:cap_f])
    assert (bv[cap_v:] == -7.0).all() and (bc[cap_v:] == 12345).all() and (bf[cap_f:] == -9).all()
    m = vol.extract_mesh()                                                                       # overflows its guess, retries once
    rpos, kept, rfaces, rbounds = MR.compact_ref(v, f)
    assert np.array_equal(m["faces"].cpu().numpy(), rfaces) and _bits(m["vertices"].cpu().numpy(), rpos)
    assert np.array_equal(m["bounds"], rbounds) and (m["colors"].cpu().numpy() == 255).all()


# ------------------------------------------------------------------------------------------------ end to end
def test_fuse_views_compact_and_glb(tmp_path):
    from spann3r_amd import fusion as F, mesh as M
    g = load_golden("views_rgbd.npz")
    views = [dict(img=_t(g["landscape_img"][i:i + 1]), depthmap=_t(g["landscape_depthmap"][i:i + 1]),
                  camera_pose=_t(g["landscape_camera_pose"][i:i + 1]), camera_intrinsics=_t(g["landscape_camera_intrinsics"][i:i + 1]),
                  pts3d=_t(g["landscape_pts3d"][i:i + 1]), valid_mask=_t(g["landscape_valid_mask"][i:i + 1])) for i in range(3)]
    mesh, vol = F.fuse_views(views, dims_max=48, return_volume=True)
    nv, nf = mesh["vertices"].shape[0], mesh["faces"].shape[0]
    assert nv > 0 and nf > 0 and max(vol.dims) <= 48 and vol.launches == 1
    faces = mesh["faces"].cpu().numpy()
    rv, rc, rf = FR.extract_ref(*_state(vol), vol.origin, np.float32(vol.voxel_size), 1.0, np.float32)
    rpos, kept, rfaces, rbounds = MR.compact_ref(rv, rf)
    assert np.array_equal(faces, rfaces) and len(np.unique(faces)) == nv == len(kept)            # no referenced vertex dropped, no other kept
    assert _bits(mesh["vertices"].cpu().numpy(), rpos) and np.array_equal(mesh["colors"].cpu().numpy().view(np.uint32).ravel(), rc[kept])
    path = str(tmp_path / "fused.glb")
    M.write_glb(path, mesh["vertices"], mesh["colors"], mesh["faces"], bounds=mesh["bounds"])
    glb = read_glb(path)
    assert glb["mode"] == 4 and np.array_equal(glb["indices"], faces) and np.array_equal(glb["positions"], rpos)
    assert np.array_equal(glb["colors"], mesh["colors"].cpu().numpy())


def test_add_triangles_equals_the_rasteriser_restatement(fused):
    from spann3r_amd import vis
    vol, _ = fused
    mesh = vol.extract_mesh()
    v, f = mesh["vertices"].cpu().numpy(), mesh["faces"].cpu().numpy()
    cam = vis.Camera([[60.0, 0, 31.25], [0, 61.0, 23.5], [0, 0, 1]], np.linalg.inv(FR.look_at((0.3, -2.2, 1.6), (0.0, 0.0, 0.2))), 64, 48)
    r = vis.PointRenderer(camera=cam)
    r.add_triangles(mesh["vertices"], mesh["faces"], mesh["colors"])
    rgb, depth, index = (x.cpu().numpy() for x in r.image(return_depth=True, return_index=True))
    E, K = cam.extrinsic, cam.intrinsic
    ref_cam = RR.Cam(E[:3, :3], E[:3, 3], K[0, 0], K[1, 1], K[0, 2], K[1, 2], 64, 48)
    ri, rd, big = MR.raster(v, f, None, ref_cam, 4096, dtype=np.float32)
    assert (ri >= 0).sum() > 300 and big == 0 and int(r.mesh_stats[1].item()) == 0 and int(r.mesh_stats[0].item()) == len(f)
    assert np.array_equal(index.astype(np.int64), ri)
    m = ri >= 0
    assert np.isinf(depth[~m]).all() and np.abs(depth[m].astype(np.float64) / rd[m].astype(np.float64) - 1).max() <= DEPTH_RTOL
    cols = mesh["colors"].cpu().numpy()
    assert np.array_equal(rgb[m], cols[ri[m], :3]) and (rgb[~m] == 0).all()
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.add_triangles(mesh["vertices"].cpu(), mesh["faces"], mesh["colors"])
    with pytest.raises(RuntimeError, match="mismatched lengths"):
        r.add_triangles(mesh["vertices"], mesh["faces"], mesh["colors"][:-1])


def test_fuse_sequence_smoke_on_the_tiny_model(tiny_sd):
    """the tiny model's geometry means nothing (its pointmaps give a focal near 0, which fuse_sequence refuses): with a focal and
    poses given, this only checks that the sequence runs and that the counts are consistent"""
    from spann3r_amd import Spann3R, TINY, fusion as F
    from spann3r_amd.weights import synth_frames
    m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False)
    m.load_state_dict(tiny_sd, strict=True)
    m = m.to("cuda:0").eval()
    frames = synth_frames(3, 64, 80)
    batch = [{"img": f["img"].to("cuda:0")} for f in frames]
    preds, _ = m(batch)
    with pytest.raises(RuntimeError, match="degenerate pointmaps"):                              # seeded random weights: focal ~ 1e-4
        F.fuse_sequence(preds, batch, conf_thresh=0.0, dims_max=40)
    poses = np.stack([np.eye(4)] * 3)
    poses[1, 0, 3], poses[2, 1, 3] = 0.05, -0.05
    mesh, vol = F.fuse_sequence(preds, batch, conf_thresh=0.0, dims_max=40, return_volume=True, focal=80.0, poses=poses)
    nv, nf = mesh["vertices"].shape[0], mesh["faces"].shape[0]
    assert vol.launches == 1 and max(vol.dims) <= 40 and float(vol.weight.max()) >= 1.0
    assert mesh["colors"].shape == (nv, 4) and mesh["colors"].dtype == torch.uint8 and mesh["faces"].dtype == torch.int32
    if nf:
        f = mesh["faces"].cpu().numpy()
        assert f.min() == 0 and f.max() == nv - 1 and len(np.unique(f)) == nv
        assert np.isfinite(mesh["bounds"]).all()
    else:
        assert nv == 0
