"""The numpy restatement of the ray-caster and of the frame-to-model tracking (tests/raycast_ref.py) checked on its own: what fp32
costs against float64, the ray-cast depth against the analytic depth of the scene, and the registration property -- a frame moved
rigidly together with its pose comes back.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
import fusion_ref as FR
import raycast_ref as RC

S = RC.SCENE
VOL = (np.float32(S["origin"]), np.float32(S["voxel"]))


@pytest.fixture(scope="module")
def frames():
    return RC.scene_frames()


@pytest.fixture(scope="module")
def fused(frames):
    return RC.fuse_ref(frames)


@pytest.fixture(scope="module")
def casts(frames, fused):
    """every scene view ray-cast in fp32 and in float64"""
    return [(RC.raycast_ref(*fused, *VOL, RC.scene_view(fr), dtype=np.float32), RC.raycast_ref(*fused, *VOL, RC.scene_view(fr), dtype=np.float64))
            for fr in frames]


def test_float32_against_float64(casts):
    """What the number format alone costs on this scene, at the pixels both hit whose march stopped in the same interval (a sample
    value near 0 can change sign between the formats; the hit then moves by a step and says nothing about rounding).  Recorded here:
    depth 1.7e-6, vertex 1.8e-6, normal 1.5e-5 (the gradient is a difference of nearly equal values over their small length);
    4 x those is the fallback bound tests/test_raycast_gpu.py names for a map that could not be made bit-equal.
    Asserted: 32 ulp of the largest depth of the scene (2^-23 x 2.5 x 32 < 1e-5) for depth and vertex -- the fraction
    f_prev / (f_prev - f) sees the rounding of the sample position divided by the voxel -- and ten times that for the normal."""
    worst = dict(depth=0.0, vertex=0.0, normal=0.0)
    for a, b in casts:
        both = a["hit"] & b["hit"]
        assert (a["hit"] != b["hit"]).mean() < 0.01 and 0.4 <= both.mean() <= 0.76          # 25-56 % of the rays miss: both outcomes in every view
        same = both & (np.abs(a["depth"] - b["depth"]) < 0.25 * S["voxel"])
        assert same.sum() >= 0.99 * both.sum()
        for k in worst:
            worst[k] = max(worst[k], float(np.abs(a[k].astype(np.float64) - b[k])[same].max()))
        assert np.abs(np.linalg.norm(a["normal"][a["hit"]].astype(np.float64), axis=-1) - 1).max() < 1e-6
        assert (a["depth"][~a["hit"]] == 0).all() and (a["rgba"][~a["hit"]] == 0).all() and (a["rgba"][a["hit"]] >> 24 == 255).all()
    print("fp32 against float64:", worst)
    assert worst["depth"] <= 1e-5 and worst["vertex"] <= 1e-5 and worst["normal"] <= 1e-4


def test_depth_against_the_analytic_scene(frames, casts):
    """the ray-cast depth of the fused volume against the analytic depth it was fused from, away from depth discontinuities: the
    median per view stays below a quarter voxel (measured 0.0014-0.0015, 0.04 voxel, 90 % of the pixels below 0.0042: the bias of
    projective distances and of the trilinear interpolant at voxel 0.04), and the normals agree with the analytic ones"""
    for fr, (_, c) in zip(frames, casts):
        d = fr["depth"].astype(np.float64)
        m = c["hit"] & RC.smooth_mask(d, S["voxel"] / 2)
        err = np.abs(c["depth"] - d)[m]
        print("pixels", int(m.sum()), "median", float(np.median(err)), "p90", float(np.quantile(err, 0.9)))
        assert m.sum() > 800 and np.median(err) <= S["voxel"] / 4
        floor = m & (np.abs(fr["pts"][..., 2]) < 1e-4)                                      # pixels of the plane z = 0: normal +z
        assert floor.sum() > 50 and np.median(c["normal"][floor][:, 2]) > 0.95


def _leftovers(Ts, motions):
    return [(RC.motion_size(M), RC.motion_size(T @ M)) for T, M in list(zip(Ts, motions))[1:]]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tracking_recovers_a_rigid_motion(frames, seed):
    """frames 1..5 moved by 2 degrees and a voxel each, pointmap and pose alike; tracked sequentially with the defaults, every frame's
    leftover rotation and translation are at most half of what it started with"""
    motions = RC.perturbations(seed)
    Ts, infos, _ = RC.track_sequence_ref(RC.perturbed_frames(frames, motions))
    for i, ((r0, t0), (r1, t1)) in enumerate(_leftovers(Ts, motions), 1):
        print("seed", seed, "frame", i, "start %.2f deg %.4f" % (r0, t0), "end %.3f deg %.4f" % (r1, t1), infos[i])
        assert infos[i]["tracked"] and infos[i]["pairs"] > 1000
        assert abs(r0 - 2.0) < 1e-6 and 0.029 < t0 < 0.05
        assert r1 <= 0.5 * r0 and t1 <= 0.5 * t0


def test_a_frame_that_cannot_be_registered_comes_back_as_identity(frames, fused):
    origin, voxel, trunc = np.float32(S["origin"]), np.float32(S["voxel"]), np.float32(S["trunc"])
    fr = frames[1]
    T, info = RC.track_frame_ref(fused, origin, voxel, trunc, fr["pts"], np.zeros_like(fr["valid"]), fr["K"], fr["cam2world"])
    assert np.array_equal(T, np.eye(4)) and info["tracked"] is False and info["pairs"] == 0
    empty = FR.empty_volume(S["dims"], False)                                                # a model with no hit
    T, info = RC.track_frame_ref(empty, origin, voxel, trunc, fr["pts"], fr["valid"], fr["K"], fr["cam2world"])
    assert np.array_equal(T, np.eye(4)) and info["tracked"] is False and info["pairs"] == 0
    pts = np.zeros_like(fr["pts"])                                                           # one point for every pixel: rank-deficient or too far
    T, info = RC.track_frame_ref(fused, origin, voxel, trunc, pts, fr["valid"], fr["K"], fr["cam2world"])
    assert np.array_equal(T, np.eye(4)) and info["tracked"] is False


def test_tsdf_view_ctypes_mirror_matches_the_header(tmp_path):
    """sizeof / offsetof of sp3_tsdf_view as gcc sees include/spann3r_hip.h equal spann3r_amd.lib.TsdfView; the new entry points
    validate before they launch"""
    from spann3r_amd import lib
    fields = [f[0] for f in lib.TsdfView._fields_]
    src = ['#include "%s"' % os.path.join(REPO, "include", "spann3r_hip.h"), "#include <stdio.h>", "#include <stddef.h>", "int main(){",
           'printf("%zu\\n", sizeof(sp3_tsdf_view));'] + ['printf("%%zu\\n", offsetof(sp3_tsdf_view, %s));' % f for f in fields] + ["return 0;}"]
    c, exe = str(tmp_path / "p.c"), str(tmp_path / "p")
    open(c, "w").write("\n".join(src) + "\n")
    subprocess.check_call(["gcc", c, "-o", exe])
    vals = [int(x) for x in subprocess.check_output([exe]).split()]
    assert vals == [ctypes.sizeof(lib.TsdfView)] + [getattr(lib.TsdfView, f).offset for f in fields]
    l = lib.load()
    o = (ctypes.c_float * 3)(0, 0, 0)
    assert l.sp3_tsdf_raycast(None, None, 1, 8, 8, 8, o, 0.1, None, None, None, 0.0, 0.1, None) != 0 and b"min_weight" in l.sp3_last_error()
    assert l.sp3_tsdf_raycast(None, None, 1, 8, 8, 8, o, 0.1, None, None, None, 1.0, 0.1, None) != 0 and b"null views" in l.sp3_last_error()
    assert l.sp3_tsdf_raycast(None, None, 0, 8, 8, 8, o, 0.1, None, None, None, 1.0, 0.1, None) == 0
    assert l.sp3_tsdf_track_accum_ws_bytes(3072) == 12 * 29 * 8
