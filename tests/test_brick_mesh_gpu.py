"""BrickTSDFVolume.extract_raw / extract_mesh(direct=True) on the device (csrc/brick_mesh.hip; include/spann3r_hip.h "Brick mesh
extraction").

Every comparison is bit for bit.  The anchors: tests/brick_mesh_ref.py (the restatement, rows in order) fed the device's own pool,
downloaded, so that the two sides start from the same bits; and the dense kernel sp3_tsdf_extract on to_dense() of the same pool,
which must give the same triangles and the same vertices as sets of rows (9 position words + 3 rgba words per face).  The scene is
bricks_ref.SCENE (376 bricks; V = 45178, F = 86084, 546 vertices no face uses: pinned in tests/test_brick_mesh_cpu.py together with
the cells that straddle brick faces, edges and corners), and for the extent a 1024 x 192 x 128 grid whose voxel centres are exact
in fp32, so that the virtual grid's origin rule and a box's give the same bits."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

import brick_mesh_ref as BM
import bricks_ref as BR
import fusion_ref as FR
import raycast_ref as RC
from test_brick_mesh_cpu import V, F, UNUSED, face_rows, vertex_rows, sorted_rows

pytestmark = pytest.mark.gpu

S = BR.SCENE
FULL = ((0, 0, 0), S["dims"])
EXTENT = ((-0.8, -0.7, -0.1), (0.85, 0.65, 0.8))


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _brick(color=True, **kw):
    from spann3r_amd import fusion as F_
    kw = dict(dict(origin=S["origin"], voxel_size=S["voxel"], dims=S["dims"], trunc=S["trunc"], band=S["band"]), **kw)
    return F_.BrickTSDFVolume(color=color, **kw)


def _args(frs, images=True):
    kw = dict(intrinsics=[f["K"] for f in frs], cam2world=[f["cam2world"] for f in frs], valid=[_t(f["valid"]) for f in frs],
              pts=[_t(f["pts"]) for f in frs])
    if images:
        kw["images"] = [_t(f["images"]) for f in frs]
    return kw


def _state(vol):
    """the device's pool as a bricks_ref state"""
    n = vol.n_bricks
    return dict(dims=vol.dims, bricks=vol.bricks, table=vol.table.cpu().numpy(), slot_brick=vol.slot_brick.cpu().numpy(), count=n,
                tsdf=vol.tsdf.cpu().numpy(), weight=vol.weight.cpu().numpy(), rgb=None if vol.rgb is None else vol.rgb.cpu().numpy())


def _raw(vol, min_weight=1.0, cap_v=None, cap_f=None):
    """extract_raw, downloaded and cut to the counts: (vertices, rgba uint32, faces, V, F)"""
    v, c, f, counts = vol.extract_raw(min_weight, cap_v, cap_f)
    nv, nf = counts.cpu().tolist()
    assert nv <= v.shape[0] and nf <= f.shape[0]
    return v[:nv].cpu().numpy(), c[:nv].cpu().numpy().view(np.uint32), f[:nf].cpu().numpy(), nv, nf


def _mesh_rows(m):
    """the face rows of a mesh dict, sorted"""
    return sorted_rows(face_rows(m["vertices"].cpu().numpy(), m["colors"].cpu().numpy().view(np.uint32).ravel(), m["faces"].cpu().numpy().astype(np.int64)))


@pytest.fixture(scope="module")
def frames():
    return RC.scene_frames()


@pytest.fixture(scope="module")
def volumes(frames):
    """the scene fused in one call and in two (frames[:2], then frames[2:]), with and without colours"""
    out = {}
    for color in (True, False):
        out[1, color] = _brick(color).integrate(**_args(frames, color))
        out[2, color] = _brick(color).integrate(**_args(frames[:2], color)).integrate(**_args(frames[2:], color))
    return out


@pytest.fixture(scope="module")
def fused(volumes):
    """(the one-call volume with colours, its extract_raw downloaded)"""
    vol = volumes[1, True]
    return vol, _raw(vol)


# ------------------------------------------------------------------------------------------------ 1. the restatement, rows in order
@pytest.mark.parametrize("calls", [1, 2])
@pytest.mark.parametrize("color", [True, False])
def test_extract_raw_equals_the_restatement_row_for_row(volumes, calls, color):
    vol = volumes[calls, color]
    state = _state(vol)
    assert vol.n_bricks == 376 and ((np.diff(state["slot_brick"][:376]) < 0).any() == (calls == 2))
    rv, rc, rf = BM.extract(state, vol.origin, np.float32(vol.voxel_size), 1.0, np.float32)
    gv, gc, gf, nv, nf = _raw(vol)
    print("calls", calls, "color", color, "V", nv, "F", nf)
    assert (nv, nf) == (len(rv), len(rf)) == (V, F)
    assert np.array_equal(gf, rf)
    assert _bits(gv, rv), float(np.abs(gv - rv).max())
    assert np.array_equal(gc, rc) and ((gc == 0xffffffff).all() == (not color))
    again = _raw(vol)
    assert _bits(again[0], gv) and np.array_equal(again[1], gc) and np.array_equal(again[2], gf)  # the same bits every run


# ------------------------------------------------------------------------------------------------ 2. the dense kernel
@pytest.mark.parametrize("calls", [1, 2])
def test_extract_raw_equals_the_dense_kernel_as_sets_of_rows(volumes, calls):
    vol = volumes[calls, True]
    gv, gc, gf, nv, nf = _raw(vol)
    dv, dc, df, counts = vol.to_dense(FULL).extract_raw()
    dnv, dnf = counts.cpu().tolist()
    assert (nv, nf) == (dnv, dnf) == (V, F)
    dv, dc, df = dv[:dnv].cpu().numpy(), dc[:dnv].cpu().numpy().view(np.uint32), df[:dnf].cpu().numpy()
    assert np.array_equal(sorted_rows(face_rows(gv, gc, gf)), sorted_rows(face_rows(dv, dc, df)))
    assert np.array_equal(sorted_rows(vertex_rows(gv, gc)), sorted_rows(vertex_rows(dv, dc)))
    assert not np.array_equal(gf, df)                                                            # (the order is another one)


# ------------------------------------------------------------------------------------------------ 3. capacities
def test_capacities_are_respected_and_counts_hold_the_need(fused):
    from spann3r_amd import lib as L
    vol, (v, c, f, nv, nf) = fused
    cap_v, cap_f, room_v, room_f = nv // 2, nf // 3, nv + 64, nf + 64
    lib = L.load()
    bv = torch.full((room_v, 3), -7.0, device="cuda")
    bc = torch.full((room_v,), 12345, dtype=torch.int32, device="cuda")
    bf = torch.full((room_f, 3), -9, dtype=torch.int32, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.sp3_tsdf_brick_extract_ws_bytes(vol.n_bricks)), dtype=torch.uint8, device="cuda")
    assert ws.numel() >= 5 * 512 * vol.n_bricks and ws.numel() < 5 * 512 * vol.n_bricks + 16 * vol.n_bricks + 128      # per allocated voxel
    L.check(lib.sp3_tsdf_brick_extract(*vol.dims, vol._origin_c, vol.voxel_size, vol.table.data_ptr(), vol.slot_brick.data_ptr(), vol.n_bricks,
                                       vol.tsdf.data_ptr(), vol.weight.data_ptr(), L.ptr(vol.rgb), 1.0, ws.data_ptr(), cap_v, cap_f,
                                       bv.data_ptr(), bc.data_ptr(), bf.data_ptr(), counts.data_ptr(), L.stream_ptr()), "sp3_tsdf_brick_extract")
    assert counts.cpu().tolist() == [nv, nf]                                                     # the need, not the capacity
    assert _bits(bv[:cap_v].cpu().numpy(), v[:cap_v]) and np.array_equal(bc[:cap_v].cpu().numpy().view(np.uint32), c[:cap_v])
    assert np.array_equal(bf[:cap_f].cpu().numpy(), f[:cap_f])
    assert (bv[cap_v:] == -7.0).all() and (bc[cap_v:] == 12345).all() and (bf[cap_f:] == -9).all()


def test_extract_mesh_direct_retries_once_when_its_first_guess_overflows(frames):
    """a pool of noise, as in the dense overflow test: far more vertices than a quarter of the allocated voxels"""
    vol = _brick(False).integrate(**_args(frames, False))
    rng = np.random.default_rng(5)
    n = vol.n_bricks
    vol.tsdf[:n].copy_(_t(rng.uniform(-1, 1, (n, 512)).astype(np.float32)))
    vol.weight[:n].copy_(_t((rng.random((n, 512)) < 0.95).astype(np.float32)))
    nv, nf = vol.extract_raw()[3].cpu().tolist()
    assert nv > max(4096, 512 * n // 4)                                                          # over the first guess
    a, b = vol.extract_mesh(direct=True), vol.to_dense(FULL).extract_mesh()
    assert a["faces"].shape[0] == nf == b["faces"].shape[0] and a["vertices"].shape == b["vertices"].shape
    assert np.array_equal(_mesh_rows(a), _mesh_rows(b)) and np.array_equal(a["bounds"], b["bounds"])
    assert (a["colors"] == 255).all()


# ------------------------------------------------------------------------------------------------ 4. extract_mesh(direct=True)
def test_extract_mesh_direct_equals_the_dense_route(fused):
    vol, _ = fused
    a, b = vol.extract_mesh(direct=True), vol.to_dense(FULL).extract_mesh()
    assert sorted(a) == sorted(b) == ["bounds", "colors", "faces", "vertices"]
    assert a["faces"].shape == (F, 3) and a["vertices"].shape == (V - UNUSED, 3) == b["vertices"].shape and a["colors"].shape == (V - UNUSED, 4)
    assert a["faces"].dtype == torch.int32 and a["colors"].dtype == torch.uint8
    assert np.array_equal(_mesh_rows(a), _mesh_rows(b))
    assert np.array_equal(a["bounds"], b["bounds"])
    ra, rb = FR.manifold_report(a["faces"].cpu().numpy()), FR.manifold_report(b["faces"].cpu().numpy())
    print("boundary edges", len(ra["boundary"]), "euler", ra["euler"])
    assert ra["bad"] == 0 and len(ra["boundary"]) == len(rb["boundary"]) and ra["euler"] == rb["euler"]
    T = np.array([[0, -1, 0, 0.5], [1, 0, 0, -0.25], [0, 0, 1, 2.0], [0, 0, 0, 1]], np.float64)
    a2, b2 = vol.extract_mesh(2.0, 10.0, T, direct=True), vol.to_dense(FULL).extract_mesh(2.0, 10.0, T)
    assert 0 < a2["faces"].shape[0] < F and np.array_equal(_mesh_rows(a2), _mesh_rows(b2)) and np.array_equal(a2["bounds"], b2["bounds"])
    assert not np.array_equal(a2["bounds"], a["bounds"])
    with pytest.raises(ValueError, match="min_weight"):
        vol.extract_mesh(0.0, direct=True)


# ------------------------------------------------------------------------------------------------ 5. edge cases
def test_empty_volume_no_observed_voxel_and_the_index_limit(fused):
    from spann3r_amd import fusion as F_, lib as L
    fresh = _brick()
    a, b = fresh.extract_mesh(direct=True), fresh.extract_mesh()
    assert fresh.n_bricks == 0 and sorted(a) == sorted(b)
    for k in ("vertices", "colors", "faces"):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].shape[0] == 0, k
    assert np.array_equal(a["bounds"], b["bounds"], equal_nan=True)
    counts = torch.full((2,), 77, dtype=torch.int32, device="cuda")                               # n_bricks = 0 writes (0, 0)
    lib = L.load()
    L.check(lib.sp3_tsdf_brick_extract(*fresh.dims, fresh._origin_c, fresh.voxel_size, None, None, 0, None, None, None, 1.0, None, 0, 0, None, None,
                                       None, counts.data_ptr(), L.stream_ptr()), "sp3_tsdf_brick_extract")
    assert counts.cpu().tolist() == [0, 0]
    vol, _ = fused
    top = float(vol.weight[:vol.n_bricks].max())
    assert vol.extract_raw(top + 1.0)[3].cpu().tolist() == [0, 0] and vol.extract_mesh(top + 1.0, direct=True)["faces"].shape == (0, 3)
    # over 12 * 512 * n_bricks < 2^31: an error before anything is launched (null buffers), ValueError with the count from Python
    o = (C.c_float * 3)(0, 0, 0)
    limit = (2 ** 31 - 1) // (12 * 512)
    assert F_.BRICK_MESH_LIMIT == limit and lib.sp3_tsdf_brick_extract_ws_bytes(limit) > 0 and lib.sp3_tsdf_brick_extract_ws_bytes(limit + 1) == 0
    assert lib.sp3_tsdf_brick_extract(1024, 1024, 1024, o, 0.1, None, None, limit + 1, None, None, None, 1.0, None, 0, 0, None, None, None, None, None) != 0
    assert b"index limit" in lib.sp3_last_error() and str(limit + 1).encode() in lib.sp3_last_error()
    assert lib.sp3_tsdf_brick_extract(8, 12, 8, o, 0.1, None, None, 0, None, None, None, 1.0, None, 0, 0, None, None, None, None, None) != 0
    assert b"multiples of 8" in lib.sp3_last_error()
    big = _brick(False, dims=(1024, 1024, 1024), capacity=1)
    big.n_bricks = limit + 1                                                                      # (made up: nothing is launched)
    with pytest.raises(ValueError, match=str(limit + 1)):
        big.extract_raw()


# ------------------------------------------------------------------------------------------------ 6. extent
def test_a_grid_the_dense_route_cannot_mesh(frames):
    """two copies of the scene 12 units apart in one 1024 x 192 x 128 grid: 902 + 902 bricks with nothing between them"""
    from spann3r_amd import fusion as F_
    dims, voxel, origin = (1024, 192, 128), 1.0 / 64, (-1.0, -1.5, -0.25)
    far = []
    for f in frames:
        P = f["cam2world"].copy()
        P[0, 3] += 12.0
        far.append(dict(f, pts=f["pts"] + np.float32([12, 0, 0]), cam2world=P))
    vol = F_.BrickTSDFVolume(origin, voxel, dims, trunc=3.0 / 64, band=3.0 / 64).integrate(**_args(frames + far))
    grid = (vol.table.cpu().numpy() >= 0).reshape(16, 24, 128)
    cols = np.flatnonzero(grid.any((0, 1))).tolist()
    assert vol.n_bricks == 1804 and cols == list(range(1, 18)) + list(range(97, 114))
    assert int(grid[:, :, :64].sum()) == 902 and int(grid[:, :, 64:].sum()) == 902
    dense_bytes = 20 * dims[0] * dims[1] * dims[2]
    print("bytes held: %.1f MB of bricks against %.1f MB dense" % (vol.memory_bytes / 1e6, dense_bytes / 1e6))
    assert vol.memory_bytes < dense_bytes // 10
    with pytest.raises(ValueError, match="dims_limit"):
        vol.extract_mesh()
    m = vol.extract_mesh(direct=True)
    halves = [vol.to_dense(((x, 0, 0), (512, 192, 128))).extract_mesh() for x in (0, 512)]
    assert min(h["faces"].shape[0] for h in halves) > 50000
    want = np.concatenate([_mesh_rows(h) for h in halves])
    assert m["faces"].shape[0] == len(want) and np.array_equal(_mesh_rows(m), sorted_rows(want))
    assert m["vertices"].shape[0] == sum(h["vertices"].shape[0] for h in halves)
    assert m["bounds"][1, 0] - m["bounds"][0, 0] > 12.0


# ------------------------------------------------------------------------------------------------ 7. drivers
def test_session_and_fuse_pointmaps_pass_direct_through(frames):
    from spann3r_amd import fusion as F_
    moved = RC.perturbed_frames(frames, RC.perturbations(3))
    ses = F_.FusionSession(S["voxel"], EXTENT, track=True)
    for f in moved:
        ses.push(_t(f["pts"]), f["K"], f["cam2world"], _t(f["valid"]), _t(f["images"]))
    args = (torch.stack([_t(f["pts"]) for f in moved]), np.stack([f["K"] for f in moved]), np.stack([f["cam2world"] for f in moved]),
            torch.stack([_t(f["valid"]) for f in moved]).bool(), torch.stack([_t(f["images"]) for f in moved]))
    kw = dict(voxel_size=S["voxel"], track=True, bricks=True, extent=EXTENT)
    a, b = ses.mesh(direct=True), F_.fuse_pointmaps(*args, direct_mesh=True, **kw)
    for k in ("vertices", "colors", "faces"):
        assert torch.equal(a[k], b[k]), k                                                         # row for row
    assert np.array_equal(a["bounds"], b["bounds"]) and a["faces"].shape[0] > 5000
    assert a["faces"].shape[0] == ses.mesh()["faces"].shape[0] == F_.fuse_pointmaps(*args, **kw)["faces"].shape[0]
    assert np.array_equal(_mesh_rows(a), _mesh_rows(ses.volume.to_dense(((0, 0, 0), ses.volume.dims)).extract_mesh()))
    with pytest.raises(ValueError, match="direct_mesh"):
        F_.fuse_pointmaps(*args, voxel_size=S["voxel"], direct_mesh=True)


def test_demo_loop_rejects_direct_mesh_without_bricks(monkeypatch, capsys):
    import demo_loop
    monkeypatch.setattr(sys, "argv", ["demo_loop.py", "--tiny", "--fused", "--direct_mesh"])
    with pytest.raises(SystemExit) as e:
        demo_loop.main()
    assert e.value.code == 2 and "--direct_mesh needs --bricks" in capsys.readouterr().err
