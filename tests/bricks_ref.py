"""Numpy restatement of the rules of include/spann3r_hip.h, "Brick TSDF volume": mark, alloc, integrate and to_dense of the
two-level volume (csrc/bricks.hip), plus the scene the brick tests use.  It is the pin of spann3r_amd.fusion.BrickTSDFVolume in
tests/test_bricks_gpu.py; tests/test_bricks_cpu.py checks the restatement itself.  There is no reference implementation.

The per-voxel step is not written again: `integrate` densifies the bricks, runs fusion_ref.integrate_ref on the whole virtual
grid and keeps the allocated voxels.  The ray-caster's restatement is raycast_ref.raycast_ref applied to `to_dense` of the full grid.
State: dict(dims, bricks, table int32 [bx by bz], slot_brick int32 [capacity], count, tsdf / weight fp32 [capacity, 512], rgb fp32
[capacity, 512, 3] or None).  No torch."""
import numpy as np

import fusion_ref as FR
import raycast_ref as RC

# ------------------------------------------------------------------------------------------------ the scene of the tests
# raycast_ref's room corner at half its voxel size, in a grid of whole bricks that covers its volume
SCENE = dict(dims=(88, 72, 48), origin=RC.SCENE["origin"], voxel=0.02, trunc=0.06, band=0.06, h=RC.SCENE["h"], w=RC.SCENE["w"])


def empty(dims, capacity, color=True):
    assert all(d % 8 == 0 for d in dims)
    bricks = tuple(d // 8 for d in dims)
    return dict(dims=tuple(dims), bricks=bricks, table=np.full(bricks[0] * bricks[1] * bricks[2], -1, np.int32),
                slot_brick=np.zeros(capacity, np.int32), count=0, tsdf=np.zeros((capacity, 512), np.float32),
                weight=np.zeros((capacity, 512), np.float32), rgb=np.zeros((capacity, 512, 3), np.float32) if color else None)


def frame_points(fr):
    """(P fp32 [h, w, 3], ok [h, w]) of one frame by the mark rule: the pixel tests of the integrate rule and the point of a pixel"""
    f32 = np.float32
    m = np.asarray(fr["w2c"], f32).reshape(12)
    src = fr["depth"] if fr.get("depth") is not None else fr["pts"]
    h, w = src.shape[:2]
    ok = np.ones((h, w), bool)
    if fr.get("valid") is not None:
        ok &= np.asarray(fr["valid"]) != 0
    with np.errstate(all="ignore"):
        if fr.get("depth") is not None:
            d = np.asarray(fr["depth"], f32)
            c = np.asarray(fr["cam2world"], np.float64)[:3].astype(f32)                # row-major 3 x 4: R | eye
            ys, xs = np.mgrid[0:h, 0:w]
            xn, yn = (xs.astype(f32) - f32(fr["cu"])) / f32(fr["fu"]), (ys.astype(f32) - f32(fr["cv"])) / f32(fr["fv"])
            X, Y = xn * d, yn * d
            P = np.stack([((c[r, 0] * X + c[r, 1] * Y) + c[r, 2] * d) + c[r, 3] for r in range(3)], -1)
        else:
            P = np.asarray(fr["pts"], f32)
            d = ((m[8] * P[..., 0] + m[9] * P[..., 1]) + m[10] * P[..., 2]) + m[11]
        ok &= np.isfinite(d) & (d > 0)
        if fr.get("pixel_weight") is not None:
            a = np.asarray(fr["pixel_weight"], f32)
            ok &= (a > 0) & np.isfinite(a)
        ok &= np.isfinite(P).all(-1)
    return P, ok


def mark(frames, dims, origin, voxel, band, flags=None, return_span=False):
    """flags uint8 [bx by bz] after marking the frames (onto `flags` when given); with return_span also the largest number of bricks a
    pixel touched on an axis"""
    f32 = np.float32
    bricks = tuple(d // 8 for d in dims)
    flags = np.zeros(bricks[0] * bricks[1] * bricks[2], np.uint8) if flags is None else flags.copy()
    grid = flags.reshape(bricks[2], bricks[1], bricks[0])
    span = 0
    for fr in frames:
        P, ok = frame_points(fr)
        P = P[ok]
        lo, hi = [], []
        keep = np.ones(len(P), bool)
        with np.errstate(all="ignore"):
            for a in range(3):
                l = np.floor(((P[:, a] - f32(band)) - f32(origin[a])) / f32(voxel))
                u = np.floor(((P[:, a] + f32(band)) - f32(origin[a])) / f32(voxel)) + f32(1)
                keep &= (u >= 0) & (l <= dims[a] - 1)
                lo.append(np.clip(l, 0, dims[a] - 1))
                hi.append(np.clip(u, 0, dims[a] - 1))
        b0 = [lo[a][keep].astype(np.int64) >> 3 for a in range(3)]
        b1 = [hi[a][keep].astype(np.int64) >> 3 for a in range(3)]
        for p in range(len(b0[0])):
            grid[b0[2][p]:b1[2][p] + 1, b0[1][p]:b1[1][p] + 1, b0[0][p]:b1[0][p] + 1] = 1
        if len(b0[0]):
            span = max(span, max(int((b1[a] - b0[a]).max()) + 1 for a in range(3)))
    return (flags, span) if return_span else flags


def alloc(state, flags):
    """-> (state', flags', (count, need)): all or nothing, the new bricks in linear brick order"""
    new = np.flatnonzero((flags != 0) & (state["table"] < 0))
    need = state["count"] + len(new)
    capacity = len(state["slot_brick"])
    if need > capacity:
        return state, flags, (state["count"], need)
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    slots = state["count"] + np.arange(len(new))
    s["table"][new] = slots
    s["slot_brick"][slots] = new
    s["tsdf"][slots], s["weight"][slots] = 1.0, 0.0
    if s["rgb"] is not None:
        s["rgb"][slots] = 0.0
    s["count"] = need
    return s, np.zeros_like(flags), (need, need)


def grow(state, capacity):
    """the pool at a larger capacity, the slots in use copied"""
    s = empty(state["dims"], capacity, state["rgb"] is not None)
    n = state["count"]
    s["table"], s["count"] = state["table"].copy(), n
    for k in ("slot_brick", "tsdf", "weight", "rgb"):
        if state[k] is not None:
            s[k][:n] = state[k][:n]
    return s


def _voxel_slots(state):
    """(slot int64 [nz, ny, nx] (-1: absent), place int64 [nz, ny, nx]) of every voxel of the virtual grid"""
    nx, ny, nz = state["dims"]
    bx, by, _ = state["bricks"]
    k, j, i = np.mgrid[0:nz, 0:ny, 0:nx]
    slot = state["table"].astype(np.int64)[((k >> 3) * by + (j >> 3)) * bx + (i >> 3)]
    return slot, (k & 7) * 64 + (j & 7) * 8 + (i & 7)


def to_dense(state, box=None):
    """the densified volume of box = (lo, size) in voxels (default: the whole grid): (tsdf, weight, rgb or None), absent = (1, 0, 0)"""
    slot, place = _voxel_slots(state)
    ok = slot >= 0
    s = np.where(ok, slot, 0)
    D = np.where(ok, state["tsdf"][s, place], np.float32(1)).astype(np.float32)
    W = np.where(ok, state["weight"][s, place], np.float32(0)).astype(np.float32)
    col = None if state["rgb"] is None else np.where(ok[..., None], state["rgb"][s, place], np.float32(0)).astype(np.float32)
    if box is not None:
        (lx, ly, lz), (sx, sy, sz) = box
        sel = (slice(lz, lz + sz), slice(ly, ly + sy), slice(lx, lx + sx))
        D, W, col = D[sel], W[sel], None if col is None else col[sel]
    return D, W, col


def integrate_slots(state, frames, origin, voxel, trunc):
    """sp3_tsdf_brick_integrate: the frames into the allocated bricks, by fusion_ref.integrate_ref on the densified grid in fp32"""
    D, W, col = FR.integrate_ref(*to_dense(state), frames, np.float32(origin), np.float32(voxel), np.float32(trunc), np.float32)
    slot, place = _voxel_slots(state)
    ok = slot >= 0
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    s["tsdf"][slot[ok], place[ok]] = D[ok]
    s["weight"][slot[ok], place[ok]] = W[ok]
    if col is not None:
        s["rgb"][slot[ok], place[ok]] = col[ok]
    return s


def integrate(state, frames, origin, voxel, trunc, band):
    """BrickTSDFVolume.integrate: mark, alloc (the pool doubling until `need` fits), integrate.  -> (state', times grown)"""
    flags = mark(frames, state["dims"], origin, voxel, band)
    grown = 0
    while True:
        state, flags, (_, need) = alloc(state, flags)
        if need <= len(state["slot_brick"]):
            break
        capacity = len(state["slot_brick"])
        while capacity < need:
            capacity *= 2
        state = grow(state, min(capacity, len(state["table"])))
        grown += 1
    return integrate_slots(state, frames, origin, voxel, trunc), grown


def scene_frames(path="pts"):
    """raycast_ref's six frames through one source, with the cam2world the depth path of `mark` needs"""
    return FR.as_path(RC.scene_frames(), path)


def scene_view(fr, **kw):
    return RC.scene_view(fr, **kw)
