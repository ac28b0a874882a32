"""Numpy restatement of include/spann3r_hip.h, "Brick mesh extraction" (sp3_tsdf_brick_extract, csrc/brick_mesh.hip): the rule of
sp3_tsdf_extract on the densified volume of the whole virtual grid, its vertices in (slot, place, edge slot) order and its faces in
(slot of the brick of corner 0, place of corner 0, tetrahedron, triangle) order.  It is the pin of
spann3r_amd.fusion.BrickTSDFVolume.extract_raw in tests/test_brick_mesh_gpu.py; tests/test_brick_mesh_cpu.py checks the restatement
itself against fusion_ref.extract_ref.  The tables (the Kuhn cut, the edge slots, the cases) are fusion_ref's; the walk over
owners and cells is written again here because its order is what this entry point changes.  No torch."""
import numpy as np

import bricks_ref as BR
import fusion_ref as FR


def pool_keys(state):
    """slot * 512 + place of every voxel of the virtual grid, int64 [nz ny nx] in linear voxel order; -1: absent"""
    slot, place = BR._voxel_slots(state)
    return np.where(slot >= 0, slot * 512 + place, -1).reshape(-1)


def corner_flags(state, min_weight=1.0):
    """(observed, inside) bool [nz, ny, nx] of the densified volume of the whole grid"""
    D, W, _ = BR.to_dense(state)
    return W >= np.float32(min_weight), D < 0


def live_cells(obs, inside):
    """(live bool, inside byte int64) [nz, ny, nx] of the cell whose corner 0 is each voxel (False on the last layer of an axis)"""
    nz, ny, nx = obs.shape
    live = np.zeros(obs.shape, bool)
    bits = np.zeros(obs.shape, np.int64)
    live[:-1, :-1, :-1] = True
    for c in range(8):
        dx, dy, dz = FR.corner_offset(c)
        b = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
        live[:-1, :-1, :-1] &= obs[b]
        bits[:-1, :-1, :-1] |= inside[b].astype(np.int64) << c
    return live, bits


def extract(state, origin, voxel, min_weight=1.0, dtype=np.float32):
    """-> (vertices `dtype` [V, 3], rgba uint32 [V], faces int64 [F, 3]) of a bricks_ref state, in the order of the contract"""
    dt = dtype
    D32, W, col32 = BR.to_dense(state)
    D = D32.astype(dt)
    nz, ny, nx = D.shape
    n = nx * ny * nz
    key = pool_keys(state)
    obs, inside = W >= np.float32(min_weight), D32 < 0
    # vertices: slot s of voxel a carries one when b = a + step lies in the grid, both are observed and exactly one is inside
    flags = np.zeros((nz, ny, nx, 7), bool)
    for s, code in enumerate(FR.SLOT_CODE):
        dx, dy, dz = FR.corner_offset(code)
        a = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        b = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        flags[a + (s,)] = obs[a] & obs[b] & (inside[a] != inside[b])
    flags = flags.reshape(n, 7)
    cnt = flags.sum(1)
    owners = np.flatnonzero(cnt)
    assert (key[owners] >= 0).all()                                   # only an allocated voxel is observed
    owners = owners[np.argsort(key[owners], kind="stable")]           # (slot, place) order
    voff = np.zeros(n, np.int64)
    voff[owners] = np.cumsum(cnt[owners]) - cnt[owners]
    vidx = voff[:, None] + np.cumsum(flags, axis=1) - flags          # row of the vertex of (owner, slot), where flagged
    row, slot = np.nonzero(flags[owners])                             # row-major: (owner in order, slot)
    owner = owners[row]
    code = np.asarray(FR.SLOT_CODE)[slot]
    i, j, k = owner % nx, (owner // nx) % ny, owner // (nx * ny)      # indices in the VIRTUAL grid
    di, dj, dk = code & 1, (code >> 1) & 1, code >> 2
    other = owner + di + nx * (dj + ny * dk)
    flat = D.reshape(n)
    ta, tb = flat[owner], flat[other]
    with np.errstate(all="ignore"):
        t = ta / (ta - tb)
        verts = np.empty((len(owner), 3), dt)
        for ax, (ia, d) in enumerate(((i, di), (j, dj), (k, dk))):
            pa = dt(origin[ax]) + ia.astype(dt) * dt(voxel)
            pb = dt(origin[ax]) + (ia + d).astype(dt) * dt(voxel)
            verts[:, ax] = pa + t * (pb - pa)
        rgba = np.full(len(owner), 0xffffffff, np.uint32)
        if col32 is not None:
            col = col32.astype(dt).reshape(n, 3)
            rgba[:] = np.uint32(255) << np.uint32(24)
            for ch in range(3):
                ca, cb = col[owner, ch], col[other, ch]
                rgba |= FR._unorm8(ca + t * (cb - ca)) << np.uint32(8 * ch)
    # faces
    live, bits = (x.reshape(n) for x in live_cells(obs, inside))
    out = np.full((n, 6, 2, 3), -1, np.int64)
    has = np.zeros((n, 6, 2), bool)
    for ti, tet in enumerate(FR.TET):
        cs = sum(((bits >> tet[m]) & 1) << m for m in range(4))
        for case in range(1, 15):
            sel = np.flatnonzero(live & (cs == case))
            for q, tri in enumerate(FR.CASES[case]):
                has[sel, ti, q] = True
                for xk, (p0, p1) in enumerate(tri):
                    lo, hi = sorted((tet[p0], tet[p1]))
                    dx, dy, dz = FR.corner_offset(lo)
                    out[sel, ti, q, xk] = vidx[sel + dx + nx * (dy + ny * dz), FR.SLOT_OF[hi - lo]]
    cells = np.flatnonzero(has.any((1, 2)))
    assert (key[cells] >= 0).all()                                    # corner 0 of a live cell is observed, so allocated
    cells = cells[np.argsort(key[cells], kind="stable")]
    faces = out[cells][has[cells]]
    return verts, rgba, faces.reshape(-1, 3)
