"""The numpy restatement of the brick mesh extraction (tests/brick_mesh_ref.py) checked against the dense restatement
(fusion_ref.extract_ref on the densified grid), and the scene the GPU tests use pinned: its counts, the cells that straddle brick
faces, edges and corners, and a two-call state whose slot order is not the brick order.  Everything in fp32.  No GPU."""
import numpy as np
import pytest

import brick_mesh_ref as BM
import bricks_ref as BR
import fusion_ref as FR

S = BR.SCENE
V, F, UNUSED = 45178, 86084, 546
ARGS = (np.float32(S["origin"]), np.float32(S["voxel"]), 1.0, np.float32)


def _integrate(state, frames):
    return BR.integrate(state, frames, S["origin"], S["voxel"], S["trunc"], S["band"])[0]


def face_rows(verts, rgba, faces):
    """one row per face: the 9 position words and the 3 rgba words of its corners, as uint32 [F, 12]"""
    v = np.ascontiguousarray(verts, np.float32).view(np.uint32)
    return np.concatenate([v[faces].reshape(len(faces), 9), np.asarray(rgba, np.uint32)[faces]], axis=1)


def vertex_rows(verts, rgba):
    return np.concatenate([np.ascontiguousarray(verts, np.float32).view(np.uint32), np.asarray(rgba, np.uint32)[:, None]], axis=1)


def sorted_rows(rows):
    return rows[np.lexsort(rows.T[::-1])]


@pytest.fixture(scope="module")
def frames():
    return BR.scene_frames("pts")


@pytest.fixture(scope="module")
def one(frames):
    """(the state after ONE integrate call of the six frames, its extraction by the restatement)"""
    state = _integrate(BR.empty(S["dims"], 4096), frames)
    assert state["count"] == 376
    return state, BM.extract(state, *ARGS)


@pytest.fixture(scope="module")
def dense(one):
    return FR.extract_ref(*BR.to_dense(one[0]), *ARGS)


def test_faces_and_vertices_equal_the_dense_restatement_as_multisets(one, dense):
    v, c, f = one[1]
    dv, dc, df = dense
    assert (len(v), len(f)) == (len(dv), len(df)) == (V, F)
    assert np.array_equal(sorted_rows(face_rows(v, c, f)), sorted_rows(face_rows(dv, dc, df)))
    assert np.array_equal(sorted_rows(vertex_rows(v, c)), sorted_rows(vertex_rows(dv, dc)))
    assert len(np.unique(c)) > 1000                                                              # colours take part


def test_scene_counts(one):
    v, c, f = one[1]
    assert V - len(np.unique(f)) == UNUSED                                                        # vertices that no face uses exist
    assert len(np.unique(np.ascontiguousarray(v).view(np.uint32), axis=0)) == V                   # no two vertices with equal position
    assert f.min() == 0 and f.max() < V and FR.manifold_report(f)["bad"] == 0


def _lattice(state, v):
    """positions in voxel units of the virtual grid, float64"""
    return (v.astype(np.float64) - np.float32(S["origin"]).astype(np.float64)) / float(np.float32(S["voxel"]))


def _in_order_of_keys(key, count):
    """the voxels with count > 0 in (slot, place) order, each repeated `count` times: (i, j, k) int64 [sum, 3]"""
    idx = np.flatnonzero(count.reshape(-1))
    assert (key[idx] >= 0).all()
    idx = idx[np.argsort(key[idx])]
    idx = np.repeat(idx, count.reshape(-1)[idx])
    nx, ny, _ = S["dims"]
    return np.stack([idx % nx, (idx // nx) % ny, idx // (nx * ny)], 1)


def test_order_is_by_slot_place_and_edge_slot(one):
    """Counted apart from the restatement: the vertices per owner and the faces per cell.  Walking the owners (cells) in (slot, place)
    order, row r of the vertices must lie on an edge that leaves its owner -- inside the owner's unit cube -- and the three corners of
    face r inside its cell (a rounding of 1e-4 voxels allowed: the test is of the order, positions are pinned elsewhere)."""
    state, (v, c, f) = one
    key = BM.pool_keys(state)
    obs, inside = BM.corner_flags(state)
    nz, ny, nx = obs.shape
    nvert = np.zeros(obs.shape, np.int64)
    for code in FR.SLOT_CODE:
        dx, dy, dz = FR.corner_offset(code)
        a, b = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx)), (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        nvert[a] += obs[a] & obs[b] & (inside[a] != inside[b])
    live, bits = BM.live_cells(obs, inside)
    ntri = np.asarray([sum(len(FR.CASES[sum(((byte >> tet[m]) & 1) << m for m in range(4))]) for tet in FR.TET) for byte in range(256)])
    nface = np.where(live, ntri[bits], 0)
    assert nvert.sum() == V and nface.sum() == F
    owner, cell = _in_order_of_keys(key, nvert), _in_order_of_keys(key, nface)
    g = _lattice(state, v)
    assert (g >= owner - 1e-4).all() and (g <= owner + 1 + 1e-4).all()
    gf = g[f]
    assert (gf >= cell[:, None] - 1e-4).all() and (gf <= cell[:, None] + 1 + 1e-4).all()
    linear = (owner[:, 2] * ny + owner[:, 1]) * nx + owner[:, 0]
    assert (np.diff(linear) < 0).any()                                                            # and that is not the dense order


def test_live_cells_straddle_brick_faces_edges_and_corners(one):
    state, (_, _, f) = one
    live, bits = BM.live_cells(*BM.corner_flags(state))
    cut = live & (bits != 0) & (bits != 255)
    k, j, i = np.nonzero(cut)
    axes = ((i & 7) == 7).astype(int) + ((j & 7) == 7) + ((k & 7) == 7)
    got = [int((axes == a).sum()) for a in range(4)]
    print("cut live cells by the number of axes on which corner 0 sits at local 7:", got)
    assert got == [10176, 4181, 556, 23] and min(got) > 0 and sum(got) == int(cut.sum())


def test_two_calls_give_the_same_counts_in_another_slot_order(frames, one):
    state = _integrate(_integrate(BR.empty(S["dims"], 4096), frames[:2]), frames[2:])
    sb = state["slot_brick"][:state["count"]]
    assert state["count"] == 376 and (np.diff(sb) < 0).any()                                     # slot order is not brick order
    v, c, f = BM.extract(state, *ARGS)
    assert (len(v), len(f)) == (V, F)
    dv, dc, df = FR.extract_ref(*BR.to_dense(state), *ARGS)
    assert np.array_equal(sorted_rows(face_rows(v, c, f)), sorted_rows(face_rows(dv, dc, df)))
