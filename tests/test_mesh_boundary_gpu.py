"""sp3_mesh_boundary_* / sp3_mesh_fill_* on the device (csrc/mesh_boundary.hip; include/spann3r_hip.h "Mesh boundary loops and hole
filling") and what drives them: mesh.BoundaryLoops, mesh.boundary_loops, mesh.fill_holes and the fill_holes argument of the fusion
extractors.

The anchor is tests/mesh_boundary_ref.py (the numpy restatement, checked against a plain walk in tests/test_mesh_boundary_cpu.py).
Every comparison with it is exact: integer arrays equal in dtype and value, new positions bit for bit, colours equal.  The inputs
are the smallest that reach each failure mode: loop lengths around the powers of two of the doubling, alone and sharing the rounds
in one mesh; more loops than one scan chunk; one loop longer than 2^17 behind short ones; open chains beside loops; a 3-loop and a
4-loop in one mesh, so that the two scans of the fill disagree.  The brick scene of the topology tests has, by the restatements of
its extraction alone, 42 loops of 4 edges, 18 of 6 and 14 of 8 inside a rim that is an open chain: fill_holes = 12 has real holes
to close there."""
import sys

import numpy as np
import pytest
import torch

import bricks_ref as BR
import mesh_boundary_ref as B
import mesh_topology_ref as T
import raycast_ref as RC

pytestmark = pytest.mark.gpu

S = BR.SCENE


def _t(x):
    return torch.from_numpy(np.array(x)).cuda()


def _colors(nv):
    return (np.arange(4 * nv, dtype=np.uint32) * np.uint32(40503) >> 3).astype(np.uint8).reshape(-1, 4)


def _mesh(verts, faces, colors=True):
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    m = dict(vertices=_t(verts), faces=_t(np.asarray(faces, np.int32).reshape(-1, 3)), bounds=np.zeros((2, 3), np.float32), label="kept")
    if colors:
        m["colors"] = _t(_colors(len(verts)))
    return m


def _positions(nv, seed=1):
    return np.random.default_rng(seed).standard_normal((nv, 3)).astype(np.float32)


def _bits(x):
    return (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x, np.float32)).view(np.uint32)


def _assert_loops(loops, ref):
    got = {}
    for k in B.TABLES:
        x = getattr(loops, k)
        assert x.dtype == torch.int32 and x.is_cuda and x.is_contiguous(), k
        got[k] = x.cpu().numpy()
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    assert tuple(loops.report) == B.REPORT_KEYS and loops.report == ref["report"] and all(type(v) is int for v in loops.report.values())
    assert loops.n_boundary == ref["report"]["boundary"] and loops.n_loops == ref["report"]["loops"]
    assert loops.rounds == (B.rounds(loops.n_boundary) if loops.n_boundary else 0)
    return got


def _loops(verts, faces):
    from spann3r_amd import mesh as M
    return M.boundary_loops(_mesh(verts, faces))


def _assert_fill(verts, faces, n, colors=True, loops=None):
    """mesh.fill_holes against the restatement -> (the filled dict, the restatement's stats)"""
    from spann3r_amd import mesh as M
    m = _mesh(verts, faces, colors)
    m["normals"] = torch.zeros_like(m["vertices"])
    out = M.fill_holes(m, n, loops=loops)
    v, c, f, stats = B.fill_holes(verts, _colors(len(verts)) if colors else None, faces, n)
    assert out["vertices"].dtype == torch.float32 and out["faces"].dtype == torch.int32
    assert out["vertices"].shape == v.shape and np.array_equal(_bits(out["vertices"]), _bits(v))
    assert out["faces"].shape == f.shape and np.array_equal(out["faces"].cpu().numpy(), f)
    if colors:
        assert out["colors"].dtype == torch.uint8 and out["colors"].shape == c.shape and np.array_equal(out["colors"].cpu().numpy(), c)
    assert sorted(out) == sorted([k for k in m if k != "normals"] + ["fill"]) and out["label"] == "kept" and out["bounds"] is m["bounds"]
    assert tuple(out["fill"]) == B.FILL_KEYS and out["fill"] == stats
    # the caller's tensors are not written, and not handed back
    assert np.array_equal(_bits(m["vertices"]), _bits(verts)) and np.array_equal(m["faces"].cpu().numpy(), np.asarray(faces, np.int32))
    assert out["vertices"].data_ptr() != m["vertices"].data_ptr() and out["faces"].data_ptr() != m["faces"].data_ptr()
    return out, stats


# ------------------------------------------------------------------------------------------------ 1. every small case
SMALL = dict(T.SMALL, bowtie=B.BOWTIE)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_cases_equal_the_restatement(name):
    nv, faces = SMALL[name]
    ref = B.boundary_loops(faces, nv)
    _assert_loops(_loops(_positions(nv), faces), ref)
    mixed, _ = T.with_unusable(faces)
    got = _assert_loops(_loops(_positions(nv), mixed), B.boundary_loops(mixed, nv))
    for k in B.TABLES:                                                              # unusable faces change h and nothing else
        if k != "half_edge":
            assert np.array_equal(got[k], ref[k]), k


def test_the_small_cases_are_what_the_rule_says():
    r = {name: _loops(_positions(nv), f) for name, (nv, f) in SMALL.items()}
    assert r["triangle"].report == dict(boundary=3, loops=1, open=0, irregular_vertices=0, longest=3)
    assert r["triangle"].loop_first.tolist() == [0, 3] and r["triangle"].rank[r["triangle"].loop_members.long()].tolist() == [0, 1, 2]
    assert r["tetrahedron"].report == dict(boundary=0, loops=0, open=0, irregular_vertices=0, longest=0)
    assert r["tetrahedron"].loop_first.tolist() == [0] and r["tetrahedron"].loop_members.shape == (0,) and r["tetrahedron"].rounds == 0
    for name, b in (("three_on_an_edge", 6), ("pair_inconsistent", 4), ("bowtie", 6)):
        rep = r[name].report
        assert (rep["boundary"], rep["loops"], rep["open"], rep["longest"]) == (b, 0, b, 0) and rep["irregular_vertices"] > 0, name
        assert bool((r[name].loop == -1).all()) and bool((r[name].rank == -1).all()) and r[name].loop_first.tolist() == [0]
    assert r["pair_consistent"].report == dict(boundary=4, loops=1, open=0, irregular_vertices=0, longest=4)


# ------------------------------------------------------------------------------------------------ 2. around the powers of two
@pytest.mark.parametrize("n", B.FAN_SIZES)
def test_a_rim_around_a_power_of_two(n):
    verts, faces = T.closed_fan(n)
    ref = B.boundary_loops(faces, len(verts))
    assert ref["report"] == dict(boundary=n, loops=1, open=0, irregular_vertices=0, longest=n)
    _assert_loops(_loops(verts, faces), ref)


def test_loops_of_every_length_share_the_rounds():
    """2^k exceeds the length of the short loops while the long ones still grow: the wrap must keep the first place of the head"""
    verts, faces = B.all_fans()
    ref = B.boundary_loops(faces, len(verts))
    assert np.diff(ref["loop_first"]).tolist() == list(B.FAN_SIZES) and ref["report"]["boundary"] == sum(B.FAN_SIZES)
    loops = _loops(verts, faces)
    _assert_loops(loops, ref)
    assert loops.rounds == 11


def test_a_permuted_face_list_changes_only_the_half_edges():
    verts, faces = B.all_fans()
    perm = np.random.default_rng(3).permutation(len(faces))
    a = _assert_loops(_loops(verts, faces), B.boundary_loops(faces, len(verts)))
    b = _assert_loops(_loops(verts, faces[perm]), B.boundary_loops(faces[perm], len(verts)))
    for k in B.TABLES:
        assert np.array_equal(a[k], b[k]) == (k != "half_edge"), k
    assert np.array_equal(np.argsort(perm)[a["half_edge"] // 3] * 3 + a["half_edge"] % 3, b["half_edge"])


# ------------------------------------------------------------------------------------------------ 3. more loops than one scan chunk
def test_ninety_thousand_triangles_are_ninety_thousand_loops():
    verts, faces = B.triangles(90000)
    assert 3 * len(faces) == 270000 > 1024 * 256
    ref = B.boundary_loops(faces, len(verts))
    assert ref["report"] == dict(boundary=270000, loops=90000, open=0, irregular_vertices=0, longest=3)
    loops = _loops(verts, faces)
    _assert_loops(loops, ref)
    out, stats = _assert_fill(verts, faces, 3, loops=None)
    assert stats == dict(max_edges=3, loops=90000, filled=90000, vertices_added=0, faces_added=90000, open=0)
    assert np.array_equal(out["faces"][90000:].cpu().numpy(), faces[:, [1, 0, 2]])   # every triangle gets its own back, reversed


# ------------------------------------------------------------------------------------------------ 4. one loop longer than 2^17
def test_a_loop_of_two_hundred_thousand_behind_short_ones():
    verts, faces = B.cat([B.triangles(3), T.closed_fan(200000), B.triangles(2)])
    ref = B.boundary_loops(faces, len(verts))
    assert np.diff(ref["loop_first"]).tolist() == [3, 3, 3, 200000, 3, 3] and 200000 > 2 ** 17
    assert ref["loop_members"][9] == 9 and ref["rank"][9] == 0                       # the head of the long loop is not element 0
    loops = _loops(verts, faces)
    _assert_loops(loops, ref)
    assert loops.rounds == 18
    _, stats = _assert_fill(verts, faces, 3, loops=loops)
    assert (stats["filled"], stats["faces_added"], stats["vertices_added"]) == (5, 5, 0)


# ------------------------------------------------------------------------------------------------ 5. open chains beside loops
@pytest.mark.parametrize("bowtie", [False, True])
def test_the_punched_sheet(bowtie):
    from spann3r_amd import mesh as M
    verts, faces, holes, open_ = B.punched_sheet(33, bowtie)
    ref = B.boundary_loops(faces, len(verts))
    assert ref["report"] == dict(boundary=128 + 4 * holes + open_, loops=holes + 1, open=open_, irregular_vertices=1 if bowtie else 0,
                                 longest=128)
    m = _mesh(verts, faces)
    topo = M.topology(m)
    loops = M.boundary_loops(m, topo)
    _assert_loops(loops, ref)
    assert loops.topology is topo
    # max_edges = 4 closes every hole and leaves the rim (and the two holes of the bow-tie)
    out, stats = _assert_fill(verts, faces, 4, loops=loops)
    assert (stats["filled"], stats["vertices_added"], stats["faces_added"], stats["open"]) == (holes, holes, 4 * holes, open_)
    r = M.topology(out).report
    assert (r["boundary"], r["inconsistent"], r["nonmanifold"]) == (128 + open_, 0, 0)
    for n in (127, 128, 10 ** 6):
        out, stats = _assert_fill(verts, faces, n, colors=False, loops=loops)
        r = M.topology(out).report
        assert stats["filled"] == holes + (n >= 128) and (r["boundary"], r["inconsistent"], r["nonmanifold"]) == (open_ if n >= 128 else 128 + open_, 0, 0)
        if not bowtie and n >= 128:
            assert r["closed"] and r["euler"] == 2
    # nothing to fill: equal bits in new tensors
    same, stats = _assert_fill(verts, faces, 3, loops=loops)
    assert stats["filled"] == 0 and np.array_equal(_bits(same["vertices"]), _bits(verts)) and torch.equal(same["faces"], m["faces"])
    assert torch.equal(same["colors"], m["colors"])


# ------------------------------------------------------------------------------------------------ 6. the icosphere
def test_an_icosphere_with_faces_dropped_comes_back_closed():
    from spann3r_amd import mesh as M
    verts, faces = B.icosphere(2)
    drop = [0, 77, 150, 231, 319]
    kept = np.delete(faces, drop, 0)
    ref = B.boundary_loops(kept, len(verts))
    assert ref["report"] == dict(boundary=15, loops=5, open=0, irregular_vertices=0, longest=3)
    _assert_loops(_loops(verts, kept), ref)
    out, stats = _assert_fill(verts, kept, 3)
    r = M.topology(out).report
    assert r["closed"] and r["euler"] == 2 and r["inconsistent"] == 0 and stats["vertices_added"] == 0 and stats["faces_added"] == 5
    assert out["vertices"].shape[0] == len(verts)
    # a 4-loop among the 3-loops: the new vertex and the new faces are counted by two scans that disagree
    b = next(g for g in range(len(faces)) if g not in drop and g != 5 and len(set(faces[g]) & set(faces[5])) == 2 and
             not any(set(faces[g]) & set(faces[d]) for d in drop))
    kept2 = np.delete(faces, drop + [5, b], 0)
    ref2 = B.boundary_loops(kept2, len(verts))
    assert sorted(np.diff(ref2["loop_first"]).tolist()) == [3, 3, 3, 3, 3, 4] and np.diff(ref2["loop_first"]).tolist()[0] != 4
    _assert_loops(_loops(verts, kept2), ref2)
    for colors in (True, False):
        out, stats = _assert_fill(verts, kept2, 4, colors=colors)
        r = M.topology(out).report
        assert r["closed"] and r["euler"] == 2 and r["inconsistent"] == 0 and (stats["vertices_added"], stats["faces_added"]) == (1, 9)
    out, stats = _assert_fill(verts, kept2, 3)
    assert stats["filled"] == 5 and M.topology(out).report["boundary"] == 4


# ------------------------------------------------------------------------------------------------ 7. arguments, empty sizes
def test_arguments_are_checked_and_empty_sizes_launch_nothing():
    from spann3r_amd import lib as L, mesh as M
    verts, faces, _, _ = B.punched_sheet(9)
    m = _mesh(verts, faces)
    topo, loops = M.topology(m), M.boundary_loops(m)
    for bad in (2, 0, -1):
        with pytest.raises(ValueError, match="max_edges"):
            M.fill_holes(m, bad)
    other = _mesh(verts, faces[::-1])
    for fn in (lambda: M.boundary_loops(other, topo), lambda: M.fill_holes(other, 4, topology=topo), lambda: M.fill_holes(other, 4, loops=loops),
               lambda: M.fill_holes(_mesh(verts, faces[:-1]), 4, loops=loops)):
        with pytest.raises(ValueError, match="another mesh"):
            fn()
    with pytest.raises(TypeError):
        M.boundary_loops(m, dict())
    with pytest.raises(TypeError):
        M.fill_holes(m, 4, loops=dict())
    cloud = dict(m, faces=None)
    for fn in (M.boundary_loops, M.BoundaryLoops, lambda c: M.fill_holes(c, 4)):
        with pytest.raises(ValueError, match="point cloud"):
            fn(cloud)
    none = np.zeros((0, 3), np.int32)
    for nv, f in ((5, none), (0, none), (4, np.array([[0, 0, 1], [1, 2, 7]], np.int32))):
        e = _mesh(_positions(nv), f)
        lp = M.boundary_loops(e)
        _assert_loops(lp, B.boundary_loops(f, nv))
        out = M.fill_holes(e, 5)
        assert out["fill"] == dict(max_edges=5, loops=0, filled=0, vertices_added=0, faces_added=0, open=0)
        assert torch.equal(out["vertices"], e["vertices"]) and torch.equal(out["faces"], e["faces"]) and out["colors"].shape == (nv, 4)
    # the entry points refuse what the wrappers never pass
    lib = L.load()
    state = torch.zeros((8, 4), dtype=torch.int32, device="cuda")
    assert lib.sp3_mesh_boundary_rank(loops.next.data_ptr(), 8, state.data_ptr(), state.data_ptr(), L.stream_ptr()) == 1
    assert b"never reads what it writes" in lib.sp3_last_error()
    info = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert lib.sp3_mesh_fill_count(loops.loop_first.data_ptr(), loops.n_loops, 2, state.data_ptr(), state.data_ptr(), state.data_ptr(),
                                   info.data_ptr(), L.stream_ptr()) == 1 and b"max_edges" in lib.sp3_last_error()
    assert lib.sp3_mesh_boundary_rounds(1) == 1 and lib.sp3_mesh_boundary_rounds(256) == 8 and lib.sp3_mesh_boundary_rounds(257) == 9
    torch.cuda.synchronize()
    assert not bool(info.any()) and not bool(state.any())


# ------------------------------------------------------------------------------------------------ 8. the extractors
FILL = 12


@pytest.fixture(scope="module")
def volumes():
    from spann3r_amd import fusion as F_
    frs = RC.scene_frames()
    kw = dict(intrinsics=[f["K"] for f in frs], cam2world=[f["cam2world"] for f in frs], valid=[_t(f["valid"]) for f in frs],
              pts=[_t(f["pts"]) for f in frs], images=[_t(f["images"]) for f in frs])
    brick = F_.BrickTSDFVolume(S["origin"], S["voxel"], S["dims"], trunc=S["trunc"], band=S["band"])
    brick.integrate(**kw)
    dense = F_.TSDFVolume(S["origin"], S["voxel"], S["dims"], trunc=S["trunc"])
    dense.integrate(**kw)
    return dict(brick_direct=(brick, dict(direct=True)), brick_dense=(brick, dict(direct=False)), dense=(dense, dict()))


def _assert_same_mesh(a, b):
    for k in ("vertices", "colors", "faces"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    assert np.array_equal(_bits(a["vertices"]), _bits(b["vertices"])) and np.array_equal(a["bounds"], b["bounds"])


@pytest.mark.parametrize("route", ["brick_direct", "brick_dense", "dense"])
def test_fill_holes_in_the_extractors_is_the_composition(volumes, route):
    from spann3r_amd import mesh as M
    vol, kw = volumes[route]
    raw = vol.extract_mesh(**kw)
    zero = vol.extract_mesh(fill_holes=0, **kw)
    assert sorted(zero) == sorted(raw) == ["bounds", "colors", "faces", "vertices"]
    _assert_same_mesh(zero, raw)
    # the holes are real: the restatement finds loops of at most FILL edges in this surface, inside a longer boundary
    ref = B.boundary_loops(raw["faces"].cpu().numpy(), raw["vertices"].shape[0])
    lengths = np.diff(ref["loop_first"])
    assert (lengths <= FILL).sum() >= 10 and ref["report"]["boundary"] > int(lengths[lengths <= FILL].sum())
    _assert_loops(M.boundary_loops(raw), ref)
    got = vol.extract_mesh(fill_holes=FILL, **kw)
    want = M.fill_holes(raw, FILL)
    assert sorted(got) == ["bounds", "colors", "faces", "fill", "vertices"] and got["fill"] == want["fill"]
    assert got["fill"]["filled"] == int((lengths <= FILL).sum())
    _assert_same_mesh(got, want)
    v, c, f, stats = B.fill_holes(raw["vertices"].cpu().numpy(), raw["colors"].cpu().numpy(), raw["faces"].cpu().numpy(), FILL, loops=ref)
    assert got["fill"] == stats and np.array_equal(_bits(got["vertices"]), _bits(v)) and np.array_equal(got["faces"].cpu().numpy(), f)
    assert np.array_equal(got["colors"].cpu().numpy(), c)
    before, after = M.topology(raw).report, M.topology(got).report
    assert after["boundary"] == before["boundary"] - int(lengths[lengths <= FILL].sum()) < before["boundary"]
    assert after["inconsistent"] <= before["inconsistent"] and after["nonmanifold"] <= before["nonmanifold"]
    # the filter first, then the fans, then the smoothing, then the clustering
    cell = 2 * S["voxel"]
    origin = vol.to_dense().origin if route == "brick_dense" else vol.origin
    all4 = vol.extract_mesh(min_component_faces=9, simplify_cell=cell, smooth_iters=3, fill_holes=FILL, **kw)
    step = M.simplify(M.smooth(M.fill_holes(M.filter_components(raw, min_faces=9), FILL), 3), cell, origin=origin)
    assert all4["components"] == step["components"] and all4["simplify"] == step["simplify"] and all4["smooth"] == step["smooth"]
    assert all4["fill"] == step["fill"]
    _assert_same_mesh(all4, step)
    two = vol.extract_mesh(smooth_iters=3, fill_holes=FILL, **kw)
    _assert_same_mesh(two, M.smooth(want, 3))
    centres = slice(raw["vertices"].shape[0], None)
    assert not torch.equal(two["vertices"][centres], want["vertices"][centres])     # the centres are interior vertices: they move


def test_scale_follows_the_fill_and_the_drivers_pass_it_through(volumes):
    from spann3r_amd import fusion as F_, mesh as M
    vol, kw = volumes["brick_direct"]
    for bad in (1, 2, -3):
        with pytest.raises(ValueError, match="fill_holes"):
            vol.extract_mesh(fill_holes=bad, **kw)
    plain = vol.extract_mesh(fill_holes=FILL, **kw)
    scaled = vol.extract_mesh(fill_holes=FILL, scale=10.0, transform=np.diag([-1.0, -1.0, 1.0, 1.0]), **kw)
    assert torch.equal(scaled["faces"], plain["faces"]) and torch.equal(scaled["colors"], plain["colors"]) and scaled["fill"] == plain["fill"]
    assert torch.equal(scaled["vertices"], plain["vertices"] * 10.0 * torch.tensor([-1.0, -1.0, 1.0], device="cuda"))
    assert np.array_equal(scaled["bounds"], np.stack([scaled["vertices"].amin(0).cpu().numpy(), scaled["vertices"].amax(0).cpu().numpy()]))
    frs = RC.scene_frames()
    args = (torch.stack([_t(f["pts"]) for f in frs]), np.stack([f["K"] for f in frs]), np.stack([f["cam2world"] for f in frs]),
            torch.stack([_t(f["valid"]) for f in frs]).bool(), torch.stack([_t(f["images"]) for f in frs]))
    a = F_.fuse_pointmaps(*args, voxel_size=S["voxel"], bricks=True, direct_mesh=True, fill_holes=FILL)
    assert a["fill"]["max_edges"] == FILL
    _assert_same_mesh(a, M.fill_holes(F_.fuse_pointmaps(*args, voxel_size=S["voxel"], bricks=True, direct_mesh=True), FILL))
    d = F_.fuse_pointmaps(*args, voxel_size=S["voxel"], fill_holes=FILL)
    _assert_same_mesh(d, M.fill_holes(F_.fuse_pointmaps(*args, voxel_size=S["voxel"]), FILL))


# ------------------------------------------------------------------------------------------------ 9. the demo's arguments
@pytest.mark.parametrize("flag,word", [(["--fill_holes", "8"], "--fused"), (["--fused", "--fill_holes", "2"], "--fill_holes")])
def test_demo_loop_checks_the_flag(monkeypatch, capsys, flag, word):
    import demo_loop
    monkeypatch.setattr(sys, "argv", ["demo_loop.py", "--tiny"] + flag)
    with pytest.raises(SystemExit) as e:
        demo_loop.main()
    assert e.value.code == 2 and word in capsys.readouterr().err
