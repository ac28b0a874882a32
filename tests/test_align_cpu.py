"""Global alignment without a GPU: the restatement (tests/align_ref.py) against a scalar loop, against the reference's formula in float64
and by hand; the host half of the registration; Kruskal; the spanning-tree initialisation and 20 descent steps on a consistent
synthetic scene through the CPU restatement path; the host checks of both entry points."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import torch

import align_ref as R
from conftest import REPO
from spann3r_amd import align as A

# fp32 restatement chained through torch against the float64 statement on the three-image fixture: the measured relative difference
# max |g32 - g64| / max |g64| per parameter group, and the bar at 4x (the project's convention).  The GPU tests use the same bars.
MEASURED = dict(loss=4.21e-8, pw_poses=1.23e-7, pw_adaptors=1.90e-7, im_depthmaps=2.28e-7, im_poses=3.03e-8, im_focals=4.68e-7, im_pp=1.46e-7)
BARS = {k: 4 * v for k, v in MEASURED.items()}
GROUPS = ("pw_poses", "pw_adaptors", "im_depthmaps", "im_poses", "im_focals", "im_pp")


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


@functools.lru_cache(None)
def scene3_results():
    imgs, edges = R.scene3()
    return imgs, edges, R.loss_grad_ref(imgs, edges, keep_items=True)


def pairs_of(edges):
    """the pair_graph dict of a scene of align_ref (lists: the images differ in shape); conf = exp(W)"""
    t = torch.from_numpy
    return dict(view1=dict(idx=[e["ij"][0] for e in edges]), view2=dict(idx=[e["ij"][1] for e in edges]),
                pred1=dict(pts3d=[t(e["P"][0]) for e in edges], conf=[t(np.exp(e["W"][0])) for e in edges]),
                pred2=dict(pts3d_in_other_view=[t(e["P"][1]) for e in edges], conf=[t(np.exp(e["W"][1])) for e in edges]))


def parametrised_aligner(backend, device="cpu"):
    """the three-image fixture as a GlobalAligner with every parameter group live and off its default"""
    _, edges, _ = scene3_results()
    al = A.GlobalAligner(pairs_of(edges), backend=backend, allow_pw_adaptors=True, optimize_pp=True, seed=3, device=device)
    with torch.no_grad():
        al.pw_adaptors.copy_(torch.randn(al.n_edges, 2, generator=torch.Generator().manual_seed(1)) * 0.5)
        al.im_pp.copy_(torch.randn(al.n_imgs, 2, generator=torch.Generator().manual_seed(2)) * 0.1)
    return al


def f64_statement(al):
    """the reference's formula in float64 at the aligner's parameters -> (L, dict of gradients per group), float64"""
    p64 = {n: getattr(al, n).detach().double().cpu().requires_grad_(True) for n in GROUPS}
    params = dict(p64)
    params["im_depthmaps"] = [p64["im_depthmaps"][o:o + h * w].view(h, w) for o, (h, w) in zip(al.problem.offsets, al.imshapes)]
    pb = al.problem
    prob = dict(ij=al.edges, shapes=al.imshapes, P_i=[p.cpu().numpy() for p in pb.P[0]], P_j=[p.cpu().numpy() for p in pb.P[1]],
                W_i=[w.cpu().numpy() for w in pb.W[0]], W_j=[w.cpu().numpy() for w in pb.W[1]])
    L = R.loss_f64(params, prob, norm_pw_scale=al.norm_pw_scale, base_scale=al.base_scale, pw_break=al.pw_break, focal_break=al.focal_break)
    L.backward()
    return float(L.detach()), {n: p64[n].grad for n in GROUPS}


# ------------------------------------------------------------------------------------------------ 1. restatement against loops
def test_restatement_equals_the_scalar_loop():
    imgs, edges, ref = scene3_results()
    assert [im["depth"].shape for im in imgs] == [(13, 21), (24, 32), (24, 32)] and len(edges) == 6
    assert sum(int((e["W"][s] == 0).sum()) for e in edges for s in (0, 1)) > 100      # weights of exactly 0 are in the fixture
    lp = R.loss_grad_loop(imgs, edges)
    for a, b in zip(ref["gd"], lp["gd"]):
        assert a.dtype == np.float32 and np.array_equal(bits(a), bits(b))
    assert len(ref["items"]) == len(lp["items"]) == 12
    for a, b in zip(ref["items"], lp["items"]):
        assert (a["n"], a["e"], a["s"]) == (b["n"], b["e"], b["s"])
        for x, y in ((a["term"], b["term"]), (np.stack(a["g"]), b["g"]), (a["gd"], b["gd"])):
            assert x.dtype == np.float32 and np.array_equal(bits(x), bits(y))
    # the fp64 sums against plain left-to-right Python-float sums: n = the count of addends of each sum
    for key, cnt in (("img", ref["img_cnt"][:, None]), ("edge", ref["edge_cnt"][:, None]), ("S", ref["S_cnt"])):
        bound = R.sum_bound(cnt, ref[key + "_abs"])
        assert (ref[key + "_abs"] > 0).all() and (np.abs(ref[key] - lp[key]) <= bound).all(), key
    assert ref["img_cnt"].tolist() == [4 * 273, 4 * 768, 4 * 768] and ref["edge_cnt"].tolist() == [1041, 1041, 1041, 1536, 1041, 1536]
    assert abs(ref["L"] - lp["L"]) <= R.sum_bound(ref["S_cnt"], ref["S_abs"]) @ (1.0 / np.array(ref["A"])) + 4 * R.U53 * abs(ref["L"])


# ------------------------------------------------------------------------------------------------ 2. against the reference's formula
def test_restatement_chained_through_torch_equals_the_float64_statement():
    """Loss and gradient of every parameter group, fp32 restatement behind AlignLoss against float64 autograd of the reference's own
    formula (quaternion normalisation, signed_expm1, scale factor, adaptors, exp of log-depth).  Measured on this fixture, relative
    to the largest float64 gradient of the group: loss 4.21e-8, pw_poses 1.23e-7, pw_adaptors 1.90e-7, im_depthmaps 2.28e-7,
    im_poses 3.03e-8, im_focals 4.68e-7, im_pp 1.46e-7; the bars are 4x these."""
    al = parametrised_aligner(R.Backend())
    L = al()
    L.backward()
    L64, g64 = f64_statement(al)
    rel = abs(float(L.detach()) - L64) / abs(L64)
    print("loss", rel)
    assert rel <= BARS["loss"]
    for n in GROUPS:
        rel = float((getattr(al, n).grad.double() - g64[n]).abs().max() / g64[n].abs().max())
        print(n, rel)
        assert rel <= BARS[n], (n, rel)


# ------------------------------------------------------------------------------------------------ 3. by hand
def _pair_by_hand(shift):
    h, w = 8, 32                                         # 256 pixels: 1 / A is exact
    rng = np.random.default_rng(7)
    imgs, P = [], []
    for n in range(2):
        d = (1 + rng.integers(0, 2048, (h, w)) / 1024).astype(np.float32)      # multiples of 2^-10 in [1, 3): d + 1 is exact
        im = dict(depth=d, C=np.eye(4, dtype=np.float32)[:3].reshape(12), f=np.float32(30.5), cx=np.float32(w / 2), cy=np.float32(h / 2))
        px = R._pixel(im)
        imgs.append(im)
        P.append(np.stack((px["xc"], px["yc"], px["d"]), -1))
    M = np.eye(4, dtype=np.float32)[:3].copy()
    M[:, 3] = shift
    W = [np.ones((h, w), np.float32)] * 2
    return imgs, [dict(ij=(0, 1), P=P, W=W, M=M.reshape(12), a=np.ones(3, np.float32))]


def test_by_hand_zero_residual_and_unit_shift():
    ref = R.loss_grad_ref(*_pair_by_hand((0, 0, 0)))
    assert ref["L"] == 0.0 and (ref["S"] == 0).all() and (ref["img"] == 0).all() and (ref["edge"] == 0).all()      # the rho == 0 rule
    assert all((g == 0).all() for g in ref["gd"])
    ref = R.loss_grad_ref(*_pair_by_hand((0, 0, 1)))
    assert ref["S"].tolist() == [256.0, 256.0] and ref["A"] == [256.0, 256.0] and ref["L"] == 2.0      # each side: S / A == 1 exactly
    assert (ref["edge"][0, 11] == 2.0) and ref["img"][:, 11].tolist() == [-1.0, -1.0]                      # dL/dM_23 = -g_2 = 1 per side


# ------------------------------------------------------------------------------------------------ 4. the host half of the registration
def test_umeyama_recovers_a_known_similarity():
    rng = np.random.default_rng(11)
    for reflect in (False, True):
        p = rng.standard_normal((500, 3)).astype(np.float32)
        Rm, s, T = R._rot(rng, 0.9), 1.7, np.array([0.3, -1.2, 2.0])
        q = (s * p.astype(np.float64) @ Rm.T + T)
        if reflect:                                       # a mirrored, noisy target: the best ROTATION is asked for
            q = q * np.array([1, 1, -1.0]) + rng.standard_normal(q.shape) * 0.01
        q = q.astype(np.float32)
        w = rng.uniform(0.1, 2.0, 500).astype(np.float32)
        m, _ = R.moments_ref(p, q, w)
        s1, R1, T1 = A.umeyama_from_moments(m)
        s2, R2, T2 = R.umeyama_f64(p, q, w)
        assert abs(np.linalg.det(R1) - 1) < 1e-12 and np.abs(R1 @ R1.T - np.eye(3)).max() < 1e-12      # a rotation, also when mirrored
        assert abs(s1 - s2) < 1e-9 * s2 and np.abs(R1 - R2).max() < 1e-9 and np.abs(T1 - T2).max() < 1e-9      # its own fp64 statement
        if not reflect:                                   # exact correspondences (to fp32 rounding of q)
            assert abs(s1 - s) < 1e-6 and np.abs(R1 - Rm).max() < 1e-6 and np.abs(T1 - T).max() < 1e-6


def test_quaternion_round_trip():
    rng = np.random.default_rng(2)
    for ang in (0.0, 0.3, 2.0, 3.1, np.pi):
        Rm = R._rot(rng, ang)
        back = A.quat_to_rotmat(torch.from_numpy(A.rotmat_to_quat(Rm))).numpy()
        assert np.abs(back - Rm).max() < 1e-12


# ------------------------------------------------------------------------------------------------ 5. Kruskal
def test_kruskal_against_scipy():
    import scipy.sparse as sp
    from scipy.sparse.csgraph import minimum_spanning_tree
    rng = np.random.default_rng(3)
    for n in (2, 5, 9):
        ij = [(i, j) for i in range(n) for j in range(n) if i != j]
        scores = rng.permutation(len(ij)) + 1.0           # distinct
        g = sp.dok_array((n, n))
        for (i, j), s in zip(ij, scores):
            g[i, j] = -s
        want = minimum_spanning_tree(g.tocsr()).tocoo()
        tree = A.maximum_spanning_tree(n, ij, scores)
        assert len(tree) == n - 1
        assert {frozenset(ij[e]) for e in tree} == {frozenset((int(a), int(b))) for a, b in zip(want.row, want.col)}
        assert abs(sum(scores[e] for e in tree) + want.data.sum()) < 1e-9
    assert A.maximum_spanning_tree(3, [(0, 1), (1, 0), (1, 2), (2, 1)], [1.0, 1.0, 1.0, 1.0]) == [0, 2]      # ties: the lower edge index


# ------------------------------------------------------------------------------------------------ 6. a consistent synthetic scene
# measured on the restatement path: init loss / scene extent 1.89e-7; after the best similarity the camera centres differ by 3.1e-8
# and the rotations by 4.0e-8; the bars are 4x these.
SHEET_MEASURED = dict(loss_rel=1.90e-7, centre=3.13e-8, rot=4.05e-8)


@functools.lru_cache(None)
def sheet_cpu():
    sc = R.sheet_scene()
    al = A.GlobalAligner(sc["pairs"], backend=R.Backend())
    tree = al.init_minimum_spanning_tree()
    with torch.no_grad():
        L0 = float(al())
        pts = torch.cat([p.reshape(-1, 3) for p in al.get_pts3d()])
        extent = float((pts.max(0).values - pts.min(0).values).norm())
        poses = al.get_im_poses().double().numpy()
    state = {k: v.detach().clone() for k, v in al.state_dict().items()}
    return sc, al, tree, L0, extent, poses, state


def perturb(al, amount=0.02, seed=5):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in (al.pw_poses, al.im_poses, al.im_depthmaps, al.im_focals):
            p.add_((torch.randn(p.shape, generator=g) * amount).to(p.device))


def test_mst_init_explains_a_consistent_scene_and_descent_lowers_the_loss():
    sc, al, tree, L0, extent, poses, state = sheet_cpu()
    assert len(tree) == 3 and len({n for e in tree for n in al.edges[e]}) == 4
    print("init loss / extent", L0 / extent)
    assert L0 / extent <= 4 * SHEET_MEASURED["loss_rel"]
    s, dc, dr = R.similarity_between(poses, sc["c2w"])
    print("similarity scale", s, "centres", dc, "rotations", dr)
    assert dc <= 4 * SHEET_MEASURED["centre"] and dr <= 4 * SHEET_MEASURED["rot"]
    assert np.allclose(al.get_focals().detach().flatten().numpy(), sc["focal"], rtol=1e-5)
    assert all((d > 0).all() for d in al.get_depthmaps())
    al.load_state_dict(state)
    perturb(al)
    last = al.compute_global_alignment(init=None, niter=20)
    assert len(al.losses) == 20 and last == al.losses[-1]
    assert all(b < a for a, b in zip(al.losses, al.losses[1:])), al.losses      # strictly lower, every iteration
    al.load_state_dict(state)


# init="known_poses" on the same scene through the restatement path, measured: loss / scene extent 3.00e-7; the pairwise scales against
# 1 / (the scale the scene gave the edge) 1.54e-7; the depth maps against the true ones 2.68e-7 (relative); the bars are 4x these.
KNOWN_POSES_MEASURED = (3.00e-7, 1.54e-7, 2.68e-7)


def known_poses_figures(al, sc):
    """-> (loss / extent, largest relative error of the pairwise scales, of the depths) of an aligner on the sheet scene"""
    with torch.no_grad():
        L0 = float(al())
        pts = torch.cat([p.reshape(-1, 3) for p in al.get_pts3d()])
        extent = float((pts.max(0).values - pts.min(0).values).norm())
        scales = al.get_pw_scale().double().cpu().numpy()
        depths = [d.double().cpu().numpy() for d in al.get_depthmaps()]
    return L0 / extent, float(np.abs(scales * sc["scales"] - 1).max()), max(float(np.abs(a / b - 1).max()) for a, b in zip(depths, sc["depth"]))


def test_known_poses_init_explains_a_consistent_scene():
    """every pose and focal preset to the truth: the pairwise poses, scales and depth maps init="known_poses" sets leave a loss at
    rounding level, and are the true ones"""
    sc = R.sheet_scene()
    al = A.GlobalAligner(sc["pairs"], backend=R.Backend())
    al.preset_focal([sc["focal"]] * 4)
    al.preset_pose([torch.from_numpy(p) for p in sc["c2w"]])
    al.init_from_known_poses()
    rel = known_poses_figures(al, sc)
    print("loss / extent %.3g, pairwise scales %.3g, depths %.3g" % rel)
    assert all(r <= 4 * m for r, m in zip(rel, KNOWN_POSES_MEASURED))
    pw = al.get_pw_poses().detach().double().numpy()
    for e, (i, j) in enumerate(al.edges):               # M_e = s_e [R_i | t_i]
        assert np.abs(pw[e, :3, :3] / np.cbrt(np.linalg.det(pw[e, :3, :3])) - sc["c2w"][i][:3, :3]).max() < 1e-6


def test_presets_and_argument_errors():
    import pytest
    sc = R.sheet_scene()
    al = A.GlobalAligner(sc["pairs"], backend=R.Backend())
    al.preset_focal([sc["focal"]] * 4)
    al.preset_pose([torch.from_numpy(p) for p in sc["c2w"]])
    assert not al.im_focals.requires_grad and not al.im_poses.requires_grad and al.norm_pw_scale is False
    assert np.abs(al.get_im_poses().double().numpy() - sc["c2w"]).max() < 1e-6
    assert np.allclose(al.get_focals().flatten().numpy(), sc["focal"], rtol=1e-6)
    al.preset_principal_point([(17.0, 11.0)] * 4)
    assert not al.im_pp.requires_grad and np.allclose(al.get_principal_points().numpy(), (17.0, 11.0))
    L = al()
    L.backward()
    assert al.im_poses.grad is None and al.im_focals.grad is None and al.im_pp.grad is None and al.pw_poses.grad is not None
    with pytest.raises(ValueError):
        al.preset_focal([30.0], msk=[0])                 # incomplete mask
    with pytest.raises(ValueError):
        al.compute_global_alignment(init="nope")
    with pytest.raises(ValueError):
        al.compute_global_alignment(schedule="step")
    empty = dict(view1=dict(idx=[]), view2=dict(idx=[]), pred1=dict(pts3d=[], conf=[]), pred2=dict(pts3d_in_other_view=[], conf=[]))
    with pytest.raises(ValueError):
        A.GlobalAligner(empty, backend=R.Backend())      # E = 0
    gap = dict(sc["pairs"], view1=dict(idx=[i + 1 for i in sc["pairs"]["view1"]["idx"]]), view2=dict(idx=[j + 1 for j in sc["pairs"]["view2"]["idx"]]))
    with pytest.raises(ValueError):
        A.GlobalAligner(gap, backend=R.Backend())
    with pytest.raises(ValueError):
        A.GlobalAligner(sc["pairs"], conf="cube", backend=R.Backend())
    with pytest.raises(RuntimeError):
        A.GlobalAligner(sc["pairs"], device="cpu")()     # no backend: the device kernels, and no CPU path


def test_schedules():
    assert A.cosine_schedule(0.0, 0.01, 1e-6) == 0.01 and abs(A.cosine_schedule(1.0, 0.01, 1e-6) - 1e-6) < 1e-18
    assert abs(A.cosine_schedule(0.5, 0.01, 1e-6) - (0.01 + 1e-6) / 2) < 1e-12 and A.linear_schedule(0.25, 1.0, 0.0) == 0.75


# ------------------------------------------------------------------------------------------------ the C boundary, without a GPU
def test_descriptors_match_the_header():
    """sizeof / offsetof of the three descriptors, as gcc sees include/spann3r_hip.h, equal the ctypes mirrors and the numpy records"""
    from spann3r_amd import lib
    lines = ['#include "%s"' % os.path.join(REPO, "include", "spann3r_hip.h"), "#include <stdio.h>", "#include <stddef.h>", "int main(){"]
    exp = []
    for cname, cls, dt in (("sp3_align_image", lib.AlignImage, A._IMG_DT), ("sp3_align_edge", lib.AlignEdge, A._EDGE_DT),
                           ("sp3_align_triple", lib.AlignTriple, A._TRIPLE_DT)):
        fields = [f[0] for f in cls._fields_]
        assert list(dt.names) == fields and dt.itemsize == ctypes.sizeof(cls)
        assert [dt.fields[f][1] for f in fields] == [getattr(cls, f).offset for f in fields]
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        lines += ['printf("%%zu\\n", offsetof(%s, %s));' % (cname, f) for f in fields]
        exp += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(c, "w").write("\n".join(lines) + "\n")
        subprocess.check_call(["gcc", c, "-o", exe])
        vals = [int(x) for x in subprocess.check_output([exe]).split()]
    assert vals == exp


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """the host checks of sp3_align_loss_grad / sp3_align_moments.  The pointers are never followed on the host, and every call here
    passes null device tables, which the entry points check last: nothing can launch, whatever else a check lets through."""
    import __graft_entry__ as g
    from spann3r_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        g.build()
    l = lib.load()
    i32 = ctypes.c_int32

    def tables():      # two images, two edges (0, 1) and (1, 0)
        imgs, edges = (lib.AlignImage * 2)(), (lib.AlignEdge * 2)()
        for n in range(2):
            imgs[n].depth, imgs[n].grad_depth = 0x1000 * (n + 1), 0x100000 * (n + 1)
            imgs[n].row_stride, imgs[n].w, imgs[n].h, imgs[n].f = 8, 8, 4, 8.0
        for e in range(2):
            for s in range(2):
                edges[e].pts[s], edges[e].weight[s], edges[e].row_stride[s] = 0x2000 * (2 * e + s + 1), 0x4000 * (2 * e + s + 1), 8
            edges[e].img[0], edges[e].img[1] = e, 1 - e
        first, edge, side = A.make_items(2, [(0, 1), (1, 0)])
        return imgs, edges, (i32 * 3)(*first), (i32 * 4)(*edge), (i32 * 4)(*side)

    def call(imgs, edges, first, edge, side, N=2, E=2, ws=0x100, out=0x200):
        return l.sp3_align_loss_grad(imgs, None, N, edges, None, E, first, edge, side, None, None, None, ws, out, out, out, None)

    def refused(match, *a, **k):
        assert call(*a, **k) != 0
        assert match in l.sp3_last_error(), l.sp3_last_error()

    refused(b"null device copy", *tables())                                                      # all else in order
    t = tables(); t[3][1] = 2; refused(b"edge index 2 outside", *t)
    t = tables(); t[3][0] = -1; refused(b"edge index -1 outside", *t)
    t = tables(); t[4][2] = 2; refused(b"neither 0 nor 1", *t)
    t = tables(); t[3][1], t[4][1] = 0, 0; refused(b"listed twice", *t)
    t = tables(); t[4][0], t[4][1] = 1, 0; refused(b"belongs to image", *t)                        # an item under the wrong image
    t = tables(); t[2][2] = 3; refused(b"item_first must run", *t)                                 # does not cover the 2 E items
    t = tables(); t[2][1] = 5; refused(b"item_first decreases", *t)
    t = tables(); t[0][1].f = 0.0; refused(b"f == 0", *t)
    t = tables(); t[1][0].img[1] = 2; refused(b"image index 2 outside", *t)
    t = tables(); t[1][1].row_stride[0] = 7; refused(b"row_stride", *t)
    t = tables(); t[0][0].w = 9; refused(b"bad geometry", *t)
    t = tables(); t[0][0].depth = None; refused(b"null depth", *t)
    t = tables(); t[1][0].weight[1] = None; refused(b"null pts / weight", *t)
    refused(b"N 4097", *tables(), N=4097)
    refused(b"N 0", *tables(), N=0)
    refused(b"E 65537", *tables(), E=65537)
    refused(b"E 0", *tables(), E=0)
    t = tables()
    for n in range(2):
        t[0][n].w = t[0][n].row_stride = t[0][n].h = 4800                                          # 300 x 300 blocks
    for e in range(2):
        t[1][e].row_stride[0] = t[1][e].row_stride[1] = 4800
    refused(b"T 90000", *t)
    refused(b"null ws / output", *tables(), ws=None)
    assert l.sp3_align_loss_grad(None, None, 2, None, None, 2, None, None, None, None, None, None, None, None, None, None, None) != 0
    assert b"null table" in l.sp3_last_error()
    assert l.sp3_align_loss_grad_ws_bytes(2, 2, 8, 4) == 8 * (2 * 17 + 2 * 30) and l.sp3_align_loss_grad_ws_bytes(0, 2, 8, 4) == 0
    assert l.sp3_align_loss_grad_ws_bytes(3, 6, 32, 24) == 8 * 4 * (3 * 17 + 6 * 30)

    def triples(B=2):
        tr = (lib.AlignTriple * B)()
        for b in range(B):
            tr[b].src, tr[b].dst, tr[b].w, tr[b].n = 0x1000 * (b + 1), 0x8000 * (b + 1), 0x10000 * (b + 1), 100 + b
        return tr

    def mrefused(match, tr, B=2, ws=0x100, out=0x200):
        assert l.sp3_align_moments(tr, None, B, ws, out, None) != 0
        assert match in l.sp3_last_error(), l.sp3_last_error()

    mrefused(b"null device copy", triples())
    mrefused(b"B 0", triples(), B=0)
    mrefused(b"B 65536", triples(), B=65536)
    mrefused(b"null table", None)
    tr = triples(); tr[1].dst = None; mrefused(b"triple 1: null pointer", tr)
    tr = triples(); tr[0].n = 0; mrefused(b"triple 0: n = 0", tr)
    tr = triples(); tr[1].n = 2 ** 31; mrefused(b"out of range", tr)
    mrefused(b"null ws / output", triples(), out=None)
    assert l.sp3_align_moments_ws_bytes(2, 101) == 2 * 17 * 8 and l.sp3_align_moments_ws_bytes(3, 10 ** 7) == 3 * 1024 * 17 * 8
