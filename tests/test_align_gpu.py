"""spann3r_amd.align on the device against the numpy restatement of the header's rule (tests/align_ref.py).

dL/dd is fp32 with every operation specified: it is compared bit for bit (NaNs by position: the payload of a generated NaN is not
part of the rule).  The fp64 sums run in another order than numpy's: they are held to the bound of a reordered fp64 sum,
n * 2^-53 * sum |addend| with n the count of addends.  Gradients through torch and the float64 statement use the bars measured in
tests/test_align_cpu.py.  The shapes are the smallest at which the tiling can go wrong: 13 x 21 next to 24 x 32 (neither a multiple of
the 16 x 16 block), 1 x 1, an image inside a wider buffer, 40 x 72 (blocks in both directions).

Parity with dust3r.cloud_opt is not tested: it cannot be imported here (spann3r_amd/align.py)."""
import ctypes

import numpy as np
import pytest
import torch

import align_ref as R
import test_align_cpu as TC
from spann3r_amd import align as A

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def run_device(imgs, edges, items=None, pad=0):
    """the raw entry point on the restatement's dicts.  pad > 0: every map lives in a buffer pad columns wider than the image, the
    padding of the inputs poisoned with NaN; the depth-gradient buffers are prefilled with SENTINEL and their padding must come back
    untouched -> dict(gd: list of [h, w], img [N, 15], edge [E, 15], S [2], L)"""
    from spann3r_amd import lib
    N, E = len(imgs), len(edges)
    first, iedge, iside = items if items is not None else R.make_items(N, [ed["ij"] for ed in edges])
    keep = []

    def up(a, tail=()):
        a = np.asarray(a, np.float32)
        h, w = a.shape[:2]
        buf = np.full((h, w + pad) + tail, np.nan, np.float32)
        buf[:, :w] = a
        t = torch.from_numpy(buf).cuda()
        keep.append(t)
        return t
    ti, te = np.zeros(N, A._IMG_DT), np.zeros(E, A._EDGE_DT)
    grads = []
    for n, im in enumerate(imgs):
        h, w = im["depth"].shape
        g = torch.full((h, w + pad), SENTINEL, device="cuda")
        grads.append(g)
        ti[n] = (up(im["depth"]).data_ptr(), g.data_ptr(), w + pad, w, h, im["f"], im["cx"], im["cy"], np.asarray(im["C"], np.float32))
    for e, ed in enumerate(edges):
        for s in (0, 1):
            te[e]["pts"][s], te[e]["weight"][s] = up(ed["P"][s], (3,)).data_ptr(), up(ed["W"][s]).data_ptr()
            te[e]["row_stride"][s], te[e]["img"][s] = ed["P"][s].shape[1] + pad, ed["ij"][s]
        te[e]["M"], te[e]["a"] = ed["M"], ed["a"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    ti_d, te_d, it_d = dev(ti), dev(te), [torch.from_numpy(x.copy()).cuda() for x in (first, iedge, iside)]
    l = lib.load()
    hmax, wmax = max(im["depth"].shape[0] for im in imgs), max(im["depth"].shape[1] for im in imgs)
    nws = l.sp3_align_loss_grad_ws_bytes(N, E, wmax, hmax) // 8
    ws = torch.full((nws + 16,), float("nan"), dtype=torch.float64, device="cuda")      # (a guard behind it: nothing is written outside)
    out_i = torch.full((N, 15), SENTINEL, dtype=torch.float64, device="cuda")
    out_e = torch.full((E, 15), SENTINEL, dtype=torch.float64, device="cuda")
    out_l = torch.full((3,), SENTINEL, dtype=torch.float64, device="cuda")
    i32p = ctypes.POINTER(ctypes.c_int32)
    first, iedge, iside = (np.ascontiguousarray(x, np.int32) for x in (first, iedge, iside))
    lib.check(l.sp3_align_loss_grad(ctypes.cast(ti.ctypes.data, ctypes.POINTER(lib.AlignImage)), ti_d.data_ptr(), N,
                                    ctypes.cast(te.ctypes.data, ctypes.POINTER(lib.AlignEdge)), te_d.data_ptr(), E, first.ctypes.data_as(i32p),
                                    iedge.ctypes.data_as(i32p), iside.ctypes.data_as(i32p), it_d[0].data_ptr(), it_d[1].data_ptr(), it_d[2].data_ptr(),
                                    ws.data_ptr(), out_i.data_ptr(), out_e.data_ptr(), out_l.data_ptr(), lib.stream_ptr()), "sp3_align_loss_grad")
    torch.cuda.synchronize()
    assert torch.isnan(ws[nws:]).all()
    gd = []
    for g, im in zip(grads, imgs):
        w = im["depth"].shape[1]
        assert (g[:, w:] == SENTINEL).all()              # nothing written outside the image
        gd.append(g[:, :w].cpu().numpy())
    l3 = out_l.cpu().numpy()
    return dict(gd=gd, img=out_i.cpu().numpy(), edge=out_e.cpu().numpy(), S=l3[:2], L=float(l3[2]))


def same_bits(a, b):
    """fp32 arrays: NaNs in the same places, every other element bit for bit"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def assert_matches(got, ref):
    for a, b in zip(got["gd"], ref["gd"]):
        assert same_bits(a, b)
    worst = 0.0
    for key, cnt in (("img", ref["img_cnt"][:, None]), ("edge", ref["edge_cnt"][:, None]), ("S", ref["S_cnt"])):
        bound = R.sum_bound(cnt, ref[key + "_abs"])
        nan = np.isnan(ref[key])
        assert np.array_equal(np.isnan(got[key]), nan), key
        d = np.abs(got[key] - ref[key])[~nan]
        b = np.broadcast_to(bound, ref[key].shape)[~nan]
        assert (d <= b).all(), (key, d.max())
        worst = max(worst, float((d[b > 0] / b[b > 0]).max(initial=0.0)))
    if np.isnan(ref["L"]):
        assert np.isnan(got["L"])
    else:
        assert abs(got["L"] - ref["L"]) <= R.sum_bound(ref["S_cnt"], ref["S_abs"]) @ (1.0 / np.array(ref["A"])) + 4 * R.U53 * abs(ref["L"])
    print("largest |difference| / bound of the fp64 sums: %.3g" % worst)


def scene_of_aligner(al):
    """the geometric parameters of an aligner as the restatement's dicts"""
    with torch.no_grad():
        depth, C, f, pp, M, a = (x.detach().cpu().numpy() for x in al.geometric_parameters())
    pb, imgs, edges = al.problem, [], []
    for n, (h, w) in enumerate(pb.shapes):
        imgs.append(dict(depth=depth[pb.offsets[n]:pb.offsets[n] + h * w].reshape(h, w), C=C[n], f=f[n], cx=pp[n, 0], cy=pp[n, 1]))
    for e, pair in enumerate(pb.ij):
        edges.append(dict(ij=pair, P=[pb.P[s][e].cpu().numpy() for s in (0, 1)], W=[pb.W[s][e].cpu().numpy() for s in (0, 1)], M=M[e], a=a[e]))
    return imgs, edges


# ------------------------------------------------------------------------------------------------ against the restatement
def test_three_image_scene_bits_bounds_and_determinism():
    imgs, edges, ref = TC.scene3_results()
    got = run_device(imgs, edges)
    assert_matches(got, ref)
    again = run_device(imgs, edges)
    for k in ("img", "edge", "S"):
        assert np.array_equal(got[k].view(np.uint64), again[k].view(np.uint64))
    assert got["L"] == again["L"] and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got["gd"], again["gd"]))


def test_four_camera_scene():
    _, al, _, _, _, _, state = TC.sheet_cpu()
    al.load_state_dict(state)
    TC.perturb(al)
    try:
        imgs, edges = scene_of_aligner(al)
    finally:
        al.load_state_dict(state)
    assert_matches(run_device(imgs, edges), R.loss_grad_ref(imgs, edges))


@pytest.mark.parametrize("shapes,ij", [
    (((13, 21), (24, 32), (24, 32)), None),                        # mixed shapes in one table, inside wider buffers
    (((1, 1), (1, 1), (5, 7)), None),                              # 1 x 1 images
    (((13, 21), (24, 32), (9, 40)), [(0, 1), (0, 2)]),             # images 1 and 2 occur only on side 1; not symmetrised
    (((17, 5), (3, 33)), [(0, 1)]),                                # E = 1, N = 2
    (((40, 72), (13, 21)), [(0, 1), (1, 0), (0, 1)]),              # 3 x 5 blocks: the sums cross workgroup partials; a repeated pair
])
def test_shapes_strides_and_structures(shapes, ij):
    imgs, edges = R.scene3(seed=len(shapes) + shapes[0][0], shapes=shapes, ij=ij)
    ref = R.loss_grad_ref(imgs, edges)
    assert_matches(run_device(imgs, edges, pad=5), ref)            # row_stride > w, poisoned padding, prefilled outputs
    assert_matches(run_device(imgs, edges), ref)


def test_item_order_is_the_tables():
    """the CSR decides the order of the fp32 depth-gradient sum: the items of every image reversed"""
    imgs, edges, _ = TC.scene3_results()
    first, iedge, iside = R.make_items(3, [e["ij"] for e in edges])
    for n in range(3):
        iedge[first[n]:first[n + 1]] = iedge[first[n]:first[n + 1]][::-1].copy()
        iside[first[n]:first[n + 1]] = iside[first[n]:first[n + 1]][::-1].copy()
    items = (first, iedge, iside)
    assert_matches(run_device(imgs, edges, items=items), R.loss_grad_ref(imgs, edges, items=items))


def test_special_values():
    # rho == 0 at every pixel: exact zeros; a unit shift: S / A == 1 exactly on each side
    got = run_device(*TC._pair_by_hand((0, 0, 0)))
    assert got["L"] == 0.0 and (got["S"] == 0).all() and (got["img"] == 0).all() and (got["edge"] == 0).all()
    assert all((g == 0).all() for g in got["gd"])
    got = run_device(*TC._pair_by_hand((0, 0, 1)))
    assert got["S"].tolist() == [256.0, 256.0] and got["L"] == 2.0 and got["edge"][0, 11] == 2.0 and got["img"][:, 11].tolist() == [-1.0, -1.0]
    # weights of exactly 0 (conf == 1 under "log") are in the three-image fixture; here also one pixel with rho == 0 among others
    imgs, edges = R.scene3(seed=21)
    edges[2]["M"] = np.eye(4, dtype=np.float32)[:3].reshape(12)      # edge (1, 0): side 0 lives in image 1
    edges[2]["a"] = np.ones(3, np.float32)
    imgs[1]["C"] = np.eye(4, dtype=np.float32)[:3].reshape(12)
    px = R._pixel(imgs[1])
    edges[2]["P"][0][5, 7] = (px["xc"][5, 7], px["yc"][5, 7], px["d"][5, 7])
    ref = R.loss_grad_ref(imgs, edges, keep_items=True)
    it = [i for i in ref["items"] if (i["e"], i["s"]) == (2, 0)][0]
    assert it["term"][5, 7] == 0 and all(g[5, 7] == 0 for g in it["g"]) and sum(int((e["W"][s] == 0).sum()) for e in edges for s in (0, 1)) > 100
    assert_matches(run_device(imgs, edges), ref)
    # a NaN in one P: the restatement's NaN set and nothing else
    imgs, edges = R.scene3(seed=22)
    edges[3]["P"][1][11, 13, 1] = np.nan                              # edge (1, 2), side 1: image 2
    ref = R.loss_grad_ref(imgs, edges)
    assert np.isnan(ref["gd"][2][11, 13]) and np.isnan(ref["gd"][2]).sum() == 1 and not np.isnan(ref["gd"][0]).any()
    assert np.isnan(ref["img"][2]).any() and not np.isnan(ref["img"][:2]).any() and np.isnan(ref["edge"][3]).any() and np.isnan(ref["S"][1])
    assert not np.isnan(ref["S"][0]) and np.isnan(ref["L"])
    assert_matches(run_device(imgs, edges), ref)


# ------------------------------------------------------------------------------------------------ through torch
def test_autograd_of_all_six_groups_and_the_float64_statement():
    """AlignLoss under torch.autograd on the device: .grad of the six parameter groups against the restatement chained through torch
    and against the float64 statement, both within the bars measured in tests/test_align_cpu.py"""
    dev, cpu = TC.parametrised_aligner(None, "cuda"), TC.parametrised_aligner(R.Backend())
    for n in TC.GROUPS:
        assert torch.equal(getattr(dev, n).detach().cpu(), getattr(cpu, n).detach())
    Ld, Lc = dev(), cpu()
    Ld.backward()
    Lc.backward()
    L64, g64 = TC.f64_statement(dev)
    print("loss", float(Ld.detach()), float(Lc.detach()), L64)
    assert abs(float(Ld.detach()) - float(Lc.detach())) <= TC.BARS["loss"] * abs(L64) and abs(float(Ld.detach()) - L64) <= TC.BARS["loss"] * abs(L64)
    for n in TC.GROUPS:
        gd_, gc_ = getattr(dev, n).grad.double().cpu(), getattr(cpu, n).grad.double()
        scale = float(g64[n].abs().max())
        print(n, float((gd_ - gc_).abs().max()) / scale, float((gd_ - g64[n]).abs().max()) / scale)
        assert float((gd_ - gc_).abs().max()) <= TC.BARS[n] * scale and float((gd_ - g64[n]).abs().max()) <= TC.BARS[n] * scale


def test_presets_freeze_what_they_should():
    sc = R.sheet_scene()
    al = A.GlobalAligner(sc["pairs"])
    assert al.device.type == "cuda" and al.norm_pw_scale is True
    al.preset_focal([sc["focal"]] * 4)
    before = al.im_focals.detach().clone()
    al.preset_pose([torch.from_numpy(p) for p in sc["c2w"]])
    assert not al.im_focals.requires_grad and not al.im_poses.requires_grad and al.norm_pw_scale is False
    L = al()
    L.backward()
    assert al.im_poses.grad is None and al.im_focals.grad is None and al.im_pp.grad is None
    assert al.pw_poses.grad is not None and al.im_depthmaps.grad is not None and torch.isfinite(al.pw_poses.grad).all()
    L64, _ = TC.f64_statement(al)
    assert abs(float(L.detach()) - L64) <= TC.BARS["loss"] * abs(L64)      # also with norm_pw_scale off
    al.init_from_known_poses()       # the start it gives explains the scene: the bars of the CPU test (here 5.3e-7, 2.9e-7, 4.8e-7)
    rel = TC.known_poses_figures(al, sc)
    print("init='known_poses' on the device: loss / extent %.3g, pairwise scales %.3g, depths %.3g" % rel)
    assert all(r <= 4 * m for r, m in zip(rel, TC.KNOWN_POSES_MEASURED))
    al.compute_global_alignment(init="known_poses", niter=2)
    assert torch.equal(al.im_focals.detach(), before) and np.abs(al.get_im_poses().detach().double().cpu().numpy() - sc["c2w"]).max() < 1e-6
    assert np.isfinite(al.losses).all()


# ------------------------------------------------------------------------------------------------ moments and the initialisation
@pytest.mark.parametrize("sizes", [(1000,), (1, 7, 256, 257, 5000, 300000)])
def test_moments(sizes):
    """B = 1 and B = 6 with different n_b (one point; not a multiple of 256; more rows than one; the 1024-row cap) against the
    restatement's fp64 sums, within the bound of a reordered sum of n_b addends"""
    rng = np.random.default_rng(len(sizes))
    tr = [(rng.standard_normal((n, 3)).astype(np.float32), (rng.standard_normal((n, 3)) + 1).astype(np.float32),
           rng.uniform(0.5, 4, n).astype(np.float32)) for n in sizes]
    got = A.DeviceBackend().moments([tuple(torch.from_numpy(x).cuda() for x in t) for t in tr]).numpy()
    again = A.DeviceBackend().moments([tuple(torch.from_numpy(x).cuda() for x in t) for t in tr]).numpy()
    assert got.shape == (len(sizes), 17) and np.array_equal(got.view(np.uint64), again.view(np.uint64))
    for b, (n, t) in enumerate(zip(sizes, tr)):
        want, absum = R.moments_ref(*t)
        assert (np.abs(got[b] - want) <= R.sum_bound(n, absum) + 2 * R.U53 * np.abs(want)).all(), b      # (+ the roundings of w p q itself)
    with pytest.raises(ValueError):
        A.DeviceBackend().moments([])
    with pytest.raises(ValueError):
        A.DeviceBackend().moments([(torch.zeros(4, 3).cuda(), torch.zeros(5, 3).cuda(), torch.zeros(4).cuda())])


# measured on the device: the start poses differ from the CPU path's by 6.0e-8 (one fp32 step of a unit entry) and the loss of the start
# is 2.7e-7 of the scene extent; the bars are 4x the measured values.
POSE_MEASURED, INIT_LOSS_MEASURED = 6.0e-8, 2.7e-7
# the loss after 20 iterations from the perturbed start, device against the restatement-driven loop on the CPU: measured once on the
# device, relative difference 1.50e-6 at iteration 20 (6.8e-8 at the first, never above 4.9e-6 on the way: the two runs drift apart by
# fp32 rounding, not chaotically); the bar is 4x the measured value (README, "Global alignment").
TRAJECTORY_MEASURED = 1.50e-6


def test_mst_init_and_twenty_iterations_follow_the_cpu_path():
    """measured on the device: poses against the CPU path 6.0e-8 (bar 2.4e-7), init loss / extent 2.7e-7 (bar 1.08e-6), the loss after
    20 iterations within 1.50e-6 of the restatement-driven loop (bar 6.0e-6)"""
    sc, cpu, tree, L0, extent, poses, state = TC.sheet_cpu()
    dev = A.GlobalAligner(sc["pairs"])
    dtree = dev.init_minimum_spanning_tree()
    assert dtree == tree and [dev.edges[e] for e in dtree] == [cpu.edges[e] for e in tree]
    dposes = dev.get_im_poses().detach().double().cpu().numpy()
    print("poses, device against the CPU path:", np.abs(dposes - poses).max())
    assert np.abs(dposes - poses).max() <= 4 * POSE_MEASURED
    with torch.no_grad():
        Ld = float(dev())
    print("init loss / extent", Ld / extent)
    assert Ld / extent <= 4 * INIT_LOSS_MEASURED
    TC.perturb(dev)
    last = dev.compute_global_alignment(init=None, niter=20)
    cpu.load_state_dict(state)
    TC.perturb(cpu)
    try:
        cpu.compute_global_alignment(init=None, niter=20)
        want = list(cpu.losses)
    finally:
        cpu.load_state_dict(state)
    rel = [abs(a - b) / b for a, b in zip(dev.losses, want)]
    print("trajectory, relative difference per iteration:", ["%.2e" % r for r in rel])
    assert len(dev.losses) == 20 and last == dev.losses[-1] and dev.losses[-1] < dev.losses[0]
    assert rel[-1] <= 4 * TRAJECTORY_MEASURED


def test_errors_and_empty_sizes():
    sc = R.sheet_scene()
    empty = dict(view1=dict(idx=[]), view2=dict(idx=[]), pred1=dict(pts3d=[], conf=[]), pred2=dict(pts3d_in_other_view=[], conf=[]))
    with pytest.raises(ValueError):
        A.GlobalAligner(empty)                           # E = 0
    with pytest.raises(ValueError):
        A.GlobalAligner(dict(view1=dict(idx=[0])))
    bad = dict(sc["pairs"], pred1=dict(sc["pairs"]["pred1"], pts3d=sc["pairs"]["pred1"]["pts3d"][:, :5]))
    with pytest.raises(ValueError):
        A.GlobalAligner(bad)                             # an image with two shapes
    al = A.GlobalAligner(sc["pairs"])
    with pytest.raises(ValueError):
        al.compute_global_alignment(init="tree")
    with pytest.raises(ValueError):
        al.compute_global_alignment(init="known_poses")  # nothing preset
    with pytest.raises(ValueError):
        al.preset_pose([torch.eye(4)], pose_msk=[0])


# ------------------------------------------------------------------------------------------------ the tiny model
def test_tiny_model_pair_graph_to_fused_mesh(tiny_sd):
    from spann3r_amd import Spann3R, TINY
    from spann3r_amd.fusion import fuse_pointmaps
    from spann3r_amd.runner import pair_graph
    from spann3r_amd.weights import synth_frames
    from conftest import load_golden
    g = load_golden("spann3r_offline.npz")
    H, W = map(int, g["meta_hw"])
    m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False)
    m.load_state_dict(tiny_sd, strict=True)
    m = m.to("cuda").eval()
    frames = [{k: (v.cuda() if k == "img" else v) for k, v in f.items()} for f in synth_frames(3, H, W, seed=int(g["meta_seed"]))]
    with torch.no_grad():
        graph = pair_graph(m.dust3r, frames)
    al = A.GlobalAligner(graph, min_conf_thr=0.0)
    last = al.compute_global_alignment(init="mst", niter=5)
    assert len(al.losses) == 5 and np.isfinite(al.losses).all() and np.isfinite(last)
    with torch.no_grad():
        poses, focals, depths, pts = al.get_im_poses(), al.get_focals().flatten(), al.get_depthmaps(), al.get_pts3d()
    assert torch.isfinite(poses).all()
    lo, hi = A.acceptable_focal_range(H, W)
    assert ((focals >= lo) & (focals <= hi)).all(), (focals.tolist(), lo, hi)
    assert all(bool((d > 0).all()) and tuple(d.shape) == (H, W) for d in depths)
    mesh = fuse_pointmaps(torch.stack(pts).contiguous(), al.get_intrinsics().detach().double().cpu().numpy(), poses.double().cpu().numpy(),
                          torch.stack(al.get_masks()))
    assert isinstance(mesh, dict) and "vertices" in mesh
