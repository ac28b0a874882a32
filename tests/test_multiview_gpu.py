"""spann3r_amd.multiview on the device against the numpy restatement of the header's rule (tests/multiview_ref.py).

The counts are integers of a per-pair predicate whose every fp32 operation is specified (order, one rounding per operation, IEEE
division), and the cleaned confidence is either the input bits or max_bad_conf: every comparison here is exact, in dtype and bits.
No tolerance is used anywhere.  The shapes are the smallest at which the tiling can go wrong: 24 x 32 and 13 x 21 (neither a
multiple of the 16 x 16 block, more than one block), a frame inside a wider buffer, 1 x 1 frames, T = 0, 1, 2.

Parity with DUSt3R's clean_pointcloud is not tested: dust3r.cloud_opt cannot be imported here (tests/multiview_ref.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import fusion_ref as FR
import multiview_ref as R

pytestmark = pytest.mark.gpu

NAMES = ("seen", "agree", "front", "stronger")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _with_kernel_matrices(frames):
    """the restatement's frames with the world-to-camera matrices the kernel is given (fusion.camera_tables' float64 inverse)"""
    from spann3r_amd import fusion as F
    _, w2c = F.camera_tables([f["K"] for f in frames], [f["cam2world"] for f in frames], len(frames))
    for f, m in zip(frames, w2c):
        f["w2c"] = m
        f["fu"], f["fv"], f["cu"], f["cv"] = f["K"][0, 0], f["K"][1, 1], f["K"][0, 2], f["K"][1, 2]
    return frames


def _frame(pts, K, P=None, valid=None):
    return dict(pts=np.asarray(pts, np.float32), K=np.asarray(K, np.float64), cam2world=np.eye(4) if P is None else np.asarray(P, np.float64),
                valid=valid)


def _kw(frames, conf=None, stack=False):
    """the arguments of view_consistency / clean_confidence for the restatement's frames, as lists or as stacks"""
    pts, valid = [_t(f["pts"]) for f in frames], [_t(f.get("valid")) for f in frames]
    cf = None if conf is None else [_t(c) for c in conf]
    if all(v is None for v in valid):
        valid = None
    if stack:
        valid = None if valid is None else [torch.ones(p.shape[:2], dtype=torch.uint8, device="cuda") if v is None else v for p, v in zip(pts, valid)]
        pts, valid, cf = torch.stack(pts), None if valid is None else torch.stack(valid), None if cf is None else torch.stack(cf)
    return dict(pts=pts, intrinsics=[f["K"] for f in frames], cam2world=[f["cam2world"] for f in frames], valid=valid, conf=cf)


def _assert_counts(got, ref):
    """view_consistency's dict (lists or stacks) against counts_ref's list, exactly"""
    for k, name in enumerate(NAMES):
        assert len(got[name]) == len(ref)
        for g, r in zip(got[name], ref):
            assert g.dtype == torch.int32 and tuple(g.shape) == r.shape[:2]
            assert np.array_equal(g.cpu().numpy(), r[..., k]), name
    for g, r in zip(got["behind"], ref):
        assert g.dtype == torch.int32 and np.array_equal(g.cpu().numpy(), R.behind(r))


def _assert_conf(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert g.dtype == torch.float32 and _bits(g.cpu().numpy(), r)


def _check_all(frames, conf, tol, mbc=0.0):
    """counts and both cleaning orders, lists and (where the sizes allow) stacks, against the restatement"""
    from spann3r_amd import multiview as MV
    ref = R.counts_ref(frames, conf, tol)
    same = len({f["pts"].shape for f in frames}) == 1 and (conf is None or all(c is not None for c in conf))      # (what a stack can hold)
    for stack in (False, True) if same else (False,):
        got = MV.view_consistency(tol=tol, **_kw(frames, conf, stack))
        assert isinstance(got["seen"], torch.Tensor) == stack
        _assert_counts(got, ref)
        if conf is None or any(c is None for c in conf):
            continue
        kw = _kw(frames, conf, stack)
        for order in ("sequence", "parallel"):
            want = R.clean_ref(frames, conf, tol, mbc, order)
            clean, counts = MV.clean_confidence(tol=tol, max_bad_conf=mbc, order=order, return_counts=True, **kw)
            assert isinstance(clean, torch.Tensor) == stack
            _assert_conf(clean, want)
            _assert_counts(counts, ref)                                      # against the ORIGINAL confidences in both orders
            _assert_conf(MV.clean_confidence(tol=tol, max_bad_conf=mbc, order=order, **kw), want)
    return ref


@pytest.fixture(scope="module")
def scene():
    return _with_kernel_matrices(FR.as_path(FR.scene_frames(0, 5), "pts")), R.scene_conf()


# ------------------------------------------------------------------------------------------------ the two scenes
@pytest.mark.parametrize("tol", [1e-3, 0.05])
def test_scene_equals_the_restatement(scene, tol):
    from test_multiview_cpu import RULE_TOTALS
    frames, conf = scene
    ref = _check_all(frames, conf, tol)
    assert R.totals(ref) == RULE_TOTALS[tol]
    seq, par = (R.clean_ref(frames, conf, tol, 0.0, o) for o in ("sequence", "parallel"))
    assert any(not _bits(a, b) for a, b in zip(seq, par))                    # the orders differ here: a kernel that ignores it fails


def test_wall_and_order_example_equal_the_restatement():
    from spann3r_amd import multiview as MV
    for patch_conf in (None, 1.5, 9.0):
        frames, conf = R.wall_frames(patch_conf=patch_conf)
        _check_all(_with_kernel_matrices(frames), conf, 1e-3)
    frames, conf = R.wall_frames(patch_conf=1.5)
    got = MV.view_consistency(tol=1e-3, **_kw(_with_kernel_matrices(frames), conf, True))
    f, rows, cols = R.WALL["patch"]
    assert int(got["seen"].sum()) == 7216 and int(got["front"].sum()) == 48 and int(got["behind"].sum()) == 48
    assert bool((got["front"][f][rows, cols] == 3).all()) and int(got["stronger"].sum()) == 48
    frames, conf, a, b = R.order_example()
    frames = _with_kernel_matrices(frames)
    _check_all(frames, conf, 1e-3)
    seq, par = (MV.clean_confidence(tol=1e-3, order=o, **_kw(frames, conf, True)) for o in ("sequence", "parallel"))
    assert float(seq[a]) == 0.0 and float(par[a]) == 0.0 and float(seq[b]) == 3.0 and float(par[b]) == 0.0


# ------------------------------------------------------------------------------------------------ shapes
def test_mixed_sizes_in_one_table(scene):
    """T = 2: 24 x 32 next to the 13 x 21 top-left crop of another frame (the crop keeps its K); neither is a multiple of 16"""
    frames, conf = scene
    small = dict(frames[1], pts=frames[1]["pts"][:13, :21].copy(), valid=frames[1]["valid"][:13, :21].copy())
    for pair, cf in (([frames[0], small], [conf[0], conf[1][:13, :21].copy()]), ([small, frames[3]], [conf[1][:13, :21].copy(), conf[3]])):
        ref = _check_all(pair, cf, 0.05)
        assert R.totals(ref)["seen"] > 100 and R.totals(ref)["front"] > 0


def test_one_pixel_frames_and_T_0_1():
    from spann3r_amd import multiview as MV
    K = np.array([[4.0, 0, 0], [0, 4.0, 0], [0, 0, 1]])
    eyes = [np.eye(4) for _ in range(3)]
    eyes[1][0, 3] = 0.03125
    frames = _with_kernel_matrices([_frame([[[0, 0, 2.0]]], K, eyes[0]), _frame([[[0.03125, 0, 1.0]]], K, eyes[1]),
                                    _frame([[[0, 0, 2.0]]], K, eyes[2], valid=np.ones((1, 1), np.uint8))])
    conf = [np.full((1, 1), c, np.float32) for c in (3.0, 1.0, 2.0)]
    ref = _check_all(frames, conf, 1e-3)
    assert [tuple(c[0, 0]) for c in ref] == [(2, 1, 0, 0), (2, 0, 2, 2), (2, 1, 0, 0)]
    # T = 1: zeros, and the confidence with its input bits (a NaN and a negative zero among them)
    one, cf = frames[:1], [np.array([[np.nan]], np.float32)]
    _check_all(one, cf, 1e-3)
    big = _with_kernel_matrices([_frame(np.random.default_rng(0).normal(size=(13, 21, 3)), K)])
    cfb = np.random.default_rng(1).uniform(-1, 9, (13, 21)).astype(np.float32)
    cfb[0, 0], cfb[12, 20], cfb[5, 5] = np.nan, -0.0, np.inf
    ref = _check_all(big, [cfb], 1e-3)
    assert not ref[0].any()
    # T = 0: as a stack and as a list
    empty = MV.view_consistency(torch.zeros((0, 5, 7, 3), device="cuda"), K, np.zeros((0, 4, 4)))
    assert all(empty[n].shape == (0, 5, 7) and empty[n].dtype == torch.int32 for n in NAMES + ("behind",))
    assert MV.view_consistency([], K, np.zeros((0, 4, 4)))["seen"] == []
    clean, counts = MV.clean_confidence(torch.zeros((0, 5, 7, 3), device="cuda"), torch.zeros((0, 5, 7), device="cuda"), K, np.zeros((0, 4, 4)),
                                        return_counts=True)
    assert clean.shape == (0, 5, 7) and clean.dtype == torch.float32 and counts["front"].shape == (0, 5, 7)
    assert MV.clean_confidence([], [], K, np.zeros((0, 4, 4))) == []


def test_row_stride_wider_than_the_frame_through_the_entry_points(scene):
    """every map of a frame inside a buffer 5 pixels wider, the padding poisoned; outputs prefilled: only w x h may be written"""
    from spann3r_amd import lib as L, multiview as MV
    frames, conf = scene
    frames, conf = frames[:3], conf[:3]
    pad = 5

    def wide(x, fill):
        out = np.full((x.shape[0], x.shape[1] + pad) + x.shape[2:], fill, x.dtype)
        out[:, :x.shape[1]] = x
        return out

    args = _kw([dict(f, pts=wide(f["pts"], np.nan), valid=wide(f["valid"], 1)) for f in frames], [wide(c, 99.0) for c in conf])
    table, table_d, T, keep = MV.frame_table(**args)
    for e in table:
        e.w -= pad
    table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    lib = L.load()
    for fn, order in ((lib.sp3_multiview_counts, "parallel"), (lib.sp3_multiview_clean, "sequence")):
        counts = [torch.full(tuple(p.shape[:2]) + (4,), -7, dtype=torch.int32, device="cuda") for p in keep["pts"]]
        out_c = [torch.full(tuple(p.shape[:2]), -5.0, dtype=torch.float32, device="cuda") for p in keep["pts"]]
        out = (L.MultiviewOut * T)()
        for i in range(T):
            out[i].counts, out[i].conf_out, out[i].max_bad_conf = counts[i].data_ptr(), out_c[i].data_ptr(), 0.5
        out_d = torch.frombuffer(bytearray(bytes(out)), dtype=torch.uint8).cuda()
        L.check(fn(table, table_d.data_ptr(), T, 0.05, out, out_d.data_ptr(), L.stream_ptr()), "multiview")
        torch.cuda.synchronize()
        ref, want = R.counts_ref(frames, conf, 0.05), R.clean_ref(frames, conf, 0.05, 0.5, order)
        for i in range(T):
            w = frames[i]["pts"].shape[1]
            assert np.array_equal(counts[i][:, :w].cpu().numpy(), ref[i]) and bool((counts[i][:, w:] == -7).all())
            assert _bits(out_c[i][:, :w].cpu().numpy(), want[i]) and bool((out_c[i][:, w:] == -5.0).all())
        assert R.totals(ref)["stronger"] > 0


# ------------------------------------------------------------------------------------------------ the borders of the lookup
def _border_case(tol):
    """A 4 x 4 target frame (identity pose, fu = fv = 8, cu = cv = 1, depth 2: every number exact) and a 1 x N probe frame whose pixels
    are the border cases -> (frames, conf, expected (seen, agree, front, stronger) per probe pixel at this tol)."""
    K = np.array([[8.0, 0, 1.0], [0, 8.0, 1.0], [0, 0, 1]])
    ys, xs = np.mgrid[0:4, 0:4]
    tgt = np.stack([(xs - 1.0) / 8 * 2, (ys - 1.0) / 8 * 2, np.full((4, 4), 2.0)], -1).astype(np.float32)
    tvalid = np.ones((4, 4), np.uint8)
    tconf = np.full((4, 4), 3.0, np.float32)
    tvalid[3, 0] = 0                                                 # the special pixels: row 3 and (2, 0)
    tgt[3, 1, 2], tgt[3, 2, 2], tgt[3, 3, 2], tgt[2, 0, 2] = np.nan, np.inf, 0.0, -2.0
    tconf[1, 2] = np.nan

    def ray(py, px, z):
        return ((px - 1.0) / 8 * z, (py - 1.0) / 8 * z, z)

    f32 = np.float32
    lo, hi = f32(f32(1) - f32(tol)) * f32(2), f32(f32(1) + f32(tol)) * f32(2)
    below_lo, above_hi = np.nextafter(lo, f32(0)), np.nextafter(hi, f32(9))
    NOT, AGREE, FRONT, BEHIND = (0, 0, 0, 0), (1, 1, 0, 0), (1, 0, 1, 0), (1, 0, 0, 0)
    cases = [  # (point, confidence, valid_i, expected)
        ((-0.375, 0.0, 2.0), 3.0, 1, AGREE),                     # u = -0.5: floor(0.0) = 0, in
        ((0.625, 0.0, 2.0), 3.0, 1, NOT),                        # u = w - 0.5 = 3.5: floor(4.0) = 4, out
        ((0.0, -0.375, 2.0), 3.0, 1, AGREE),                     # v = -0.5: in
        ((0.0, 0.625, 2.0), 3.0, 1, NOT),                        # v = h - 0.5 = 3.5: out
        ((0.0, 0.0, 0.0), 3.0, 1, NOT),                          # zc = 0
        ((0.0, 0.0, -2.0), 3.0, 1, NOT),                         # zc < 0
        (ray(1, 1, float(lo)), 3.0, 1, AGREE),                   # zc == lo exactly: agree, not front
        (ray(1, 1, float(below_lo)), 3.0, 1, FRONT if below_lo < lo else AGREE),
        (ray(1, 1, float(hi)), 3.0, 1, AGREE),                   # zc == hi exactly: agree
        (ray(1, 1, float(above_hi)), 3.0, 1, BEHIND),
        (ray(3, 0, 2.0), 3.0, 1, NOT),                           # valid_j == 0 at the target
        (ray(3, 1, 2.0), 3.0, 1, NOT),                           # d NaN
        (ray(3, 2, 2.0), 3.0, 1, NOT),                           # d inf
        (ray(3, 3, 2.0), 3.0, 1, NOT),                           # d 0
        (ray(2, 0, 2.0), 3.0, 1, NOT),                           # d negative
        ((np.nan, 0.0, 2.0), 3.0, 1, NOT), ((0.0, np.nan, 2.0), 3.0, 1, NOT), ((0.0, 0.0, np.nan), 3.0, 1, NOT),
        ((np.inf, 0.0, 2.0), 3.0, 1, NOT), ((0.0, -np.inf, 2.0), 3.0, 1, NOT), ((0.0, 0.0, np.inf), 3.0, 1, NOT),
        (ray(1, 1, 2.0), 3.0, 0, NOT),                           # valid_i == 0
        (ray(1, 1, 1.0), 2.0, 1, (1, 0, 1, 1)),                  # front and weaker: stronger
        (ray(1, 1, 1.0), 3.0, 1, FRONT),                         # equal confidences: not stronger
        (ray(1, 1, 1.0), np.nan, 1, FRONT),                      # NaN on this side
        (ray(1, 2, 1.0), 2.0, 1, FRONT),                         # NaN at the target
        (ray(1, 1, 1.0), 2.0, 0, NOT),                           # valid_i == 0 although it would be stronger
    ]
    n = len(cases)
    probe = np.array([c[0] for c in cases], np.float32).reshape(1, n, 3)
    pconf = np.array([c[1] for c in cases], np.float32).reshape(1, n)
    pvalid = np.array([c[2] for c in cases], np.uint8).reshape(1, n)
    far = np.eye(4)
    far[:3, 3] = (50.0, 50.0, 50.0)                                  # the probe frame's own camera sees nothing of the target
    frames = _with_kernel_matrices([_frame(probe, K, far, pvalid), _frame(tgt, K, None, tvalid)])
    return frames, [pconf, tconf], np.array([c[3] for c in cases], np.int32)


@pytest.mark.parametrize("tol", [0.125, 0.0, 1e-3])
def test_borders_of_the_lookup(tol):
    frames, conf, expected = _border_case(tol)
    ref = _check_all(frames, conf, tol, mbc=1.0)
    assert np.array_equal(ref[0][0], expected), (ref[0][0], expected)     # the restatement says what the rule text says
    assert not ref[1].any()                                              # nothing of the target lands in the probe frame
    # the cleaning on these: only the front-and-weaker probe is clipped, NaN passes through
    for order in ("sequence", "parallel"):
        out = R.clean_ref(frames, conf, tol, 1.0, order)[0][0]
        changed = out.view(np.uint32) != conf[0][0].view(np.uint32)
        assert np.array_equal(changed, expected[:, 3] > 0) and (out[changed] == 1.0).all()


# ------------------------------------------------------------------------------------------------ confidences and arguments
def test_frames_without_confidence(scene):
    from spann3r_amd import multiview as MV
    frames, conf = scene
    some = [conf[0], None, conf[2], conf[3], None]
    ref = _check_all(frames, some, 0.05)
    assert not ref[1][..., 3].any() and not ref[4][..., 3].any() and ref[0][..., 3].any()
    _check_all(frames, None, 0.05)
    with pytest.raises(ValueError, match="every frame needs a confidence"):
        MV.clean_confidence(tol=0.05, **_kw(frames, some))
    with pytest.raises(ValueError, match="every frame needs a confidence"):
        MV.clean_confidence(tol=0.05, **_kw(frames, None))


def test_argument_errors(scene):
    from spann3r_amd import lib as L, multiview as MV
    frames, conf = scene
    frames, conf = frames[:2], conf[:2]
    kw = _kw(frames, conf)
    for tol in (-1e-3, 1.0, 2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tol"):
            MV.view_consistency(tol=tol, **kw)
        with pytest.raises(ValueError, match="tol"):
            MV.clean_confidence(tol=tol, **kw)
    with pytest.raises(ValueError, match="order"):
        MV.clean_confidence(order="reverse", **kw)
    with pytest.raises(ValueError, match="max_bad_conf"):
        MV.clean_confidence(max_bad_conf=float("nan"), **kw)
    skew = frames[0]["K"].copy()
    skew[0, 1] = 0.01
    with pytest.raises(ValueError, match="skew"):
        MV.view_consistency(**dict(kw, intrinsics=[skew, frames[1]["K"]]))
    flat = frames[1]["cam2world"].copy()
    flat[:3, 2] = 0.0
    with pytest.raises(ValueError, match="singular"):
        MV.view_consistency(**dict(kw, cam2world=[frames[0]["cam2world"], flat]))
    with pytest.raises(ValueError):
        MV.view_consistency(**dict(kw, cam2world=[frames[0]["cam2world"]]))
    with pytest.raises(RuntimeError, match="mismatched lengths"):
        MV.view_consistency(**dict(kw, conf=kw["conf"][:1]))
    with pytest.raises(RuntimeError, match="mismatched lengths"):
        MV.view_consistency(**dict(kw, valid=kw["valid"] + kw["valid"]))
    with pytest.raises(RuntimeError, match="mismatched shapes"):
        MV.view_consistency(**dict(kw, conf=[kw["conf"][0], kw["conf"][1][:, :-1]]))
    with pytest.raises(RuntimeError, match="must be"):
        MV.view_consistency(**dict(kw, pts=[kw["pts"][0], kw["pts"][1][..., :2]]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        MV.view_consistency(**dict(kw, pts=[p.cpu() for p in kw["pts"]]))
    # the entry points themselves: a depth frame, and a conf_out that is a pixel_weight
    lib = L.load()
    table, table_d, T, keep = MV.frame_table(**kw)
    counts = [torch.zeros(tuple(p.shape[:2]) + (4,), dtype=torch.int32, device="cuda") for p in keep["pts"]]
    fresh = [torch.empty_like(c) for c in keep["conf"]]
    out = (L.MultiviewOut * T)()
    for i in range(T):
        out[i].counts, out[i].conf_out = counts[i].data_ptr(), fresh[i].data_ptr()
    out_d = torch.frombuffer(bytearray(bytes(out)), dtype=torch.uint8).cuda()
    depth = (L.TsdfFrame * T)()
    C.memmove(depth, table, C.sizeof(table))
    depth[1].depth, depth[1].pts = depth[1].pts, None
    for fn in (lib.sp3_multiview_counts, lib.sp3_multiview_clean):
        with pytest.raises(RuntimeError, match="gives depth"):
            L.check(fn(depth, table_d.data_ptr(), T, 1e-3, out, out_d.data_ptr(), L.stream_ptr()), "multiview")
    out[0].conf_out, out[1].conf_out = keep["conf"][1].data_ptr(), counts[1].data_ptr()
    for fn in (lib.sp3_multiview_counts, lib.sp3_multiview_clean):
        with pytest.raises(RuntimeError, match="aliases a pixel_weight"):
            L.check(fn(table, table_d.data_ptr(), T, 1e-3, out, out_d.data_ptr(), L.stream_ptr()), "multiview")
    with pytest.raises(RuntimeError, match="null conf_out"):
        out[0].conf_out = None
        L.check(lib.sp3_multiview_clean(table, table_d.data_ptr(), T, 1e-3, out, out_d.data_ptr(), L.stream_ptr()), "multiview")


@pytest.mark.parametrize("mbc", [0.0, 1.0, 4.0])
def test_parallel_order_is_the_stronger_count(scene, mbc):
    from spann3r_amd import multiview as MV
    frames, conf = scene
    kw = _kw(frames, conf, True)
    counts = MV.view_consistency(tol=0.05, **kw)
    clean = MV.clean_confidence(tol=0.05, max_bad_conf=mbc, order="parallel", **kw)
    cf = kw["conf"]
    want = torch.where(counts["stronger"] > 0, torch.minimum(cf, torch.tensor(mbc, device="cuda")), cf)
    assert int((counts["stronger"] > 0).sum()) == 212 and torch.equal(clean.view(torch.int32), want.view(torch.int32))
    mask = MV.support_mask(counts, min_agree=1, max_front=0)
    assert mask.dtype == torch.bool and torch.equal(mask, (counts["agree"] >= 1) & (counts["front"] == 0)) and bool(mask.any()) and not bool(mask.all())
    listed = MV.support_mask(MV.view_consistency(tol=0.05, **_kw(frames, conf)), 2, 1)
    assert all(torch.equal(m, (a >= 2) & (f <= 1)) for m, a, f in zip(listed, counts["agree"], counts["front"]))


# ------------------------------------------------------------------------------------------------ composition with what exists
def test_clean_sequence_on_the_tiny_model(tiny_sd):
    """the tiny model's geometry means nothing (a focal near 0, which clean_sequence refuses as fuse_sequence does): with a focal and
    poses given, clean_sequence is clean_confidence on sequence_tensors' output"""
    from spann3r_amd import Spann3R, TINY, mesh as M, multiview as MV
    from spann3r_amd.weights import synth_frames
    m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False)
    m.load_state_dict(tiny_sd, strict=True)
    m = m.to("cuda:0").eval()
    batch = [{"img": f["img"].to("cuda:0")} for f in synth_frames(3, 64, 80)]
    preds, _ = m(batch)
    with pytest.raises(RuntimeError, match="degenerate pointmaps"):
        MV.clean_sequence(preds, batch)
    poses = np.stack([np.eye(4)] * 3)
    poses[1, 0, 3], poses[2, 1, 3] = 0.05, -0.05
    pts_all, images_all, conf_all = M.sequence_tensors(preds, batch)
    t, h, w, _ = pts_all.shape
    K = np.array([[80.0, 0, w / 2], [0, 80.0, h / 2], [0, 0, 1]])
    for order in ("sequence", "parallel"):
        pts, images, clean, info = MV.clean_sequence(preds, batch, tol=0.05, order=order, focal=80.0, poses=poses)
        want = MV.clean_confidence(pts_all, conf_all, K, poses, tol=0.05, order=order)
        assert torch.equal(pts, pts_all) and torch.equal(images, images_all) and clean.dtype == torch.float32 and clean.shape == conf_all.shape
        assert torch.equal(clean.view(torch.int32), want.view(torch.int32))
        assert info["focal"] == 80.0 and np.array_equal(info["poses"], poses)
        assert info["cleaned"] == (clean.view(torch.int32) != conf_all.view(torch.int32)).flatten(1).sum(1).tolist()


def _wall_sequence():
    """the wall with the floater as model.forward would hand it over (principal point at the image centre, which fuse_sequence
    assumes): preds, batch, focal, poses, the restatement's frames and confidences"""
    frames, conf = R.wall_frames(patch_conf=1.5, cu=R.WALL["w"] / 2, cv=R.WALL["h"] / 2)
    rng = np.random.default_rng(3)
    preds = [{"pts3d" if i == 0 else "pts3d_in_other_view": _t(f["pts"])[None], "conf": _t(c)[None]} for i, (f, c) in enumerate(zip(frames, conf))]
    batch = [{"img": _t(rng.uniform(-1, 1, (1, 3, R.WALL["h"], R.WALL["w"])).astype(np.float32))} for _ in frames]
    return preds, batch, R.WALL["fu"], np.stack([f["cam2world"] for f in frames]), _with_kernel_matrices(frames), conf


def test_fuse_sequence_with_cleaned_confidences():
    from spann3r_amd import fusion as F, mesh as M, multiview as MV
    from spann3r_amd.postprocess import confident_points
    preds, batch, focal, poses, frames, conf = _wall_sequence()
    kw = dict(conf_thresh=1e-3, dims_max=48, focal=focal, poses=poses)
    plain, off = F.fuse_sequence(preds, batch, **kw), F.fuse_sequence(preds, batch, clean_tol=None, **kw)
    for k in ("vertices", "colors", "faces"):
        assert torch.equal(plain[k], off[k])
    assert np.array_equal(plain["bounds"], off["bounds"])
    pts_all, images_all, conf_all = M.sequence_tensors(preds, batch)
    K = np.array([[focal, 0, R.WALL["w"] / 2], [0, focal, R.WALL["h"] / 2], [0, 0, 1]])
    for order in ("sequence", "parallel"):
        clean = MV.clean_confidence(pts_all, conf_all, K, poses, tol=1e-3, order=order)
        _assert_conf(clean, R.clean_ref(frames, conf, 1e-3, 0.0, order))
        got = F.fuse_sequence(preds, batch, clean_tol=1e-3, clean_order=order, **kw)
        want = F.fuse_pointmaps(pts_all, K, poses, (clean - 1) / clean > 1e-3, images_all, dims_max=48)
        for k in ("vertices", "colors", "faces"):
            assert torch.equal(got[k], want[k])
        assert got["faces"].shape[0] > 0
        # (the volume's own free-space rule already carves this floater away, so the surface is not what shows the cleaning; the
        # confident cloud is: it loses exactly the 16 points of the patch)
        before, _ = confident_points(pts_all, conf_all, 1e-3)
        after, _ = confident_points(pts_all, clean, 1e-3)
        f, rows, cols = R.WALL["patch"]
        keep = torch.ones(conf_all.shape, dtype=torch.bool, device="cuda")
        keep[f][rows, cols] = False
        assert before.shape[0] == conf_all.numel() and after.shape[0] == before.shape[0] - 16
        assert torch.equal(after, pts_all[keep])
