"""Backward through the memory fusion: the HIP forward / backward of the train-mode spatial-memory read
against the CPU oracle in float64 with autograd; the oracle against the unmodified reference module."""
import os

import numpy as np

import pytest
import torch

from conftest import rel_err
from oracle import train_oracle as TO


MEMREAD_GRAD_TOL = 1e-5          # measured 8.2e-7


def _inputs(B, P, T, C, seed, dtype=torch.float32, device="cpu", p_drop=0.15):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    t = dict(feat=rn(B, P, C), mem_k=rn(B, T, C) * 1.3 + 0.1, mem_v=rn(B, T, C) * 0.8 - 0.2)
    for n in ("q", "k", "v"):
        t["g" + n], t["b" + n] = 1.0 + 0.2 * rn(C), 0.1 * rn(C)
    mask = (torch.rand(B, P, T, generator=g) >= p_drop).float() / (1.0 - p_drop)
    dout = rn(B, P, C)
    leaves = {k: v.to(dtype).to(device).requires_grad_(True) for k, v in t.items()}
    return leaves, mask.to(dtype).to(device), dout.to(dtype).to(device)


def _run(fn, leaves, mask, dout):
    out = fn(leaves["feat"], leaves["mem_k"], leaves["mem_v"], (leaves["gq"], leaves["bq"]), (leaves["gk"], leaves["bk"]),
             (leaves["gv"], leaves["bv"]), mask)
    out.backward(dout)
    return out.detach(), {k: v.grad for k, v in leaves.items()}


MEMREAD_REF_CASE = (2, 24, 72, 64, 3)        # B, P, T, C, seed of the stored reference read (tests/golden/make_golden.py memread)


def test_oracle_matches_reference_memory_read():
    """the oracle's train-mode read against the output of the unmodified reference module on the same seeded inputs
    (tests/golden/memory_read_train.npz: SpatialMemory.memory_read(res=True) after two add_mem calls, attn_thresh = 0, no dropout)"""
    from conftest import load_golden
    B, P, T, C, seed = MEMREAD_REF_CASE
    leaves, _, _ = _inputs(B, P, T, C, seed=seed)
    g = load_golden("memory_read_train.npz")
    assert np.array_equal(g["feat"], leaves["feat"].detach().numpy())             # the fixture was made from these inputs
    ref = torch.from_numpy(g["out"])
    got = TO.memory_read_train(leaves["feat"], leaves["mem_k"], leaves["mem_v"], (leaves["gq"], leaves["bq"]), (leaves["gk"], leaves["bk"]),
                               (leaves["gv"], leaves["bv"]), None)
    assert rel_err(got.detach(), ref.detach()) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("B,P,T,C,drop", [(1, 196, 588, 1024, True), (2, 50, 150, 256, True), (1, 37, 111, 128, False)])
def test_memory_read_train_forward_backward(B, P, T, C, drop):
    from spann3r_amd.train import memory_read_train
    leaves, mask, dout = _inputs(B, P, T, C, seed=P, device="cuda")
    out, grads = _run(memory_read_train, leaves, mask if drop else None, dout)
    l64, m64, d64 = _inputs(B, P, T, C, seed=P, dtype=torch.float64)
    ref, gref = _run(TO.memory_read_train, l64, m64 if drop else None, d64)
    assert rel_err(out.cpu(), ref) < 1e-5
    worst = (0.0, None)
    for k in grads:
        if k == "bk":        # softmax is invariant to a shift of every score of a row: d out / d beta_k == 0 exactly
            assert float(gref[k].abs().max()) < 1e-12 and float(grads[k].abs().max()) < 1e-5 * float(grads["gk"].abs().max())
            continue
        worst = max(worst, (rel_err(grads[k].cpu(), gref[k]), k))
    print("memory read (train) gradients: worst rel err %.2e (%s)" % worst)
    assert worst[0] < MEMREAD_GRAD_TOL, worst
    # deterministic: a second run gives the same bits
    leaves2, _, _ = _inputs(B, P, T, C, seed=P, device="cuda")
    out2, grads2 = _run(memory_read_train, leaves2, mask if drop else None, dout)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


def _block_params(C, seed, cross, dtype, device):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    P = {}
    def lin(name, n, k):
        P[name + ".weight"], P[name + ".bias"] = rn(n, k) * (k ** -0.5), 0.1 * rn(n)
    def ln(name):
        P[name + ".weight"], P[name + ".bias"] = 1 + 0.2 * rn(C), 0.1 * rn(C)
    ln("b.norm1"); lin("b.attn.qkv", 3 * C, C); lin("b.attn.proj", C, C)
    ln("b.norm2"); lin("b.mlp.fc1", 4 * C, C); lin("b.mlp.fc2", C, 4 * C)
    if cross:
        ln("b.norm3"); ln("b.norm_y")
        for n in ("projq", "projk", "projv", "proj"):
            lin("b.cross_attn." + n, C, C)
    return {k: v.to(dtype).to(device).requires_grad_(True) for k, v in P.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,H,hd,rope", [(2, 196, 3, 64, True), (1, 37, 2, 64, True), (3, 70, 4, 48, False), (2, 64, 1, 64, True)])
def test_head_shuffle_split_rope_transpose_and_merge(B, N, H, hd, rope):
    """sp3_head_shuffle: [B, N, 3C] -> per-head q, k (RoPE2D), v and their transposes (pad columns zero) in one launch; the
    backward direction (inverse rotation, merge) is its exact transpose"""
    from spann3r_amd import train as T
    from oracle import spann3r_oracle as O
    C = H * hd
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn(B, N, 3 * C, generator=g)
    nh = 7 if N % 7 == 0 else 1
    pos = O.positions(B, nh, N // nh)
    Np = (N + 7) // 8 * 8
    outs, outsT = [], []
    parts = []
    dev_qkv, dev_pos = qkv.cuda(), pos.cuda()
    for i in range(3):
        dst = torch.full((B * H, N, hd), float("nan"), device="cuda")
        dstT = torch.full((B * H, hd, Np), float("nan"), device="cuda")
        outs.append(dst); outsT.append(dstT)
        parts.append(dict(src=dev_qkv[0, 0, i * C:], s=(N * 3 * C, 3 * C, hd), N=N, dst=dst, d=(H * N * hd, hd, N * hd), dstT=dstT,
                          pos=dev_pos if (rope and i < 2) else None, fwd=1.0))
    T._head_shuffle(parts, B, H, hd, 100.0)
    for i in range(3):
        ref = qkv[:, :, i * C:(i + 1) * C].reshape(B, N, H, hd).permute(0, 2, 1, 3).double()        # [B, H, N, hd]
        if rope and i < 2:
            ref = O.rope2d(ref, pos, 100.0)
        ref = ref.reshape(B * H, N, hd)
        assert rel_err(outs[i].cpu(), ref) < 5e-6            # (fp32 sin / cos of the angles)
        tT = outsT[i].cpu()
        assert torch.equal(tT[:, :, :N], outs[i].cpu().transpose(1, 2)) and float(tT[:, :, N:].abs().sum()) == 0.0
    # merge with the inverse rotation undoes the split exactly up to rounding
    back = torch.full((B, N, 3 * C), float("nan"), device="cuda")
    parts = [dict(src=outs[i], s=(H * N * hd, hd, N * hd), N=N, dst=back[0, 0, i * C:], d=(N * 3 * C, 3 * C, hd),
                  pos=dev_pos if (rope and i < 2) else None, fwd=-1.0) for i in range(3)]
    T._head_shuffle(parts, B, H, hd, 100.0)
    assert rel_err(back.cpu(), qkv) < 5e-6


@pytest.mark.gpu
def test_transpose_and_softmax_backward_write_their_pads():
    from spann3r_amd import train as T
    from spann3r_amd import lib as L
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 197, 50, generator=g).cuda()
    t = T._tb(x, 197, 50, 50, 5, 197 * 50)
    assert t.shape == (5, 50, 200) and torch.equal(t[:, :, :197], x.transpose(1, 2)) and float(t[:, :, 197:].abs().sum()) == 0.0
    t2 = T._transpose(x[0], 197, 50, 50)
    assert torch.equal(t2, t[0])
    A = torch.softmax(torch.randn(40, 197, generator=g), -1)
    dA = torch.randn(40, 197, generator=g)
    Ap, dAp = torch.zeros(40, 200), torch.zeros(40, 200)
    Ap[:, :197], dAp[:, :197] = A, dA
    dS = torch.full((40, 200), float("nan"), device="cuda")
    Ad, dAd = Ap.cuda(), dAp.cuda()
    L.check(L.load().sp3_softmax_bwd_pad(Ad.data_ptr(), dAd.data_ptr(), None, dS.data_ptr(), 200, 40, 197, 200, 0.5, L.stream_ptr()), "sp3_softmax_bwd_pad")
    ref = 0.5 * A.double() * (dA.double() - (dA.double() * A.double()).sum(-1, keepdim=True))
    assert rel_err(dS[:, :197].cpu(), ref) < 1e-5 and float(dS[:, 197:].abs().sum()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("gain", [1.0, 6.0])
def test_flash_attention_is_as_close_to_float64_as_the_materialised_one(gain):
    """The two fp32 attention paths of the train-mode blocks against float64 on the same q, k, v (gain 6: peaked softmax rows with
    scores of +-60): output and the three input gradients.  Neither reproduces the other's rounding, both must sit at fp32 level."""
    from spann3r_amd import train as T
    B, N, Nk, H = 2, 196, 201, 4
    C = 64 * H
    g = torch.Generator().manual_seed(11)
    q0, k0, v0, d0 = (torch.randn(B, n, C, generator=g) for n in (N, Nk, Nk, N))
    q0, k0 = q0 * gain, k0 * gain
    scale = 64 ** -0.5
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q0, k0, v0))
    hd = lambda t, n: t.reshape(B, n, H, 64).transpose(1, 2)
    a = torch.softmax(hd(qd, N) @ hd(kd, Nk).transpose(-1, -2) * scale, -1)
    ref = (a @ hd(vd, Nk)).transpose(1, 2).reshape(B, N, C)
    ref.backward(d0.double())
    refs = [ref.detach(), qd.grad, kd.grad, vd.grad]
    errs = {}
    try:
        for mode, flash in (("flash", True), ("gemm", False)):
            T.FLASH_ATTENTION = flash
            q, k, v = (t.cuda().requires_grad_(True) for t in (q0, k0, v0))
            out = T._mha(q, k, v, None, None, H, scale, 100.0)
            out.backward(d0.cuda())
            errs[mode] = [rel_err(x.detach().cpu(), r) for x, r in zip((out, q.grad, k.grad, v.grad), refs)]
    finally:
        T.FLASH_ATTENTION = True
    print("attention vs float64 (gain %g): flash %s, materialised %s" % (gain, ["%.1e" % e for e in errs["flash"]], ["%.1e" % e for e in errs["gemm"]]))
    lim = 2e-6 if gain == 1.0 else 4e-5           # measured 7e-7 / 1.3e-5 (flash), 6e-7 / 9e-6 (materialised): scores of +-60 cost 2 digits in both
    assert max(errs["flash"]) < lim and max(errs["gemm"]) < lim, errs
    assert all(f < 3 * m + 3e-7 for f, m in zip(errs["flash"], errs["gemm"])), errs


@pytest.mark.gpu
@pytest.mark.parametrize("N,Nk", [(196, 201), (64, 256), (300, 260), (37, 500)])
def test_flash_attention_bf16_products(N, Nk):
    """bf16 training precision: the flash kernels with bf16 products (one to eight 64-row tiles per wave) against float64, next to the
    materialised path with the same operand rounding (fp32 operands rounded to bf16 inside the GEMMs)"""
    from spann3r_amd import train as T
    B, H = 2, 3
    C = 64 * H
    g = torch.Generator().manual_seed(N)
    q0, k0, v0, d0 = (torch.randn(B, n, C, generator=g) for n in (N, Nk, Nk, N))
    scale = 64 ** -0.5
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q0, k0, v0))
    hd = lambda t, n: t.reshape(B, n, H, 64).transpose(1, 2)
    a = torch.softmax(hd(qd, N) @ hd(kd, Nk).transpose(-1, -2) * scale, -1)
    ref = (a @ hd(vd, Nk)).transpose(1, 2).reshape(B, N, C)
    ref.backward(d0.double())
    refs = [ref.detach(), qd.grad, kd.grad, vd.grad]
    errs = {}
    T.set_precision("bf16")
    try:
        for mode, flash in (("flash", True), ("gemm", False)):
            T.FLASH_ATTENTION = flash
            q, k, v = (t.cuda().requires_grad_(True) for t in (q0, k0, v0))
            out = T._mha(q, k, v, None, None, H, scale, 100.0)
            out.backward(d0.cuda())
            errs[mode] = [rel_err(x.detach().cpu(), r) for x, r in zip((out, q.grad, k.grad, v.grad), refs)]
    finally:
        T.FLASH_ATTENTION = True
        T.set_precision("fp32")
    print("bf16 attention vs float64 (%d x %d): flash %s, materialised %s" % (N, Nk, ["%.1e" % e for e in errs["flash"]], ["%.1e" % e for e in errs["gemm"]]))
    assert max(errs["flash"]) < 2e-2 and all(f < 2 * m + 2e-3 for f, m in zip(errs["flash"], errs["gemm"])), errs


@pytest.mark.gpu
@pytest.mark.parametrize("cross", [False, True])
def test_fused_heads_match_the_separate_reshapes(cross):
    """_FlashMHA (no attention matrix) and _MHA (one shuffle launch each way around the GEMMs) against the ATen reshapes + _Attention"""
    from spann3r_amd import train as T
    from oracle import spann3r_oracle as O
    B, nh, nw, C, H = 2, 14, 14, 192, 3
    N = nh * nw
    g = torch.Generator().manual_seed(5)
    x0, y0, d0 = torch.randn(B, N, C, generator=g), torch.randn(B, N + 5, C, generator=g), torch.randn(B, N, C, generator=g)
    pos = O.positions(B, nh, nw).cuda()
    ypos = torch.cat((pos, pos[:, :5]), 1).contiguous()
    res = {}
    try:
        for mode, (fused, flash) in {"flash": (True, True), "gemm": (True, False), "aten": (False, False)}.items():
            T.FUSED_HEADS, T.FLASH_ATTENTION = fused, flash
            P = _block_params(C, 3, cross, torch.float32, "cuda")
            x, y = x0.cuda().requires_grad_(True), y0.cuda().requires_grad_(True)
            out = T.decoder_block(x, y, pos, ypos, P, "b.", H) if cross else T.block(x, pos, P, "b.", H)
            out.backward(d0.cuda())
            res[mode] = (out.detach(), {**{k: v.grad for k, v in P.items()}, "x": x.grad, **({"y": y.grad} if cross else {})})
    finally:
        T.FUSED_HEADS = T.FLASH_ATTENTION = True
    for mode in ("flash", "gemm"):
        assert rel_err(res[mode][0], res["aten"][0]) < 2e-6, mode
        worst = max((rel_err(res[mode][1][k], v), k) for k, v in res["aten"][1].items())
        print("attention path %s vs the ATen reshapes: worst gradient rel err %.2e (%s)" % (mode, worst[0], worst[1]))
        assert worst[0] < 5e-6, (mode, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("cross,grid,rope", [(False, (5, 7), True), (True, (5, 7), True), (False, (14, 14), True), (True, (14, 14), True),
                                             (False, (14, 14), False)])
def test_vit_blocks_forward_backward(cross, grid, rope):
    """Block / DecoderBlock (croco/models/blocks.py:127-130,186-191) in train mode: HIP forward and backward against the
    oracle's functional block in float64 + autograd"""
    from spann3r_amd import train as T
    from oracle import spann3r_oracle as O
    B, (nh, nw), C, H = 2, grid, 128, 2                   # head_dim 64: the RoPE kernel's geometry
    N = nh * nw
    g = torch.Generator().manual_seed(1)
    x0, y0, d0 = torch.randn(B, N, C, generator=g), torch.randn(B, N + 5, C, generator=g), torch.randn(B, N, C, generator=g)
    pos = O.positions(B, nh, nw)
    ypos = torch.cat((pos, pos[:, :5]), 1)
    res = {}
    for name, dt, dev in (("hip", torch.float32, "cuda"), ("ref", torch.float64, "cpu")):
        P = _block_params(C, 3, cross, dt, dev)
        x = x0.to(dt).to(dev).requires_grad_(True)
        y = y0.to(dt).to(dev).requires_grad_(True)
        if name == "hip":
            out = T.decoder_block(x, y, pos.to(dev), ypos.to(dev), P, "b.", H) if cross else T.block(x, pos.to(dev), P, "b.", H, use_rope=rope)
        else:
            out = O.decoder_block(x, y, pos, ypos, P, "b.", H, 100.0) if cross else O.block(x, pos, P, "b.", H, 100.0, use_rope=rope)
        out.backward(d0.to(dt).to(dev))
        res[name] = (out.detach().cpu(), {**{k: v.grad.cpu() for k, v in P.items()}, "x": x.grad.cpu(), **({"y": y.grad.cpu()} if cross else {})})
    assert rel_err(res["hip"][0], res["ref"][0]) < 1e-5
    worst = max((rel_err(res["hip"][1][k], v), k) for k, v in res["ref"][1].items())
    print("ViT block (cross=%s) gradients: worst rel err %.2e (%s)" % (cross, worst[0], worst[1]))
    assert worst[0] < 1e-5, worst            # measured 5.4e-7


@pytest.mark.gpu
def test_dpt_head_train_forward_backward(tiny_sd):
    """DPT head + postprocess in train mode (im2col + linear convolutions, bilinear adjoint, expm1 head) against the oracle's
    downstream_head in float64 + autograd: outputs, gradients w.r.t. the four hooked decoder outputs and every head parameter"""
    from spann3r_amd import train as T, TINY
    from oracle import spann3r_oracle as O
    cfg = TINY
    B, nh, nw = 1, 3, 4
    g = torch.Generator().manual_seed(2)
    widths = [cfg.enc_dim] + [cfg.dec_dim] * cfg.dec_depth
    dec0 = [torch.randn(B, nh * nw, w_, generator=g) for w_ in widths]
    H, W = nh * cfg.patch, nw * cfg.patch
    gp, gc = torch.randn(B, H, W, 3, generator=g), torch.randn(B, H, W, generator=g)
    keys = [k for k in tiny_sd if k.startswith("dust3r.downstream_head1.dpt.")]
    res = {}
    for name, dt, dev in (("hip", torch.float32, "cuda"), ("ref", torch.float64, "cpu")):
        P = {k: tiny_sd[k].to(dt).to(dev).requires_grad_(True) for k in keys}
        dec = [d.to(dt).to(dev).requires_grad_(i in cfg.hooks) for i, d in enumerate(dec0)]
        if name == "hip":
            pts, conf = T.dpt_head(dec, nh, nw, P, cfg, 1)
        else:
            r = O.downstream_head(dec, torch.tensor([[H, W]] * B), P, cfg, 1)
            pts, conf = r["pts3d"], r["conf"]
        (pts * gp.to(dt).to(dev)).sum().add((conf * gc.to(dt).to(dev)).sum()).backward()
        grads = {k: (None if v.grad is None else v.grad.cpu()) for k, v in P.items()}     # (refinenet4.resConfUnit1 is never used)
        grads.update({"dec%d" % i: dec[i].grad.cpu() for i in cfg.hooks})
        res[name] = (pts.detach().cpu(), conf.detach().cpu(), grads)
    assert rel_err(res["hip"][0], res["ref"][0]) < 1e-4 and rel_err(res["hip"][1], res["ref"][1]) < 1e-4
    assert {k for k, v in res["hip"][2].items() if v is None} == {k for k, v in res["ref"][2].items() if v is None}
    worst = max((rel_err(res["hip"][2][k], v), k) for k, v in res["ref"][2].items() if v is not None)
    print("DPT head gradients: worst rel err %.2e (%s) over %d tensors" % (worst[0], worst[1], len(res["ref"][2])))
    assert worst[0] < 1.5e-5, worst          # measured 1.1e-6


def _synth_gts(n, B, H, W, seed, dtype, device):
    g = torch.Generator().manual_seed(seed)
    gts = []
    for i in range(n):
        Q, _ = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))
        pose = torch.eye(4).repeat(B, 1, 1)
        pose[:, :3, :3] = Q
        pose[:, :3, 3] = torch.randn(B, 3, generator=g) * 0.3
        pts = torch.randn(B, H, W, 3, generator=g) + torch.tensor([0.0, 0.0, 3.0])
        valid = torch.rand(B, H, W, generator=g) < 0.85
        gts.append(dict(pts3d=pts.to(dtype).to(device), valid_mask=valid.to(device), camera_pose=pose.to(dtype).to(device)))
    return gts


@pytest.mark.gpu
def test_training_step_gradients_match_oracle(tiny_sd):
    """A whole train-mode step on the tiny geometry (2 encoder / 10 decoder layers, full widths): Spann3R.forward in train mode
    (spann3r/model.py:473-539) -> ConfLoss_t -> backward, every kernel HIP, against float64 autograd through the oracle's
    forward + criterion: the loss and the gradient of EVERY parameter tensor."""
    from spann3r_amd import train as T, TINY
    from spann3r_amd.loss import ConfLoss_t, Regr3D_t, L21
    from spann3r_amd.weights import synth_frames
    from oracle import spann3r_oracle as O, loss_oracle as LO
    n, B, H, W = 3, 1, 32, 48
    frames = synth_frames(n, H, W, batch=B, seed=11)
    # hip
    P = {k: v.float().cuda().requires_grad_(True) for k, v in tiny_sd.items() if v.is_floating_point()}
    preds, preds_all = T.forward_train(P, [{"img": f["img"].cuda()} for f in frames], TINY)
    gts = _synth_gts(n, B, H, W, 5, torch.float32, "cuda")
    loss, details, factor = ConfLoss_t(Regr3D_t(L21, norm_mode="avg_dis", fix_first=False), alpha=0.4).compute_frame_loss(gts, preds_all)
    (loss + factor).backward()
    # oracle, float64
    P64 = {k: v.double().requires_grad_(True) for k, v in tiny_sd.items() if v.is_floating_point()}
    _, pa64 = O.forward.__wrapped__([{"img": f["img"].double()} for f in frames], P64, TINY, training_policy=True)
    l64, _, f64 = LO.conf_loss_t(_synth_gts(n, B, H, W, 5, torch.float64, "cpu"), pa64, 0.4, False)
    (l64 + f64).backward()
    assert abs(float(loss) + float(factor) - float(l64) - float(f64)) < 1e-4 * abs(float(l64))
    assert rel_err(preds_all[-1][1]["pts3d_in_other_view"].detach().cpu(), pa64[-1][1]["pts3d_in_other_view"].detach()) < 1e-4
    gmax = max(float(v.grad.abs().max()) for v in P64.values() if v.grad is not None)
    worst, n_checked, errs, num, den = (0.0, None), 0, [], 0.0, 0.0
    for k, v in P64.items():
        if v.grad is None:
            assert P[k].grad is None or float(P[k].grad.abs().max()) < 1e-6 * gmax, k
            continue
        d = P[k].grad.cpu().double() - v.grad
        e = float(d.abs().max()) / max(float(v.grad.abs().max()), 1e-4 * gmax)
        num, den = num + float((d ** 2).sum()), den + float((v.grad ** 2).sum())
        errs.append(e)
        n_checked += 1
        if e > worst[0]:
            worst = (e, k)
    errs.sort()
    print("training step: loss %.6f (oracle %.6f), %d parameter gradients, worst scaled error %.2e (%s), median %.2e, global rel. L2 %.2e" %
          (float(loss) + float(factor), float(l64) + float(f64), n_checked, worst[0], worst[1], errs[len(errs) // 2], (num / den) ** 0.5))
    # A convolution in front of a ReLU (head.2, the residual units) sums 1[pre-activation > 0] terms: a pre-activation within 1e-7 of
    # zero lands on either side under ANY fp32 rounding of the forward; one flipped unit moves entries of that weight gradient by ~1e-4
    # and everything upstream of it by ~1e-5 (measured with the flip: worst 9.8e-5, median 8.7e-6, global 1.2e-5; without: worst 5.5e-6).
    # The full-geometry test against the reference's own fp32 step is the tight one (global 8e-7).
    assert (num / den) ** 0.5 < 3e-5 and errs[len(errs) // 2] < 2e-5 and worst[0] < 4e-4, worst


@pytest.mark.gpu
def test_model_train_mode_runs_a_step(tiny_sd):
    """Spann3R in train mode (grad enabled, dropout active) records the HIP autograd forward; criterion + backward + the
    gradient reducer + an optimizer step run end to end and change the parameters"""
    from spann3r_amd import Spann3R, TINY
    from spann3r_amd.loss import ConfLoss_t, Regr3D_t, L21
    from spann3r_amd.runner import GradReducer
    from spann3r_amd.weights import synth_frames
    m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False)
    m.load_state_dict(tiny_sd, strict=True)
    m = m.cuda().train()
    n, B, H, W = 3, 1, 32, 48
    frames = [{"img": f["img"].cuda()} for f in synth_frames(n, H, W, batch=B, seed=3)]
    crit = ConfLoss_t(Regr3D_t(L21, norm_mode="avg_dis", fix_first=False), alpha=0.4)
    from spann3r_amd.train import AdamW
    opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05)
    preds, preds_all = m(frames)
    assert preds_all[0][0]["pts3d"].requires_grad and len(preds) == n
    loss, details, factor = crit.compute_frame_loss(_synth_gts(n, B, H, W, 5, torch.float32, "cuda"), preds_all)
    red = GradReducer(m.parameters(), overlap=True)
    red.prepare()
    (loss + factor).backward()
    red.finish()                                          # single process: no-op, same call sequence as the multi-GPU step
    w0 = m.state_dict()["dust3r.dec_blocks.0.mlp.fc1.weight"].clone()
    g = m.state_dict(keep_vars=True)["dust3r.dec_blocks.0.mlp.fc1.weight"].grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0
    opt.step()
    assert not torch.equal(m.state_dict()["dust3r.dec_blocks.0.mlp.fc1.weight"], w0)
    # the forward-only growing-bank policy is still what train() + mem_dropout.eval() selects
    m.mem_dropout.eval()
    with torch.no_grad():
        p2, _ = m(frames)
    assert not p2[0]["pts3d"].requires_grad


@pytest.mark.gpu
def test_train_mode_forward_without_grad_and_return_memory(tiny_sd):
    """spann3r/model.py:474-477,536-539 allow both: (a) model.train() under torch.no_grad() with ACTIVE memory dropout (a validation
    pass that leaves the model in train mode) -- the train-mode ops run without a tape; (b) return_memory=True in train mode -- the
    reference hands out its SpatialMemory (mem_k / mem_v / mem_attn / mem_count).  With dropout p = 0 the train-mode ops and the
    forward-only growing-bank runner (model.train() + mem_dropout.eval()) are the same function: outputs and memory must agree."""
    from spann3r_amd import Spann3R, TINY
    from spann3r_amd import train as T
    from spann3r_amd.weights import synth_frames
    m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False, memory_dropout=0.15)
    m.load_state_dict(tiny_sd, strict=True)
    m = m.cuda().train()
    T.set_precision("fp32")
    n, B, H, W = 4, 1, 32, 48
    frames = [{"img": f["img"].cuda()} for f in synth_frames(n, H, W, batch=B, seed=3)]
    with torch.no_grad():                                   # (a): dropout active, no tape
        preds, preds_all, mem = m(frames, return_memory=True)
    assert len(preds) == n and not preds[0]["pts3d"].requires_grad and torch.isfinite(preds[-1]["pts3d_in_other_view"]).all()
    P = (H // 16) * (W // 16)
    assert tuple(mem.mem_k.shape) == (B, (n - 1) * P, TINY.enc_dim) and tuple(mem.mem_attn.shape) == (B, (n - 1) * P, 1)
    # (b): p = 0 -> same function as the forward-only growing-bank policy
    m.mem_dropout.p = 0.0
    preds_t, _, mem_t = m(frames, return_memory=True)       # grad enabled: the training forward
    assert preds_t[0]["pts3d"].requires_grad
    m.mem_dropout.eval()
    with torch.no_grad():
        preds_f, _, mem_f = m(frames, return_memory=True)   # forward-only runner, train-mode memory policy
    for a, b in zip(preds_t, preds_f):
        for k in a:
            assert (a[k].detach() - b[k]).abs().max() <= 2e-4 * b[k].abs().max(), k
    for name in ("mem_k", "mem_v", "mem_attn"):
        x, y = getattr(mem_t, name).detach(), getattr(mem_f, name)
        assert (x - y).abs().max() <= 2e-4 * y.abs().max(), name
    assert torch.equal(mem_t.mem_count, mem_f.mem_count)
    # the read counts of the reference's add_mem: frame j of the bank has been read (n - 2 - j) times
    assert mem_t.mem_count[0, ::P, 0].tolist() == [float(n - 2 - j) for j in range(n - 1)]


@pytest.mark.gpu
def test_adamw_kernel_matches_torch():
    from spann3r_amd.train import AdamW
    g = torch.Generator().manual_seed(0)
    w0 = [torch.randn(257, 33, generator=g), torch.randn(1000, generator=g)]
    a = [torch.nn.Parameter(t.clone().cuda()) for t in w0]
    b = [torch.nn.Parameter(t.clone().double()) for t in w0]
    oa = AdamW(a, lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    ob = torch.optim.AdamW(b, lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    for it in range(4):
        for pa, pb in zip(a, b):
            gr = torch.randn(pa.shape, generator=g)
            pa.grad, pb.grad = gr.cuda(), gr.double()
        oa.step(); ob.step()
    for pa, pb in zip(a, b):
        assert rel_err(pa.detach().cpu(), pb.detach()) < 1e-6


# ------------------------------------------------------------------------------------------------- bf16 step, flat optimizer, RCCL
@pytest.mark.gpu
@pytest.mark.parametrize("R,C", [(784, 1024), (100, 200), (65, 4), (3, 130), (1568, 768)])
def test_pack_bf16_both_layouts(R, C):
    """sp3_pack_bf16 == the host-side fragment-order packing (ops.PackedAct.from_dense) of the bf16-rounded matrix and of its
    transpose, pads zero, for aligned and ragged shapes and a strided source"""
    from spann3r_amd import ops
    g = torch.Generator().manual_seed(R + C)
    big = torch.randn(R, C + 12, generator=g).cuda()
    x = big[:, 4:4 + C]                                     # row stride != cols, unaligned start unless C % 4 == 0 offsets agree
    a, t = ops.pack_bf16(x, True, True)
    ref = ops.PackedAct.from_dense(x.contiguous().to(torch.bfloat16))
    refT = ops.PackedAct.from_dense(x.t().contiguous().to(torch.bfloat16))
    assert torch.equal(a.data.view(-1), ref.data.view(-1))
    assert torch.equal(t.data.view(-1), refT.data.view(-1))
    only_t = ops.pack_bf16(x, False, True)
    assert only_t[0] is None and torch.equal(only_t[1].data.view(-1), refT.data.view(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("R,C", [(784, 768), (784, 3072), (100, 200), (3, 130), (8192, 64)])
def test_pack_bf16_column_sums_ride_along(R, C):
    """sp3_pack_bf16_colsum: the bias gradient dY.sum(0) from the pack launch's tile sums (+ a small fixed-order finish launch): equal to
    float64 within fp32 rounding, bit-identical across launches, accumulates"""
    from spann3r_amd import ops
    g = torch.Generator().manual_seed(R + C)
    x = torch.randn(R, C, generator=g).cuda()
    ref = x.double().sum(0).cpu()
    outs = []
    for rep in range(3):
        out = torch.full((C,), float("nan"), device="cuda")
        a, t = ops.pack_bf16(x, True, rep != 1, colsum=out)
        outs.append(out.clone())
    a0, _ = ops.pack_bf16(x, True, False)
    assert torch.equal(a.data, a0.data)
    assert rel_err(outs[0].cpu(), ref) < 2e-6
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    acc = torch.ones(C, device="cuda")
    ops.pack_bf16(x, True, False, colsum=acc, accumulate=True)
    assert torch.allclose(acc, outs[0] + 1.0, rtol=0, atol=1e-5 * float(outs[0].abs().max()))


@pytest.mark.gpu
def test_activation_on_load_matches_separate_launches():
    """bf16 mode: GELU in front of fc2 and ReLU in front of a 3x3 convolution applied by the consumer's pack launch (sp3_pack_bf16_act,
    sp3_pack_bf16_conv3x3 act) -- bit-identical values and gradients to the separate activation launches"""
    from spann3r_amd import train as T
    g = torch.Generator().manual_seed(3)
    C = 64
    P0 = {"m.fc1.weight": torch.randn(4 * C, C, generator=g) * 0.1, "m.fc1.bias": torch.randn(4 * C, generator=g) * 0.1,
          "m.fc2.weight": torch.randn(C, 4 * C, generator=g) * 0.1, "m.fc2.bias": torch.randn(C, generator=g) * 0.1,
          "r.conv1.weight": torch.randn(C, C, 3, 3, generator=g) * 0.05, "r.conv1.bias": torch.randn(C, generator=g) * 0.1,
          "r.conv2.weight": torch.randn(C, C, 3, 3, generator=g) * 0.05, "r.conv2.bias": torch.randn(C, generator=g) * 0.1}
    x0, m0, d0, e0 = torch.randn(2, 100, C, generator=g), torch.randn(2, 9, 11, C, generator=g), torch.randn(2, 100, C, generator=g), torch.randn(2, 9, 11, C, generator=g)
    res = {}
    T.set_precision("bf16")
    try:
        for on in (True, False):
            T.ACT_ON_LOAD = on
            T.invalidate_weight_cache()
            P = {k: v.cuda().requires_grad_(True) for k, v in P0.items()}
            x, m = x0.cuda().requires_grad_(True), m0.cuda().requires_grad_(True)
            y = T.mlp(x, P, "m.", res=x)
            z = T._rcu(m, P, "r.")
            y.backward(d0.cuda())
            z.backward(e0.cuda())
            res[on] = [y.detach(), z.detach(), x.grad, m.grad] + [P[k].grad for k in sorted(P)]
    finally:
        T.ACT_ON_LOAD = True
        T.set_precision("fp32")
        T.invalidate_weight_cache()
    assert all(torch.equal(a, b) for a, b in zip(res[True], res[False]))


@pytest.mark.gpu
@pytest.mark.parametrize("stride,geo", [(1, (2, 9, 7, 8, 12)), (2, (1, 14, 14, 64, 32)), (1, (2, 33, 20, 68, 256))])
def test_conv3x3_gather_in_the_pack_launch(stride, geo):
    """bf16 3x3 convolution: the im2col matrix gathered inside sp3_pack_bf16_conv3x3 gives the SAME fragment-order operands as
    sp3_im2col3x3 + sp3_pack_bf16, hence bit-identical outputs and gradients"""
    from spann3r_amd import train as T
    B, H, W, Cin, Cout = geo
    g = torch.Generator().manual_seed(H * W)
    x0, w0, b0 = torch.randn(B, H, W, Cin, generator=g), torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1, torch.randn(Cout, generator=g)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    r0, d0 = torch.randn(B, OH, OW, Cout, generator=g), torch.randn(B, OH, OW, Cout, generator=g)
    res = {}
    T.set_precision("bf16")
    try:
        for gather in (True, False):
            T.CONV_GATHER = gather
            T.invalidate_weight_cache()
            x, w, b, r = (t.cuda().requires_grad_(True) for t in (x0, w0, b0, r0))
            y = T.conv3x3(x, w, b, stride=stride, res=r)
            y.backward(d0.cuda())
            res[gather] = [y.detach(), x.grad, w.grad, b.grad, r.grad]
    finally:
        T.CONV_GATHER = True
        T.set_precision("fp32")
        T.invalidate_weight_cache()
    assert all(torch.equal(a, c) for a, c in zip(res[True], res[False]))
    ref = torch.nn.functional.conv2d(x0.permute(0, 3, 1, 2).double(), w0.double(), b0.double(), stride=stride, padding=1).permute(0, 2, 3, 1) + r0.double()
    assert rel_err(res[True][0].cpu(), ref) < 2e-2


@pytest.mark.gpu
@pytest.mark.parametrize("R,K,N", [(784, 1024, 3072), (196, 768, 768), (50, 200, 4), (1568, 864, 256)])
def test_linear_bf16_forward_backward(R, K, N):
    """the bf16 Linear (packed operands, no transposes): y, dX, dW, db against float64 on the bf16-rounded operands"""
    from spann3r_amd import train as T
    g = torch.Generator().manual_seed(R)
    x0, W0, b0, r0, d0 = torch.randn(R, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g), torch.randn(R, N, generator=g), torch.randn(R, N, generator=g)
    bf = lambda t: t.to(torch.bfloat16).double()
    T.set_precision("bf16")
    try:
        x, W, b = x0.cuda().requires_grad_(True), torch.nn.Parameter(W0.cuda()), b0.cuda().requires_grad_(True)
        y = T.linear(x, W, b, res=r0.cuda())
        y.backward(d0.cuda())
        y2 = T.linear(x.detach(), W, b.detach())            # second use: cached packed weights
    finally:
        T.set_precision("fp32")
        T.invalidate_weight_cache()
    yr = bf(x0) @ bf(W0).T + b0.double() + r0.double()
    assert rel_err(y.detach().cpu(), yr) < 1e-5
    assert rel_err(y2.cpu(), yr - r0.double()) < 1e-5
    assert rel_err(x.grad.cpu(), bf(d0) @ bf(W0)) < 1e-5
    assert rel_err(W.grad.cpu(), bf(d0).T @ bf(x0)) < 1e-5
    assert rel_err(b.grad.cpu(), d0.double().sum(0)) < 1e-5


@pytest.mark.gpu
def test_training_step_bf16_gradients(tiny_sd):
    """the whole train-mode step in bf16 mode (bf16 products, fp32 accumulate / master tensors) against float64 autograd through the
    oracle: loss within 2e-3; gradients: global relative L2 error and the median per-tensor scaled max error within 4e-2
    (measured on MI355X: 2.4e-2 / 2.0e-2 -- every GEMM operand of the ~40-layer forward AND backward chain is rounded to 8 mantissa
    bits, exactly what bf16 autocast does to the reference; the fp32 mode of the same code is held to 6e-5 above)"""
    from spann3r_amd import train as T, TINY
    from spann3r_amd.loss import ConfLoss_t, Regr3D_t, L21
    from spann3r_amd.weights import synth_frames
    from oracle import spann3r_oracle as O, loss_oracle as LO
    n, B, H, W = 3, 2, 32, 48
    frames = synth_frames(n, H, W, batch=B, seed=11)
    P = {k: v.float().cuda().requires_grad_(True) for k, v in tiny_sd.items() if v.is_floating_point()}
    T.set_precision("bf16")
    try:
        preds, preds_all = T.forward_train(P, [{"img": f["img"].cuda()} for f in frames], TINY)
        gts = _synth_gts(n, B, H, W, 5, torch.float32, "cuda")
        loss, details, factor = ConfLoss_t(Regr3D_t(L21, norm_mode="avg_dis", fix_first=False), alpha=0.4).compute_frame_loss(gts, preds_all)
        (loss + factor).backward()
    finally:
        T.set_precision("fp32")
        T.invalidate_weight_cache()
    P64 = {k: v.double().requires_grad_(True) for k, v in tiny_sd.items() if v.is_floating_point()}
    _, pa64 = O.forward.__wrapped__([{"img": f["img"].double()} for f in frames], P64, TINY, training_policy=True)
    l64, _, f64 = LO.conf_loss_t(_synth_gts(n, B, H, W, 5, torch.float64, "cpu"), pa64, 0.4, False)
    (l64 + f64).backward()
    assert abs(float(loss) + float(factor) - float(l64) - float(f64)) < 2e-3 * abs(float(l64))
    gmax = max(float(v.grad.abs().max()) for v in P64.values() if v.grad is not None)
    errs = []
    num = den = 0.0
    for k, v in P64.items():
        if v.grad is None:
            continue
        d = P[k].grad.cpu().double() - v.grad
        errs.append((float(d.abs().max()) / max(float(v.grad.abs().max()), 1e-3 * gmax), float(d.norm() / max(float(v.grad.norm()), 1e-30)), k))
        num += float(d.square().sum())
        den += float(v.grad.square().sum())
    errs.sort(reverse=True)
    med = errs[len(errs) // 2][0]
    print("bf16 training step: loss %.5f (oracle %.5f), %d gradients: global relative L2 error %.2e, median scaled max error %.2e, worst %s" %
          (float(loss) + float(factor), float(l64) + float(f64), len(errs), (num / den) ** 0.5, med, ["%.2e/%.2e %s" % e for e in errs[:6]]))
    assert (num / den) ** 0.5 < 4e-2 and med < 4e-2


@pytest.mark.gpu
def test_flat_adamw_and_clip_match_torch():
    """FlatAdamW on the GradReducer's flat buckets == torch.optim.AdamW + clip_grad_norm_ (float64) over several steps: two
    parameter groups (decay / no decay), a changing lr, gradient scaling, the returned norm; parameters stay views of the flat
    buffers and gradients accumulate in place"""
    from spann3r_amd import train as T
    from spann3r_amd.runner import GradReducer
    g = torch.Generator().manual_seed(0)
    shapes = [(257, 33), (1000,), (64, 64), (5,), (3000, 7)]
    w0 = [torch.randn(*s, generator=g) for s in shapes]
    a = [torch.nn.Parameter(t.clone().cuda()) for t in w0]
    b = [torch.nn.Parameter(t.clone().double()) for t in w0]
    red = GradReducer(a, bucket_mb=0.05)
    assert len(red.buckets) >= 2
    groups = lambda ps: [{"params": [p for p in ps if p.dim() == 1], "weight_decay": 0.0}, {"params": [p for p in ps if p.dim() > 1], "weight_decay": 0.05}]
    oa = T.FlatAdamW(groups(a), red, lr=3e-3, betas=(0.9, 0.95), eps=1e-8)
    ob = torch.optim.AdamW(groups(b), lr=3e-3, betas=(0.9, 0.95), eps=1e-8)
    for (flat, items) in red.flat_buffers():
        for p, o in items:
            assert p.grad.data_ptr() == flat.data_ptr() + 4 * o
    for it in range(5):
        oa.zero_grad()
        ob.zero_grad()
        scale = 0.5 if it % 2 else 1.0
        for pa, pb in zip(a, b):
            gr = torch.randn(pa.shape, generator=g) * (3.0 if it < 3 else 0.01)      # clipped steps and unclipped ones
            pa.grad.add_(gr.cuda())                       # accumulates into the bucket view, as autograd does
            pb.grad = gr.double() * scale
        for grp_a, grp_b in zip(oa.param_groups, ob.param_groups):
            grp_a["lr"] = grp_b["lr"] = 3e-3 * (1.0 - 0.1 * it)
        norm_b = torch.nn.utils.clip_grad_norm_(b, 1.0)
        norm_a = oa.step(grad_scale=scale, max_norm=1.0)
        ob.step()
        assert abs(float(norm_a) - float(norm_b)) < 1e-5 * float(norm_b)
    for pa, pb in zip(a, b):
        assert rel_err(pa.detach().cpu(), pb.detach()) < 2e-6
    # a skipped parameter (no gradient on any rank) is left alone
    before = [p.detach().clone() for p in a]
    oa.step(skip=[a[1]])
    assert torch.equal(a[1].detach(), before[1]) and not torch.equal(a[0].detach(), before[0])


@pytest.mark.gpu
def test_rccl_gradient_all_reduce_runs_on_the_device(tiny_sd):
    """RCCL on the GPU (one rank, collectives forced): the bucket all-reduces are launched from inside backward by the
    post-accumulate-grad hooks, in bucket order, on flat gradient buffers; a whole TrainStep (forward, ConfLoss, backward,
    all-reduce, clip, AdamW) runs on top and changes the parameters"""
    import torch.distributed as dist
    from spann3r_amd import Spann3R, TINY
    from spann3r_amd import train as T
    from spann3r_amd.weights import synth_frames
    own = not dist.is_initialized()
    if own:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29617")
        dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False)
        m.load_state_dict(tiny_sd, strict=True)
        m = m.cuda()
        m.mem_dropout.p = 0.0                               # (keeps the two runs below comparable)
        ts = T.TrainStep(m, precision="bf16", bucket_mb=4.0, force_collectives=True)
        assert ts.reducer.active() and len(ts.reducer.buckets) >= 3
        n, B, H, W = 3, 2, 32, 48
        frames = [{"img": f["img"].cuda()} for f in synth_frames(n, H, W, batch=B, seed=3)]
        gts = _synth_gts(n, B, H, W, 5, torch.float32, "cuda")
        w0 = m.state_dict()["dust3r.dec_blocks.0.mlp.fc1.weight"].clone()
        l0, n0 = ts.run(frames, gts)
        assert ts.reducer.launched_in_backward >= 1          # collectives started while backward was still running
        torch.cuda.synchronize()
        assert torch.isfinite(l0) and torch.isfinite(n0) and float(n0) > 0
        w1 = m.state_dict()["dust3r.dec_blocks.0.mlp.fc1.weight"].clone()
        assert not torch.equal(w1, w0)
        # the same step without collectives lands on the same parameters bit for bit: a one-rank all-reduce is the identity
        T.invalidate_weight_cache()
        m2 = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False)
        m2.load_state_dict(tiny_sd, strict=True)
        torch.manual_seed(0)
        ts2 = T.TrainStep(m2.cuda(), precision="bf16", bucket_mb=4.0)
        assert not ts2.reducer.active()
        m2.mem_dropout.p = 0.0
        l2, n2 = ts2.run(frames, gts)
        assert float(l2) == float(l0) and torch.equal(m2.state_dict()["dust3r.dec_blocks.0.mlp.fc1.weight"], w1)
        # world 1: the averaged gradient is the local one
        g = torch.randn(1000, device="cuda")
        p = torch.nn.Parameter(torch.zeros(1000, device="cuda"))
        from spann3r_amd.runner import GradReducer
        r = GradReducer([p], force=True)
        p.grad.copy_(g)
        r.reduce()
        assert torch.equal(p.grad, g)
    finally:
        T.set_precision("fp32")
        T.invalidate_weight_cache()
        if own:
            dist.destroy_process_group()


@pytest.mark.gpu
def test_train_step_hip_graph_replay_matches_eager(tiny_sd):
    """TrainStep(graph=True): the captured step (forward, ConfLoss, backward, clip, AdamW with device-side step count / lr) replayed
    on new batches follows the same parameter trajectory as the eager step (dropout off to make the two runs comparable)"""
    from spann3r_amd import Spann3R, TINY
    from spann3r_amd import train as T
    from spann3r_amd.weights import synth_frames
    n, B, H, W = 3, 2, 32, 48
    batches = [([{"img": f["img"].cuda()} for f in synth_frames(n, H, W, batch=B, seed=30 + i)], _synth_gts(n, B, H, W, 40 + i, torch.float32, "cuda")) for i in range(3)]
    traj = {}
    try:
        for mode in (False, True):
            m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False, memory_dropout=0.0)
            m.load_state_dict(tiny_sd, strict=True)
            ts = T.TrainStep(m.cuda(), precision="fp32", lr=1e-4, graph=mode)
            out = []
            for i, (fr, gt) in enumerate(batches):
                ts.set_lr(1e-4 * (1 + i))
                loss, norm = ts.run(fr, gt)
                out.append((float(loss), float(norm)))
            traj[mode] = (out, m.state_dict()["dust3r.dec_blocks.1.attn.qkv.weight"].clone(), ts.opt.step_count)
            del ts, m
    finally:
        T.set_precision("fp32")
        T.invalidate_weight_cache()
    # warm-up and capture are undone (parameters, moments, step count restored): replay i is update i of the same trajectory
    assert all(map(lambda t: t[0] == t[0] and t[1] > 0, traj[True][0]))
    assert abs(traj[True][0][1][0] - traj[True][0][2][0]) > 0            # different batches -> different losses: inputs are refreshed
    assert not torch.equal(traj[True][1], tiny_sd["dust3r.dec_blocks.1.attn.qkv.weight"].cuda())
    assert traj[True][2] == traj[False][2] == len(batches)               # host-side step count follows the replays
    for (le, ne), (lg, ng) in zip(traj[False][0], traj[True][0]):
        assert abs(le - lg) <= 1e-5 * abs(le) and abs(ne - ng) <= 1e-4 * abs(ne), (traj[False][0], traj[True][0])
    we, wg = traj[False][1].double(), traj[True][1].double()
    assert float((we - wg).abs().max() / (we - tiny_sd["dust3r.dec_blocks.1.attn.qkv.weight"].cuda().double()).abs().max()) < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_inference_after_training_sees_the_new_weights(tiny_sd, graph):
    """An Engine built before training must not survive an optimizer step (FlatAdamW re-points .data and, under a hipGraph,
    never touches the version counters): eval forward after TrainStep == eval forward of a fresh model with the trained weights"""
    from spann3r_amd import Spann3R, TINY
    from spann3r_amd import train as T
    from spann3r_amd.weights import synth_frames
    n, B, H, W = 3, 1, 32, 48
    fr = [{"img": f["img"].cuda()} for f in synth_frames(n, H, W, batch=B, seed=3)]
    gt = _synth_gts(n, B, H, W, 41, torch.float32, "cuda")
    try:
        m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False, memory_dropout=0.0)
        m.load_state_dict(tiny_sd, strict=True)
        m = m.cuda().eval()
        with torch.no_grad():
            before = m(fr)[0][0]["pts3d"].clone()                        # builds (and caches) the inference engine
        ts = T.TrainStep(m, precision="fp32", lr=1e-4, graph=graph)
        for _ in range(2):
            ts.run(fr, gt)
        m.eval()
        with torch.no_grad():
            after = m(fr)[0][0]["pts3d"].clone()
        fresh = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False, memory_dropout=0.0)
        fresh.load_state_dict({k: v.clone() for k, v in m.state_dict().items()}, strict=True)
        with torch.no_grad():
            want = fresh.cuda().eval()(fr)[0][0]["pts3d"]
        assert bool(torch.isfinite(after).all())
        assert not torch.equal(before, after), "eval forward still runs on the pre-training weights"
        assert rel_err(after.cpu(), want.cpu()) < 1e-6
    finally:
        T.set_precision("fp32")
        T.invalidate_weight_cache()


@pytest.mark.gpu
def test_graph_captured_at_lr_zero_follows_set_lr(tiny_sd):
    """the reference's warm-up starts at lr = 0 (croco/utils/misc.py:464-479): a step captured there must still move the weights
    once set_lr raises the rate (chunk tables hold the groups' lr SCALE, not lr / lr0)"""
    from spann3r_amd import Spann3R, TINY
    from spann3r_amd import train as T
    from spann3r_amd.weights import synth_frames
    n, B, H, W = 3, 1, 32, 48
    fr = [{"img": f["img"].cuda()} for f in synth_frames(n, H, W, batch=B, seed=3)]
    gt = _synth_gts(n, B, H, W, 41, torch.float32, "cuda")
    try:
        m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False, memory_dropout=0.0)
        m.load_state_dict(tiny_sd, strict=True)
        ts = T.TrainStep(m.cuda(), precision="fp32", lr=0.0, graph=True)
        key = "dust3r.dec_blocks.1.attn.qkv.weight"
        ts.run(fr, gt)
        w0 = m.state_dict()[key].clone()
        assert torch.equal(w0, tiny_sd[key].cuda())                      # lr = 0: nothing moves
        ts.set_lr(1e-4)
        ts.run(fr, gt)
        assert not torch.equal(m.state_dict()[key], w0)
    finally:
        T.set_precision("fp32")
        T.invalidate_weight_cache()


@pytest.mark.gpu
def test_weight_cache_is_bounded_and_refreshed():
    """bf16 packed-weight cache: one entry per (weight, derivation); train.AdamW (raw-pointer update) and torch optimizers
    (version bump) both lead to a re-pack, neither grows the cache"""
    from spann3r_amd import train as T
    try:
        T.set_precision("bf16")
        T.invalidate_weight_cache()
        W = torch.nn.Parameter(torch.randn(64, 128, device="cuda") * 0.1)
        x = torch.randn(32, 128, device="cuda")
        for opt in (T.AdamW([W], lr=1e-1), torch.optim.SGD([W], lr=1e-1)):
            outs = []
            for _ in range(4):
                y = T.linear(x, W)
                outs.append(y.detach().clone())
                y.square().mean().backward()
                opt.step()
                opt.zero_grad(set_to_none=True)
            assert len(T._wcache) <= 1
            ref = x.to(torch.bfloat16).double() @ W.detach().to(torch.bfloat16).double().T
            assert rel_err(T.linear(x, W).detach().cpu(), ref.cpu()) < 1e-5     # the product uses the CURRENT weights
            assert not torch.equal(outs[0], outs[-1])
    finally:
        T.set_precision("fp32")
        T.invalidate_weight_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("precision,flash,tol", [("fp32", False, 2e-5), ("fp32", True, 2e-5), ("bf16", True, 3e-2)])
def test_full_geometry_gradients_vs_reference_step(full_sd, precision, flash, tol):
    """BASELINE config 5's step at FULL depth and width (24 encoder / 12 decoder layers, ViT-L / ViT-B / DPT) against ONE TRAINING
    STEP OF THE UNMODIFIED REFERENCE (torch CPU float32, tests/golden/make_golden.py traingrad: Spann3R.forward in train mode +
    spann3r/loss.py ConfLoss_t + backward): the loss and a strided sample of EVERY parameter gradient (~1090 tensors).
    fp32 mode, attention materialised (S, softmax, P.V as the reference computes them): global relative L2 error of the sampled
    gradients within 2e-5 (measured 3.2e-6) and every tensor within 2e-3 of the reference scaled by the tensor's own maximum
    (measured worst 3.1e-4, a bias = a sum over 10^4 pixels: both sides carry fp32 rounding through ~80 chained GEMMs and
    differently ordered sums);
    fp32 mode, flash attention (the default): within 2e-5 (measured 8.3e-7, worst tensor 4.0e-6) -- with RoPE angles taken from the
    reference's own fp32 tables; with angles computed to full precision in the kernel the same run measured 3.2e-5 (worst 8.4e-4 on a
    ReLU-gated convolution): parity with an fp32 reference means repeating its rounded constants, not improving on them;
    bf16 mode: global relative L2 error within 3e-2 (measured 8.0e-3: operand rounding of ~80 chained GEMMs)."""
    import numpy as np
    from spann3r_amd import train as T, FULL
    from spann3r_amd.loss import ConfLoss_t, Regr3D_t, L21
    from spann3r_amd.weights import synth_frames, state_dict_fingerprint, alias_of
    path = os.path.join(os.path.dirname(__file__), "golden", "train_grad_full.npz")
    if not os.path.exists(path):
        pytest.skip("fixture not generated (tests/golden/make_golden.py traingrad)")
    g = np.load(path)
    assert state_dict_fingerprint(full_sd) == float(g["fingerprint"])
    H, W, NF, B, fseed, _ = (int(v) for v in g["meta"])
    frames = [{"img": f["img"].cuda()} for f in synth_frames(NF, H, W, batch=B, seed=fseed)]
    gts = [dict(pts3d=torch.from_numpy(g["gt_pts3d"][i]).float().cuda(), valid_mask=torch.from_numpy(g["gt_valid_mask"][i]).cuda(),
                camera_pose=torch.from_numpy(g["gt_camera_pose"][i]).float().cuda()) for i in range(NF)]
    P = {k: v.float().cuda().requires_grad_(True) for k, v in full_sd.items() if v.is_floating_point()}
    T.set_precision(precision)
    T.FLASH_ATTENTION = flash
    try:
        preds, preds_all = T.forward_train(P, frames, FULL, dropout_p=0.0)
        loss, details, factor = ConfLoss_t(Regr3D_t(L21, norm_mode="avg_dis", fix_first=False), alpha=0.4).compute_frame_loss(gts, preds_all)
        (loss + factor).backward()
    finally:
        T.set_precision("fp32")
        T.FLASH_ATTENTION = True
        T.invalidate_weight_cache()
    ref_total = float(g["loss"]) + float(g["factor"])
    assert abs(float(loss) + float(factor) - ref_total) < (1e-4 if precision == "fp32" else 5e-3) * abs(ref_total)
    names = [str(n) for n in g["names"]]
    gmax = max(float(g["g_" + n + "_max"]) for n in names)
    worst, num, den, contrib = (0.0, None), 0.0, 0.0, []
    for n in names:
        p = P.get(n)
        if p is None or p.grad is None:
            other = [k for k in P if alias_of(k) == n or alias_of(n) == k]
            p = next((P[k] for k in other if P[k].grad is not None), None)
        assert p is not None and p.grad is not None, n
        step = int(g["g_" + n + "_step"])
        mine = p.grad.reshape(-1)[::step][:256].double().cpu().numpy()
        ref = g["g_" + n + "_sample"]
        d = np.abs(mine - ref)
        e = float(d.max()) / max(float(g["g_" + n + "_max"]), 1e-4 * gmax)
        num, den = num + float((d ** 2).sum()), den + float((ref ** 2).sum())
        contrib.append((float((d ** 2).sum()), float((ref ** 2).sum()), n))
        worst = max(worst, (e, n))
    print("largest error contributions:", ["%s %.1e of %.1e" % (n, a, b) for a, b, n in sorted(contrib, reverse=True)[:6]])
    print("full-geometry step (%s): loss %.6f (reference %.6f), %d gradient tensors sampled, worst scaled error %.2e (%s), global rel. L2 %.2e"
          % (precision, float(loss) + float(factor), ref_total, len(names), worst[0], worst[1], (num / den) ** 0.5))
    assert len(names) > 1000
    assert (num / den) ** 0.5 < tol
    if precision == "fp32":
        assert worst[0] < 2e-3, worst


@pytest.mark.gpu
def test_train_forward_mixed_orientation_batch(tiny_sd):
    """Training batches mix landscape samples and portraits rotated to landscape (spann3r/training.py:216,
    dust3r/utils/misc.py:80-94): the train-mode forward of a mixed batch equals the per-sample forwards in their own orientation
    (samples of a batch are independent), and gradients flow through both head passes."""
    from spann3r_amd import Spann3R, TINY
    from spann3r_amd import train as T
    from spann3r_amd.weights import synth_frames
    n, H, W = 3, 32, 48
    try:
        T.set_precision("fp32")
        m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False, memory_dropout=0.0)
        m.load_state_dict(tiny_sd, strict=True)
        m = m.cuda().train()
        base = synth_frames(n, H, W, batch=2, seed=5)
        ts = torch.tensor([(H, W), (W, H)], dtype=torch.int32)
        mixed = [{"img": f["img"].cuda(), "true_shape": ts} for f in base]
        preds, _ = m(mixed)
        singles = []
        for b in range(2):
            fr = [{"img": f["img"][b:b + 1].cuda(), "true_shape": ts[b:b + 1]} for f in base]
            singles.append(m(fr)[0])
        for j, p in enumerate(preds):
            for k in p:
                for b in range(2):
                    assert rel_err(p[k][b].detach().cpu(), singles[b][j][k][0].detach().cpu()) < 1e-5, (j, k, b)
        loss = sum(p[k].square().mean() for p in preds for k in p)
        loss.backward()
        gnorm = sum(float(q.grad.abs().sum()) for q in m.parameters() if q.grad is not None)
        assert gnorm > 0 and gnorm == gnorm
    finally:
        T.set_precision("fp32")
        T.invalidate_weight_cache()


@pytest.mark.gpu
def test_captured_step_with_rccl_collectives_matches_eager(tiny_sd):
    """TrainStep(graph=True) with a process group up (one rank, collectives forced): the bucket all-reduces are captured INTO the
    step's hipGraph (no silent fall-back to the eager step) and the replayed trajectory equals the eager one."""
    import torch.distributed as dist
    from spann3r_amd import Spann3R, TINY
    from spann3r_amd import train as T
    from spann3r_amd.weights import synth_frames
    own = not dist.is_initialized()
    if own:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29619")
        dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        n, B, H, W = 3, 2, 32, 48
        batches = [([{"img": f["img"].cuda()} for f in synth_frames(n, H, W, batch=B, seed=30 + i)], _synth_gts(n, B, H, W, 40 + i, torch.float32, "cuda")) for i in range(3)]
        traj = {}
        for mode in (False, True):
            m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False, memory_dropout=0.0)
            m.load_state_dict(tiny_sd, strict=True)
            ts = T.TrainStep(m.cuda(), precision="fp32", lr=1e-4, graph=mode, bucket_mb=4.0, force_collectives=True)
            assert ts.reducer.active() and bool(ts.graph) == mode
            out = []
            for fr, gt in batches:
                loss, norm = ts.run(fr, gt)
                out.append((float(loss), float(norm)))
            traj[mode] = (out, m.state_dict()["dust3r.dec_blocks.1.attn.qkv.weight"].clone())
            del ts, m
            T.invalidate_weight_cache()
        for (le, ne), (lg, ng) in zip(traj[False][0], traj[True][0]):
            assert abs(le - lg) <= 1e-5 * abs(le) and abs(ne - ng) <= 1e-4 * abs(ne), traj
        we, wg = traj[False][1].double(), traj[True][1].double()
        assert float((we - wg).abs().max() / (we - tiny_sd["dust3r.dec_blocks.1.attn.qkv.weight"].cuda().double()).abs().max()) < 1e-3
    finally:
        T.set_precision("fp32")
        T.invalidate_weight_cache()
        if own:
            dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True])
def test_training_loop_vs_reference_train_one_epoch(tiny_sd, graph):
    """The loop around the step -- gradient accumulation over accum_iter = 2 iterations, the per-iteration learning-rate hook (warm-up
    from lr 0, then the cosine branch), clip + AdamW every second iteration, parameters without a gradient passed over -- against the
    reference's UNMODIFIED train_one_epoch run for two epochs of 4 iterations (tests/golden/make_golden.py trainloop: losses,
    learning rates, gradient norms per iteration and a strided sample of every parameter after each epoch).  Eager and captured
    (one hipGraph per position in the accumulation window)."""
    import argparse
    from conftest import load_golden
    from spann3r_amd import Spann3R, TINY
    from spann3r_amd import train as T
    from spann3r_amd.weights import synth_frames, state_dict_fingerprint
    g = load_golden("train_loop_tiny.npz")
    H, W, NF, B, NIT, NEP, _, seed0 = map(int, g["meta"])
    assert state_dict_fingerprint(tiny_sd) == float(g["fingerprint"])
    a = g["args"]
    args = argparse.Namespace(accum_iter=int(a[0]), epochs=int(a[1]), warmup_epochs=int(a[2]), lr=float(a[3]), min_lr=float(a[4]))
    batches = []
    for i in range(NIT * NEP):
        valid = np.unpackbits(g["gt%d_valid" % i])[:NF * B * H * W].reshape(NF, B, H, W).astype(bool)
        views = []
        for j, f in enumerate(synth_frames(NF, H, W, batch=B, seed=seed0 + i)):
            views.append({"img": f["img"].cuda(), "true_shape": torch.tensor([[H, W]] * B, dtype=torch.int32),
                          "pts3d": torch.from_numpy(g["gt%d_pts3d" % i][j]).cuda(), "valid_mask": torch.from_numpy(valid[j]).cuda(),
                          "camera_pose": torch.from_numpy(g["gt%d_pose" % i][j]).cuda()})
        batches.append(views)
    rec = []
    try:
        m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False, memory_dropout=0.0)
        m.load_state_dict(tiny_sd, strict=True)
        m = m.cuda()
        ts = T.TrainStep(m, precision="fp32", lr=args.lr, weight_decay=float(a[5]), accum_iter=args.accum_iter, graph=graph)
        params = dict(m.named_parameters())
        for ep in range(NEP):
            stats = T.train_one_epoch(ts, batches[ep * NIT:(ep + 1) * NIT], ep, args, on_iteration=lambda *r: rec.append(r))
            assert stats["loss"] == stats["loss"]
            # Adam's first updates are +-lr per element whatever the gradient's size, so an element whose accumulated gradient is
            # rounding noise (softmax-invariant directions: norm_k.bias, the k third of every qkv bias, ...) moves by an arbitrary
            # amount up to the sum of the learning rates on either machine.  The comparison is therefore a distribution over all
            # sampled elements of |p - p_ref| in units of that sum: the bulk must agree closely, outliers must be rare (the
            # per-iteration losses and gradient norms below pin the trajectory as a whole).
            lr_sum = float(np.sum(g["it_lr"][1:(ep + 1) * NIT:args.accum_iter]))
            errs, names_of = [], []
            untouched = set(map(str, g["untouched"]))
            for name in g["names"]:
                name = str(name)
                flat = params[name].detach().reshape(-1)
                step = max(1, flat.numel() // 64)
                mine = flat[::step][:64].double().cpu().numpy()
                ref, init = g["p%d_%s" % (ep, name)], tiny_sd[name].reshape(-1)[::step][:64].double().numpy()
                if name in untouched:
                    assert np.array_equal(mine, init), name                  # no gradient: not even weight decay (AdamW passes over it)
                    assert np.array_equal(ref, init), name
                    continue
                errs.append(np.abs(mine - ref) / lr_sum)
                names_of += [name] * len(mine)
            errs = np.concatenate(errs)
            p50, p95, p99 = np.percentile(errs, [50, 95, 99])
            out_frac = float((errs > 0.5).mean())
            bad = sorted({names_of[k] for k in np.nonzero(errs > 0.5)[0]})
            print("epoch %d (graph=%s): |p - p_ref| / sum(lr) over %d elements: median %.2e p95 %.2e p99 %.2e max %.2e; %.3f%% beyond 0.5: %s"
                  % (ep, graph, errs.size, p50, p95, p99, errs.max(), 100 * out_frac, bad[:12]))
            # measured: median <= 7e-5, p95 5e-4, p99 1.2e-3, max 2.1e-2 of the summed learning rates, no outlier
            assert p50 < 1e-3 and p95 < 5e-3 and out_frac < 1e-3, (ep, p50, p95, out_frac)
        if graph:
            assert sorted(ts._graphs) == [(False, True), (True, False)]          # one graph per position in the window
        assert ts.opt.step_count == NIT * NEP // args.accum_iter
    finally:
        T.set_precision("fp32")
        T.invalidate_weight_cache()
    assert len(rec) == NIT * NEP
    for i, (it, loss, norm, lr) in enumerate(rec):
        assert abs(lr - g["it_lr"][i]) <= 1e-12 + 1e-9 * abs(g["it_lr"][i]), (i, lr, g["it_lr"][i])
        assert abs(loss - g["it_loss"][i]) <= 2e-3 * abs(g["it_loss"][i]), (i, loss, g["it_loss"][i])
        if np.isnan(g["it_norm"][i]):
            assert norm is None                                                  # update_grad=False iterations return no norm
        else:
            assert abs(norm - g["it_norm"][i]) <= 2e-3 * g["it_norm"][i], (i, norm, g["it_norm"][i])
    print("losses", [round(r[1], 4) for r in rec], "ref", np.round(g["it_loss"], 4).tolist())
