"""Streaming sessions (spann3r_amd/stream.py) on an MI355X: frames pushed one at a time must give, bit for bit, what Spann3R.forward
returns for every prefix under the frame-by-frame schedule (batch_encode = False) -- the streaming step launches the same kernels at
the same shapes -- and stay within the project's bars of the default schedule and of the reference dump.
TINY config, 48 x 64 frames (3 x 4 = 12 tokens)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FP32 = 1e-3          # as tests/test_model_gpu.py::test_tiny_forward_vs_golden
TOL_BF16 = 3e-2
TOL_SCHEDULE = 2e-5      # whole-sequence encoder against per-frame, tests/test_model_gpu.py::test_batched_encoder_equals_per_frame


def make_model(tiny_sd, precision):
    from spann3r_amd import Spann3R, TINY
    m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False)
    m.load_state_dict(tiny_sd, strict=True)
    return m.to(DEV).eval().set_precision(precision)


@pytest.fixture(scope="module")
def models(tiny_sd):
    cache = {}

    def get(precision):
        if precision not in cache:
            cache[precision] = make_model(tiny_sd, precision)
        return cache[precision]
    yield get
    cache.clear()


def to_dev(frames):
    return [{k: (v.to(DEV) if k == "img" else v) for k, v in f.items()} for f in frames]


def frames_of(n, seed, batch=1):
    from spann3r_amd.weights import synth_frames
    return to_dev(synth_frames(n, 48, 64, batch=batch, seed=seed))


def forward_per_frame(m, frames):
    """forward under the frame-by-frame schedule: the reference of the bit-for-bit contract"""
    m.batch_encode = False
    try:
        return m(frames, return_memory=True)
    finally:
        m.batch_encode = True


def push_all(s, frames):
    steps = [s.push(f) for f in frames]
    assert steps[0] is None and all(st is not None for st in steps[1:])
    return steps[1:]


def preds_of(steps):
    return [st.final for st in steps] + [steps[-1].latest], [st.pair for st in steps]


def assert_same_preds(got, ref, what=""):
    (gp, gpa), (rp, rpa) = got, ref
    assert len(gp) == len(rp) and len(gpa) == len(rpa)
    for j, (a, b) in enumerate(zip(gp, rp)):
        assert set(a) == set(b) == {"pts3d" if j == 0 else "pts3d_in_other_view", "conf"}, (what, j, set(a), set(b))
        for k in a:
            assert torch.equal(a[k], b[k]), (what, "preds", j, k)
    for j, (a, b) in enumerate(zip(gpa, rpa)):
        for side in (0, 1):
            assert set(a[side]) == set(b[side]), (what, j, side)
            for k in a[side]:
                assert torch.equal(a[side][k], b[side][k]), (what, "preds_all", j, side, k)


def assert_same_memory(a, b, what=""):
    for name in ("mem_k", "mem_v", "mem_attn", "mem_count"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
    assert (a.M, a.wm, a.lm, a.events) == (b.M, b.wm, b.lm, b.events), (what, (a.M, a.wm, a.lm, a.events), (b.M, b.wm, b.lm, b.events))


# ----------------------------------------------------------------------------- 1. the prefix contract
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_stream_equals_forward_of_every_prefix(models, precision):
    """n = 8: the working memory (5 frames) fills and hands over to long-term.  k = 2: the first step alone; k = 3: the first
    streaming-kind step with the first memory read; k = 8: the working memory overflowing."""
    m = models(precision)
    frames = frames_of(8, seed=7)
    refs = {k: forward_per_frame(m, frames[:k]) for k in (2, 3, 8)}
    with m.stream() as s:
        steps = []
        for t, f in enumerate(frames):
            st = s.push(f)
            assert s.n_frames == t + 1
            if t == 0:
                assert st is None
                continue
            steps.append(st)
            assert st.index == t and st.pair[0] is st.final and st.pair[1] is st.latest
            k = t + 1
            if k in refs:
                got_mem, ref = s.memory(), refs[k]
                assert_same_preds(preds_of(steps), ref[:2], "k=%d" % k)
                assert_same_memory(got_mem, ref[2], "k=%d" % k)
                assert ref[0][0] is ref[1][0][0]
        assert s.memory().wm == 5 and s.memory().lm > 0


# ----------------------------------------------------------------------------- 2. default schedule, reference dump
def test_stream_vs_default_schedule_fp32(tiny_sd):
    m = make_model(tiny_sd, "fp32")                                  # (the shared models only ever run the frame-by-frame schedule)
    frames = frames_of(8, seed=7)
    ref = m(frames, return_memory=True)                              # whole-sequence encoder, deferred head
    with m.stream() as s:
        got = preds_of(push_all(s, frames))
        mem = s.memory()
    worst = 0.0
    for a, b in zip(got[0], ref[0]):
        assert set(a) == set(b)
        worst = max([worst] + [rel_err(a[k].cpu(), b[k].cpu()) for k in a])
    print("stream vs default schedule (fp32): worst rel err %.2e" % worst)
    assert worst < TOL_SCHEDULE
    assert (mem.M, mem.wm) == (ref[2].M, ref[2].wm)


@pytest.mark.parametrize("precision,tol", [("fp32", TOL_FP32), ("bf16", TOL_BF16)])
def test_stream_vs_golden(models, precision, tol):
    from spann3r_amd.weights import synth_frames
    g = load_golden("spann3r_tiny.npz")
    H, W = map(int, g["meta_hw"])
    m = models(precision)
    frames = to_dev(synth_frames(int(g["meta_frames"]), H, W))
    with m.stream() as s:
        preds, _ = preds_of(push_all(s, frames))
        mem = s.memory()
    assert len(preds) == len(frames)
    worst = 0.0
    for j, p in enumerate(preds):
        key = "pts3d" if j == 0 else "pts3d_in_other_view"
        assert set(p.keys()) == {key, "conf"}
        assert p[key].dtype == torch.float32 and tuple(p[key].shape) == (1, H, W, 3)
        worst = max(worst, rel_err(p[key].cpu(), g["pred%d_pts" % j]), rel_err(p["conf"].cpu(), g["pred%d_conf" % j]))
    print("stream vs golden %s: worst rel err %.3e" % (precision, worst))
    assert worst < tol
    if precision == "fp32":
        assert rel_err(mem.mem_k.cpu(), g["mem_k"]) < tol and rel_err(mem.mem_v.cpu(), g["mem_v"]) < tol
        assert np.array_equal(mem.mem_count.cpu().numpy(), g["mem_count"])
        assert rel_err(mem.mem_attn.cpu(), g["mem_attn"]) < tol
        assert [mem.wm, mem.lm] == list(g["mem_wm_lm"])


# ----------------------------------------------------------------------------- 3. graphs
def test_stream_graphs_bounded_and_equal_eager(models):
    m = models("bf16")
    frames = frames_of(18, seed=11)
    m.use_graphs = False
    try:
        with m.stream() as s:
            eager = preds_of(push_all(s, frames))
            eager_mem = s.memory()
            assert len(s._run.graphs) == 0 and s.replays == 0
    finally:
        m.use_graphs = True
    with m.stream() as s:
        steps = push_all(s, frames[:12])
        run = s._run
        assert run.mem.state is not None
        held = [k for k in run.graphs if k[0] == "whole"]
        assert 1 <= len(held) <= 3, held                             # the bound of test_one_step_graph_serves_a_growing_bank
        steps += [s.push(f) for f in frames[12:]]
        assert len([k for k in run.graphs if k[0] == "whole"]) == len(held) and len(run.graphs) == len(held)
        assert s.replays >= 15
        assert_same_preds(preds_of(steps), eager, "graphs vs eager")
        assert_same_memory(s.memory(), eager_mem, "graphs vs eager")
        # a new sequence on the same buffers and graphs: every streaming step replays, nothing is captured
        keys = list(run.graphs)
        s.reset()
        assert s.n_frames == 0
        again = []
        for t, f in enumerate(frames):
            st = s.push(f)
            if t >= 2:
                assert run.graphs.last == "replay", t
            if t >= 1:
                again.append(st)
        assert s._run is run and list(run.graphs) == keys
        assert_same_preds(preds_of(again), eager, "after reset")
        assert_same_memory(s.memory(), eager_mem, "after reset")


# ----------------------------------------------------------------------------- 4. independence
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_forward_between_pushes_does_not_touch_the_session(tiny_sd, precision):
    m = make_model(tiny_sd, precision)
    frames, other = frames_of(7, seed=7), frames_of(5, seed=8)
    with m.stream() as s:
        plain = preds_of(push_all(s, frames))
        plain_mem = s.memory()
    with m.stream() as s:
        steps = []
        for t, f in enumerate(frames):
            if t == 4:                                               # between pushes 3 and 4: same geometry, same engine workspaces
                m(other)
            steps.append(s.push(f))
        assert_same_preds(preds_of(steps[1:]), plain, "interrupted")
        assert_same_memory(s.memory(), plain_mem, "interrupted")


def test_two_sessions_on_one_model(models):
    m = models("bf16")
    fa, fb = frames_of(7, seed=7), frames_of(7, seed=8)
    ra, rb = forward_per_frame(m, fa), forward_per_frame(m, fb)
    assert not torch.equal(ra[0][-1]["conf"], rb[0][-1]["conf"])
    with m.stream() as sa, m.stream() as sb:
        a, b = [], []
        for x, y in zip(fa, fb):
            a.append(sa.push(x))
            b.append(sb.push(y))
        assert_same_preds(preds_of(a[1:]), ra[:2], "session a")
        assert_same_preds(preds_of(b[1:]), rb[:2], "session b")
        assert_same_memory(sa.memory(), ra[2], "session a")
        assert_same_memory(sb.memory(), rb[2], "session b")


# ----------------------------------------------------------------------------- 5. batch and orientation
@pytest.mark.parametrize("case", ["batch2", "swap"])
def test_stream_batch_and_orientation(models, case):
    m = models("bf16")
    if case == "batch2":
        frames = frames_of(6, seed=7, batch=2)
        shape = (2, 48, 64, 3)
    else:
        # portrait views the data set rotated to landscape: true_shape is the transposed image shape; the heads work on the 4 x 3
        # grid and the landscape_only wrapper hands the results back axis-swapped, i.e. in the image's own 48 x 64 raster
        ts = torch.tensor([[64, 48]], dtype=torch.int32)
        frames = [dict(f, true_shape=ts.clone()) for f in frames_of(6, seed=7)]
        shape = (1, 48, 64, 3)
    ref = forward_per_frame(m, frames)
    with m.stream() as s:
        got = preds_of(push_all(s, frames))
        assert s._run.swap == (case == "swap")
        assert tuple(got[0][0]["pts3d"].shape) == shape and got[0][0]["pts3d"].is_contiguous() == (case != "swap")
        assert_same_preds(got, ref[:2], case)
        assert_same_memory(s.memory(), ref[2], case)


# ----------------------------------------------------------------------------- 6. a long stream
def test_long_stream_crosses_prune_and_bank_switch(models):
    """352 frames: the CPU oracle on these frames prunes three times, never skips and ends at M = 4000, wm = 5, lm = 3940 -- the
    stream crosses the read's grid buckets, the prune and the switch of the arena half (each a new graph key).  Device memory the
    session holds does not grow with the frames pushed: between push 100 and push 351 only the second arena half arrives."""
    m = models("bf16")
    n = 352
    frames = frames_of(n, seed=11)
    ref = forward_per_frame(m, frames)
    ref_preds = ref[0]
    check = {1, 200, 340, 351}
    torch.cuda.synchronize()
    with m.stream() as s:
        alloc, banks = {}, {}
        for t, f in enumerate(frames):
            st = s.push(f)
            if t in check:
                for k in st.final:
                    assert torch.equal(st.final[k], ref_preds[t - 1][k]), (t, k)
            if t == n - 1:
                assert set(st.latest) == set(ref_preds[-1])
                for k in st.latest:
                    assert torch.equal(st.latest[k], ref_preds[-1][k]), ("latest", k)
            del st
            if t in (100, 351):
                torch.cuda.synchronize()
                alloc[t], banks[t] = torch.cuda.memory_allocated(), s._run.mem.bank_bytes()
        mem = s.memory()
        assert_same_memory(mem, ref[2], "long stream")
        assert mem.events == ["prune 4068->4000", "prune 4072->4000", "prune 4072->4000"]
        assert (mem.M, mem.wm, mem.lm) == (4000, 5, 3940)
        second_bank = banks[351] - banks[100]
        assert second_bank > 0
        print("device bytes after push 100: %d, after push 351: %d, second bank: %d; %d graphs" % (alloc[100], alloc[351], second_bank, len(s._run.graphs)))
        assert alloc[351] - alloc[100] in (0, second_bank)
        assert len(s._run.mem.events) <= 1024 and len(s._run.graphs) <= s._run.graphs.MAX_GRAPHS


# ----------------------------------------------------------------------------- 7. errors
def test_stream_errors(tiny_sd):
    m = make_model(tiny_sd, "fp32")
    frames = frames_of(4, seed=7)
    # training mode: both the autograd path and the growing bank
    m.train()
    with pytest.raises(RuntimeError, match="eval policy only"):
        m.stream()
    m.mem_dropout.eval()
    with pytest.raises(RuntimeError, match="eval policy only"):
        m.stream()
    m.eval()
    s = m.stream()
    with pytest.raises(RuntimeError, match="no CPU path"):
        s.push({"img": frames[0]["img"].cpu()})
    assert s.n_frames == 0
    assert s.push(frames[0]) is None and s.n_frames == 1
    with pytest.raises(RuntimeError):
        s.memory()
    with pytest.raises(ValueError, match="geometry"):                # another image size
        s.push({"img": torch.zeros(1, 3, 64, 80, device=DEV)})
    with pytest.raises(ValueError, match="geometry"):                # another batch
        s.push({"img": torch.zeros(2, 3, 48, 64, device=DEV)})
    with pytest.raises(ValueError, match="geometry"):                # another true_shape
        s.push(dict(frames[1], true_shape=torch.tensor([[64, 48]], dtype=torch.int32)))
    with pytest.raises(ValueError):                                  # no multiple of the patch size
        s.push({"img": torch.zeros(1, 3, 50, 64, device=DEV)})
    assert s.n_frames == 1
    step = s.push(frames[1])
    assert step.index == 1 and s.n_frames == 2
    # the engine is rebuilt under the session: precision, then weights
    m.set_precision("f32x6")
    with pytest.raises(RuntimeError, match="engine was rebuilt"):
        s.push(frames[2])
    with pytest.raises(RuntimeError, match="engine was rebuilt"):
        s.memory()
    s.close()
    m.set_precision("fp32")
    s = m.stream()
    s.push(frames[0])
    s.push(frames[1])
    with torch.no_grad():
        m._params["norm_q.weight"].mul_(1.0)                         # (same values: only the version counter moves)
    with pytest.raises(RuntimeError, match="engine was rebuilt"):
        s.push(frames[2])
    s.close()
    with pytest.raises(RuntimeError, match="closed"):
        s.push(frames[2])
    with pytest.raises(RuntimeError, match="closed"):
        s.reset()
    # the context manager closes
    with m.stream() as s:
        s.push(frames[0])
    with pytest.raises(RuntimeError, match="closed"):
        s.push(frames[1])


def test_stream_f16x3_range_guard(tiny_sd):
    """f16x3: an activation beyond the fp16 range turns the split products non-finite; the session checks `latest` of every push, as
    forward checks its last prediction.  (Non-finite values are planted behind the view-2 head's last ReLU, which would turn a NaN
    into 0: an infinite bias of its final 1 x 1 convolution.)"""
    m = make_model(tiny_sd, "f16x3")
    frames = frames_of(3, seed=7)
    with m.stream() as s:
        st = push_all(s, frames)[-1]
        assert torch.isfinite(st.latest["conf"]).all() and torch.isfinite(st.latest["pts3d_in_other_view"]).all()
    with torch.no_grad():
        m._params["dust3r.downstream_head2.dpt.head.4.bias"].fill_(float("inf"))
    with m.stream() as s:
        s.push(frames[0])
        with pytest.raises(FloatingPointError, match="f16x3"):
            s.push(frames[1])
    m.f16x3_range_guard = False
    with m.stream() as s:
        s.push(frames[0])
        st = s.push(frames[1])
        assert not torch.isfinite(st.latest["conf"]).all()
        assert torch.isfinite(st.final["conf"]).all()                # (view 1's head is untouched)
