"""The last step of forward(frames) without return_memory (spann3r_amd/model.py, _SequenceRunner.run(last=True)): what it would leave for
a next step has no reader, so it launches neither the key MLPs, the similarity scores, the value encoder nor the bank write, and the
host neither polls nor commits.  Held here, on the tiny model at 48 x 64:
  * the outputs are torch.equal, key by key, to forward(frames, return_memory=True)[:2] -- eagerly, at capture and at replay;
  * a later return_memory=True call on the same model returns the memory of a fresh model (nothing pending, nothing staged);
  * launched eagerly under ops.Profiler, the last step issues none of those launches and the step before it all of them;
  * the trimmed step is one more hipGraph per geometry, not more.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
_REF = {}


def _model(tiny_sd, policy, prec):
    from spann3r_amd import Spann3R, TINY
    m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False)
    m.load_state_dict(tiny_sd, strict=True)
    m = m.to(DEV).eval().set_precision(prec)
    if policy == "growing":                       # the forward-only growing bank: train policy, dropout off
        m.train()
        m.mem_dropout.eval()
    return m


def _frames(n):
    from spann3r_amd.weights import synth_frames
    return [{k: (v.to(DEV) if k == "img" else v) for k, v in f.items()} for f in synth_frames(n, 48, 64, seed=21)]


def _ref(tiny_sd, policy, prec, n):
    """forward(frames, return_memory=True) of a fresh model: computed once per (policy, precision, length), never changed"""
    key = (policy, prec, n)
    if key not in _REF:
        _REF[key] = _model(tiny_sd, policy, prec)(_frames(n), return_memory=True)
    return _REF[key]


def _same_outputs(got, ref, tag):
    preds, preds_all = got[0], got[1]
    assert len(preds) == len(ref[0]) and len(preds_all) == len(ref[1]), tag
    for a, b in zip(preds, ref[0]):
        assert sorted(a) == sorted(b), tag
        for k in a:
            assert torch.equal(a[k], b[k]), (tag, k)
    for (a1, a2), (b1, b2) in zip(preds_all, ref[1]):
        for a, b in ((a1, b1), (a2, b2)):
            assert sorted(a) == sorted(b), tag
            for k in a:
                assert torch.equal(a[k], b[k]), (tag, k)


def _same_memory(got, ref, tag):
    for name in ("mem_k", "mem_v", "mem_attn", "mem_count"):
        a, b = getattr(got, name), getattr(ref, name)
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), (tag, name)
    assert got.events == ref.events, tag


def _whole(run):
    return {k for k in run.graphs if k[0] == "whole"}


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("policy,prec", [("eval", "bf16"), ("growing", "bf16"), ("eval", "fp32")])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_trimmed_last_step(tiny_sd, n, policy, prec, graphs):
    ref = _ref(tiny_sd, policy, prec, n)
    frames = _frames(n)
    m = _model(tiny_sd, policy, prec)
    m.use_graphs = graphs
    tag = (n, policy, prec, graphs)
    if graphs:
        for _ in range(3):                                       # eager, capture, replay
            full = m(frames, return_memory=True)
            _same_outputs(full, ref, tag)
    run = next(iter(m._runners.values())) if graphs else None
    before = _whole(run) if graphs else set()
    for call in range(3 if graphs else 1):                       # the trimmed kind: eager, capture, replay
        got = m(frames)
        assert len(got) == 2
        _same_outputs(got, ref, tag + (call,))
    if graphs:
        after = _whole(run)
        assert before <= after and len(after - before) == 1, (tag, after - before)
        assert len(run.graphs) <= run.graphs.MAX_GRAPHS
    # nothing of the trimmed call is left behind: the next full call returns a fresh model's memory
    full = m(frames, return_memory=True)
    _same_outputs(full, ref, tag)
    _same_memory(full[2], ref[2], tag)
    run = next(iter(m._runners.values()))
    assert run.mem._pending_attn is None and not run.mem._score_pending
    if graphs:
        assert _whole(run) == after and len(run.graphs) <= run.graphs.MAX_GRAPHS


@pytest.mark.parametrize("policy", ["eval", "growing"])
def test_last_step_launches(tiny_sd, policy, monkeypatch):
    """eager launches under ops.Profiler, 5 frames: per step, which of the trimmed launches were issued"""
    from spann3r_amd import ops
    from spann3r_amd.engine import Engine
    from spann3r_amd.model import SpatialMemory
    n = 5
    frames = _frames(n)
    m = _model(tiny_sd, policy, "bf16")
    m.use_graphs = False
    seen = []                                                    # (step, what)

    class Prof(ops.Profiler):
        steps = 0

        def step_begin(self):
            self.steps += 1

    prof = Prof()

    def spy(owner, name, what):
        orig = getattr(owner, name)

        def wrapped(*a, **kw):
            seen.append((prof.steps - 1, what))
            return orig(*a, **kw)
        monkeypatch.setattr(owner, name, wrapped)

    for name in ("encode_feat_keys_grouped", "encode_feat_key"):
        spy(Engine, name, "key MLP")
    for name in ("encode_cur_value", "encode_cur_value_feat"):
        spy(Engine, name, "value encoder")
    spy(SpatialMemory, "sim_scores", "cosine")
    for name in ("cos_sim", "cos_sim_state"):
        spy(ops, name, "cosine")
    spy(ops, "bank_write", "bank write")
    spy(ops, "colsum_softmax", "column sums")
    spy(ops, "mem_append", "append")
    ops.set_profiler(prof)
    try:
        got = m(frames)
    finally:
        ops.set_profiler(None)
    torch.cuda.synchronize()
    _same_outputs(got, _ref(tiny_sd, policy, "bf16", n), policy)
    assert prof.steps == n - 1
    keys = [r[0] for r in prof.rec]
    assert keys.count("bank_write") == n - 2                      # the profiler's own record: one bank write per step but the last
    last = {w for s, w in seen if s == n - 2}
    prev = {w for s, w in seen if s == n - 3}
    # (the column sums of the read before / the append are issued by the policy call BEHIND a step: they carry that step's index)
    assert last == set(), last
    want = {"key MLP", "value encoder", "bank write"} | ({"cosine"} if policy == "eval" else set())
    assert want <= prev, (want, prev)
