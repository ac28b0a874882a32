"""Streaming sessions: the per-frame step of Spann3R.forward fed one frame at a time (INTEGRATION.md "Streaming").

    with model.stream() as s:
        for view in camera:                  # forward-style dicts: img fp32 [B,3,H,W] on the device, optional true_shape
            step = s.push(view)              # None for the first frame, a StreamStep afterwards
            ...

The reference's loop is causal (spann3r/model.py:485-531: step i reads frames i, i+1 and the memory of the steps before it), so after
frames 0..n-1 a session has handed out exactly what forward(frames[:n]) returns: [step.final ...] + [last step.latest] is `preds`,
[step.pair ...] is `preds_all`, memory() is the `return_memory=True` snapshot -- bit for bit against the frame-by-frame schedule
(batch_encode = False), whose kernels the streaming step launches at the same shapes.
"""
import torch

from .model import _SequenceRunner

MAX_EVENTS = 1024        # SpatialMemory.events entries (skip / window / prune) a session keeps: the most recent ones


class StreamStep:
    """What one push returns.  index: the frame just pushed (t).  final: the prediction of frame t-1, as forward puts it in
    preds[t-1] ('pts3d' for frame 0, else 'pts3d_in_other_view'; 'conf').  latest: the prediction of frame t as view 2 -- what forward
    would return as its last element if the sequence ended here.  pair: (final, latest), the same dict objects (preds_all's aliasing)."""
    __slots__ = ("index", "final", "latest", "pair")

    def __init__(self, index, final, latest):
        self.index, self.final, self.latest = index, final, latest
        self.pair = (final, latest)

    def __repr__(self):
        return "StreamStep(index=%d)" % self.index


class Spann3RStream:
    """One sequence in flight on one model.  The session owns a private _SequenceRunner -- static buffers, memory arena, hipGraphs --
    that is no entry of the model's runner cache: a forward call on the same geometry, or another session, cannot reset or overwrite
    its memory.  It is bound to the engine it was opened with; after changed weights or set_precision a push raises.
    (session -> model and session -> runner are strong references, the runner holds the model weakly, the model does not know the
    session: no cycle, so the session's hipGraphs die by reference count -- at close(), or when the last reference to it goes.)"""

    def __init__(self, model):
        if model.training:
            # train mode is either the autograd path (spann3r_amd/train.py) or the growing bank, whose capacity is (n - 1) * P: no
            # bound without the number of frames
            raise RuntimeError("Spann3R.stream(): eval policy only -- a training-mode memory grows with the sequence and a stream "
                               "has no known length; call model.eval() first")
        self._model = model
        self._eng = model.engine              # (raises on a CPU model: no CPU fallback)
        self._run = None
        self._geom = None
        self._n = 0
        self._closed = False
        self.replays = 0                      # pushes whose step replayed (or was captured as) a hipGraph

    # ------------------------------------------------------------------ life cycle
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        """drop the session's graphs and buffers here (outside any capture); a later push raises"""
        run, self._run = self._run, None
        if run is not None:
            run.graphs.clear()
            run.mem = None
        self._closed = True

    def reset(self):
        """a new sequence on the same buffers and graphs (the geometry stays fixed)"""
        self._check_open()
        if self._run is not None:
            self._run.ensure_memory(2)
        self._n = 0

    @property
    def n_frames(self):
        return self._n

    def memory(self):
        """what forward(..., return_memory=True) hands out after the frames pushed so far"""
        self._check_open()
        if self._run is None or self._n < 2:
            raise RuntimeError("Spann3RStream.memory(): the memory is written by the first step (push two frames first)")
        self._engine()
        return self._run.mem.snapshot()

    # ------------------------------------------------------------------ checks
    def _check_open(self):
        if self._closed:
            raise RuntimeError("Spann3RStream is closed")

    def _engine(self):
        eng = self._model.engine
        if eng is not self._eng:
            raise RuntimeError("Spann3RStream: the model's engine was rebuilt (weights changed or set_precision) since the session was "
                               "opened; its memory and packed weights are stale -- open a new session")
        return eng

    def _geometry(self, view):
        """(B, H, W, true_hw) of one frame by forward's rule for a uniform sequence (Spann3R._uniform_true_hw)"""
        img = view["img"]
        hw = self._model._uniform_true_hw([view])
        if hw is None or img.dim() != 4 or img.shape[1] != 3:
            raise ValueError("Spann3RStream.push: img must be [B, 3, H, W] with H, W multiples of the patch size and one true_shape "
                             "(the image shape or its transpose) for the whole batch; got img %s, true_shape %s"
                             % (tuple(img.shape), view.get("true_shape")))
        return int(img.shape[0]), int(img.shape[2]), int(img.shape[3]), hw

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def push(self, view):
        self._check_open()
        img = view["img"]
        if not img.is_cuda:
            raise RuntimeError("spann3r_amd runs on an MI355X (HIP kernels); there is no CPU path -- move the frames to the GPU")
        eng = self._engine()
        geom = self._geometry(view)
        if self._geom is None:
            B, H, W, hw = self._geom = geom
            self._run = run = _SequenceRunner(self._model, eng, B, H, W, False, hw)
            run.own_key_aux()
            run.batched = run.defer2 = False
            run.ensure_memory(2)
        elif geom != self._geom:
            raise ValueError("Spann3RStream.push: frame geometry (B, H, W, true_shape) %s differs from the session's %s "
                             "(mixed shapes stay with forward's general path)" % (geom, self._geom))
        run, model, B, t = self._run, self._model, self._geom[0], self._n
        if t == 0:
            run.img_pair[:B].copy_(img)
            self._n = 1
            return None
        if t == 1:
            run.img_pair[B:].copy_(img)
            # the first step happens once per sequence: launched eagerly, never captured (a reset() then replays without a new capture)
            res1, res2 = run.run(True, False, False, stream=True)
        else:
            run.img_next.copy_(img)
            res1, res2 = run.run(False, False, model.use_graphs, stream=True)
            self.replays += run.graphs.last != "eager"
        res2["pts3d_in_other_view"] = res2.pop("pts3d")                  # spann3r/model.py:523
        if t > 1:
            res1["pts3d_in_other_view"] = res1.pop("pts3d")
        ev = run.mem.events
        if len(ev) > MAX_EVENTS:
            del ev[:-MAX_EVENTS]
        self._n = t + 1
        if model.precision == "f16x3" and model.f16x3_range_guard:
            # as Spann3R._forward_inference, on every push (the step has already synchronised on its similarity verdict)
            ok = torch.isfinite(res2["conf"]).all() & torch.isfinite(res2["pts3d_in_other_view"]).all()
            if not bool(ok):
                raise FloatingPointError("f16x3: non-finite outputs -- an activation left the fp16 range (|x| >= 65504) of the split "
                                         "products; run this checkpoint with set_precision('f32x6') or 'fp32'")
        return StreamStep(t, res1, res2)
