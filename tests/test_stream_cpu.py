"""The ground the streaming contract (spann3r_amd/stream.py) stands on, checked without a GPU: the reference's loop is causal, and the
streaming interface exists on a CPU build and refuses to run there."""
import pytest
import torch


def test_reference_loop_is_causal(tiny_sd):
    """forward(frames[:k]) is a prefix of forward(frames): its predictions are the first k - 1 of the full run bit for bit, and its
    last one is the view-2 result of the full run's step k - 2 -- what a session hands out as `final` ... `latest` after k pushes."""
    from oracle import spann3r_oracle as O
    from spann3r_amd import TINY
    from spann3r_amd.weights import synth_frames
    frames = synth_frames(6, 48, 64, seed=7)
    preds, preds_all = O.forward(frames, tiny_sd, TINY)
    assert len(preds) == 6 and len(preds_all) == 5
    for k in range(2, 6):
        p, pa = O.forward(frames[:k], tiny_sd, TINY)
        assert len(p) == k and len(pa) == k - 1
        for j in range(k - 1):
            assert set(p[j]) == set(preds[j])
            for key in p[j]:
                assert torch.equal(p[j][key], preds[j][key]), (k, j, key)
        last = preds_all[k - 2][1]
        assert set(p[-1]) == set(last) == {"pts3d_in_other_view", "conf"}
        for key in last:
            assert torch.equal(p[-1][key], last[key]), (k, key)


def test_stream_module_imports_and_refuses_the_cpu():
    import spann3r_amd.stream as S
    from spann3r_amd import Spann3R, TINY
    assert hasattr(S, "Spann3RStream") and hasattr(S, "StreamStep")
    m = Spann3R(dus3r_name=None, cfg=TINY, init_weights=False).eval()
    with pytest.raises(RuntimeError, match="MI355X"):                # the error of test_no_cpu_fallback, not an AttributeError
        m.stream()
    st = S.StreamStep(3, {"conf": 0}, {"conf": 1})
    assert st.index == 3 and st.pair[0] is st.final and st.pair[1] is st.latest
