"""Query blocks per workgroup of sp3_attention_packed (csrc/attention.hip): the library states its rule through the host-only
sp3_attention_packed_qb(B, heads, Nq), and a query block's result must not depend on the count that computed it.

The rule that ships takes two blocks from 512 query rows on and one below, whatever the batch: two and four blocks were measured on
the whole-sequence encoder's launch (10 images x 16 heads x 196 rows) and lost to one (profiles/encoder_attention_last_step.txt), so
no batch at 196 or 33 rows yields more than one block.  The cases below therefore ask the library which count each launch takes and
hold, for whatever it answers:
  * the output within the float64 bound of tests/attention_ref.py, nothing outside the defined rows touched (guard bands, NaN pre-fill);
  * the output torch.equal to the same rows computed image by image, in calls of fewer than 512 query rows, which take ONE block.
Shapes: the encoder's own (10 x 16 x 196 x 196); ragged q block and a ragged key tile that holds one key at the same batch
(33 x 65); and the two-block launch with both, its last workgroup's second block past the padded rows (513 x 65, three images so that
the XCD map hands out more than one (head, image) pair per column).
"""
import copy

import pytest
import torch

import attention_ref as AR
from gemm_desc_ref import BF

DEV = "cuda"
# (B, heads, Nq, Nk, extra) next to the shapes of the forms matrix
AR.SHAPES.setdefault("qb_encoder", (10, 16, 196, 196, {}))
AR.SHAPES.setdefault("qb_ragged", (10, 16, 33, 65, {}))
AR.SHAPES.setdefault("qb_two_blocks", (3, 2, 513, 65, {"npad_q": 528}))
CHUNK = 496                  # query rows of a reference call: whole 16-row blocks, fewer than 512 rows
_CASES = {}


def _ops():
    from spann3r_amd import ops
    return ops


def _case(shape):
    """one float64 reference per shape, shared by the output kinds"""
    if shape not in _CASES:
        _CASES[shape] = AR.Case("c", "bf16", shape, "flat")
    return _CASES[shape]


def _sub(case, b, r0, r1):
    """rows [r0, r1) of image b of `case` as a launch of its own (operands only: no reference)"""
    s = copy.copy(case)
    s.Bt, s.Nq, s.npad_q_min = 1, r1 - r0, None
    s.q, s.k, s.v = case.q[b:b + 1, r0:r1], case.k[b:b + 1], case.v[b:b + 1]
    return s


def test_rule_cpu():
    """host only: no launch, no GPU"""
    qb = _ops().attention_packed_qb
    assert qb(2, 12, 196) == 1 and qb(1, 16, 196) == 1          # the per-step launches: decoder self-attention, value encoder
    assert qb(1, 16, 513) == 2 and qb(1, 16, 512) == 2 and qb(1, 16, 511) == 1
    for heads, Nq in ((16, 196), (16, 33), (12, 196), (16, 513), (2, 1024)):
        got = [qb(B, heads, Nq) for B in range(1, 65)]
        assert all(g in (1, 2, 4) for g in got), got
        assert got == sorted(got), (heads, Nq, got)              # monotone in B
    assert qb(0, 16, 196) == 0 and qb(1, 0, 196) == 0 and qb(1, 16, 0) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [(BF, True), (torch.float32, False)], ids=["bf16-packed", "fp32-rows"])
@pytest.mark.parametrize("shape", ["qb_encoder", "qb_ragged", "qb_two_blocks"])
def test_block_count_does_not_change_a_row(shape, kind):
    ops = _ops()
    c = _case(shape)
    took = ops.attention_packed_qb(c.Bt, c.heads, c.Nq)
    assert took == (2 if c.Nq >= 512 else 1), (shape, took)
    lay = c.layout(DEV, kind, "stale")
    lay.launch(ops)
    torch.cuda.synchronize()
    assert lay.untouched(), shape
    got = lay.output()
    assert not bool(torch.isnan(got).any()), shape
    r = AR.ratio(c, got, kind[0])
    print("%s %s: %d block(s) per workgroup, ratio to the float64 bound %.3f" % (shape, kind, took, r))
    assert r <= 1.0, (shape, r)
    for b in range(c.Bt):
        for r0 in range(0, c.Nq, CHUNK):
            r1 = min(c.Nq, r0 + CHUNK)
            assert ops.attention_packed_qb(1, c.heads, r1 - r0) == 1
            sl = _sub(c, b, r0, r1).layout(DEV, kind, "stale")
            sl.launch(ops)
            torch.cuda.synchronize()
            assert sl.untouched(), (shape, b, r0)
            assert torch.equal(sl.output()[0], got[b, r0:r1]), (shape, b, r0)
