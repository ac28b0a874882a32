"""Host-side logic of the DPT head's level launches: the workgroup -> (problem, tile) map of conv_level_kernel (csrc/gemm_sm.hip),
restated by ops.level_block_map, produces every output tile of every problem exactly once for each level the head issues."""
import pytest


def _head_levels(B, nh, nw):
    """(tile, M, N, K) of the small-map convolutions dpt_head puts into its three level launches; tile by the library's size rule"""
    h3, w3 = (nh - 1) // 2 + 1, (nw - 1) // 2 + 1
    t = lambda M: 40 if M <= 256 else 41
    c = lambda M, N, K: (t(M), M, N, K)
    P, P2, P3 = B * nh * nw, B * 4 * nh * nw, B * h3 * w3
    levels = [[c(P3, 768, 9 * 768), c(P, 256, 9 * 384)],
              [c(P2, 256, 9 * 192), c(P3, 256, 9 * 768), c(P, 256, 9 * 256)],
              [c(P3, 256, 9 * 256), c(P2, 256, 9 * 256)]]
    return [[p for p in lv if p[1] <= 2048] for lv in levels]         # (larger maps run on the LDS-tiled kernel, outside the group)


@pytest.mark.parametrize("B,nh,nw", [(1, 14, 14), (9, 14, 14), (1, 10, 14), (9, 10, 14), (4, 14, 14), (1, 32, 32), (1, 3, 5)])
def test_level_block_map_is_a_bijection(B, nh, nw):
    from spann3r_amd import ops
    for lv in _head_levels(B, nh, nw):
        if len(lv) < 2:
            continue
        order = ops.level_order([(t, K) for t, _, _, K in lv])
        assert sorted(order) == list(range(len(lv)))
        cost = [(lv[i][3] // 64) * (2 if lv[i][0] == 40 else 3) for i in order]
        assert cost == sorted(cost, reverse=True)                      # the longest contraction per wave is dispatched first
        probs = [lv[i][:3] for i in order]
        total, f = ops.level_block_map(probs)
        assert total % 8 == 0
        seen, last_p = {}, 0
        for w in range(total):
            p, tm, tn = f(w)
            assert p >= last_p                                         # each problem owns one contiguous range
            last_p = p
            tile, M, N = probs[p]
            bm = 16 if tile == 40 else 32
            assert 0 <= tm < (M + bm - 1) // bm
            if tn * bm >= N:
                continue                                               # padding of an 8-wide group: the workgroup exits
            assert (p, tm, tn) not in seen
            seen[(p, tm, tn)] = w % 8
            assert tn % 8 == w % 8                                     # the sharers of a weight panel sit on one XCD, as in a launch of its own
        want = sum(((M + (16 if t == 40 else 32) - 1) // (16 if t == 40 else 32)) * (N // (16 if t == 40 else 32)) for t, M, N in probs)
        assert len(seen) == want
