"""CPU model of the frame decoder's recursion engine (csrc/tdec_frame.hip).

The kernel's correctness rests on three pieces of algebra that can be checked
without a GPU, in numpy float32 with the same operations:
  1. the time-varying lane labelling: with lane l holding state rotl^t(l)
     (beta: rotr^t(rev(l))), every state's two predecessors (successors) are
     the lane itself and lane l ^ (8 >> (t % 4)), with the pair-maxima indices
     fr_lane() computes;
  2. the segment rounds: 4 segments from zero, re-runs from the predecessor's
     end until the vector equals the stored one (checked at 4-step block
     starts), the reference's second pass as a round from the first pass's
     end vector -- the stored vectors equal the serial two-pass recursion of
     dvb_rcs2_turbo.py:162-230 bit for bit;
  3. that this holds when merging is slow or impossible (NaN, tiny inputs).
"""
import numpy as np
import pytest

from frame_model import (frame_recursion, lane_consts, lane_step, reference_two_pass, rev4, rotl4, rotr4,
                         serial_pass)


def _pm(rng, N, scale):
    g = (rng.standard_normal((N, 8)) * scale).astype(np.float32)
    return g


def test_labelling_partner_is_the_other_predecessor():
    for beta in (False, True):
        lbl, idx = lane_consts(beta)
        for ph in range(4):
            for l in range(16):
                p = l ^ (8 >> ph)
                if not beta:
                    assert lbl[ph, p] == lbl[ph, l] ^ 8
                    assert rotr4(rotl4(l, ph + 1), 1) == lbl[ph, l]
                else:
                    assert lbl[ph, p] == lbl[ph, l] ^ 1
                    assert rotl4(rotr4(rev4(l), ph + 1), 1) == lbl[ph, l]
            assert lbl[ph, 0] == 0    # state 0 stays in lane 0: the normalisation reads lane 0


@pytest.mark.parametrize("beta", [False, True])
def test_lane_step_equals_serial_step(beta):
    rng = np.random.default_rng(1)
    pm = _pm(rng, 12, 3.0)
    ref, _ = serial_pass(pm, np.zeros(16, np.float32), beta)
    lbl, idx = lane_consts(beta)
    v = np.zeros(16, np.float32)
    for u in range(12):
        ph = u % 4
        np.testing.assert_array_equal(v, ref[u][lbl[ph]])
        v = lane_step(v, pm[12 - 1 - u if beta else u], ph, idx)


@pytest.mark.parametrize("beta", [False, True])
@pytest.mark.parametrize("N", [1, 2, 3, 5, 8, 13, 16, 17, 33, 48, 101, 212])
@pytest.mark.parametrize("scale", [3.0, 1e-3])
@pytest.mark.parametrize("P", [4, 8, 16])
@pytest.mark.parametrize("lmin", [0, 32, 48])
@pytest.mark.parametrize("blk", [4, 8])
def test_segment_rounds_equal_two_pass(beta, N, scale, P, lmin, blk):
    rng = np.random.default_rng(N * 3 + int(beta))
    pm = _pm(rng, N, scale)
    st, _ = frame_recursion(pm, beta, P, lmin, blk)
    np.testing.assert_array_equal(st, reference_two_pass(pm, beta))


@pytest.mark.parametrize("beta", [False, True])
def test_segment_rounds_never_merging(beta):
    """NaN branch metrics: vectors with NaN never compare equal, so every
    segment runs to its end and the rounds hand the vectors down the chain."""
    rng = np.random.default_rng(5)
    pm = _pm(rng, 60, 2.0)
    pm[7, 3] = np.nan
    pm[40, :] = np.inf
    st, stats = frame_recursion(pm, beta)
    ref = reference_two_pass(pm, beta)
    np.testing.assert_array_equal(st, ref)


def test_segment_rounds_random_sweep_covers_every_path():
    """Random block lengths and metric scales: every control path of the rounds
    (speculative second pass kept, dropped, dropped with the chain broken at
    segment 0) is taken, and every result equals the serial two passes."""
    rng = np.random.default_rng(2025)
    seen = set()
    for trial in range(120):
        N = int(rng.integers(9, 90)) if trial % 3 else int(rng.integers(300, 420))
        scale = float(10 ** rng.uniform(-3, 1))
        pm = _pm(rng, N, scale)
        if trial % 7 == 0:
            pm[rng.integers(0, N)] = np.nan
        beta = bool(trial % 2)
        st, stats = frame_recursion(pm, beta, (4, 8, 16, 8)[trial % 4], (0, 0, 48, 32, 64)[trial % 5],
                                    (8, 4)[trial % 2 if trial % 3 else 0])
        np.testing.assert_array_equal(st, reference_two_pass(pm, beta))
        seen.add((stats["spec"], stats["broken"]))
    assert {(True, False), (False, False), (False, True)} <= seen, seen
