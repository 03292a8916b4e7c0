"""Context.hmm_batch's repeat on PS_ERR_CAPACITY (the per-sequence-slot rule of engine._retry_slots) on the device: Viterbi paths
that do not fit their slots make the call run again with slots of the exact lengths.  Nothing else reaches this repeat: the
default slots, 2 (n + 1) + the silent states + 1, always fit."""
import numpy as np
import pytest

from pypore_amd import _lib
from pypore_amd.hmm import Model, NormalDistribution, State


@pytest.mark.gpu
def test_viterbi_paths_longer_than_their_slots_are_decoded_again_with_exact_slots():
    m = Model("two")                                       # the smallest finite model with two emitting states
    a, b = State(NormalDistribution(0.0, 1.0), "a"), State(NormalDistribution(4.0, 1.0), "b")
    m.add_transition(m.start, a, 1.0)
    m.add_transition(a, a, 0.5)
    m.add_transition(a, b, 0.5)
    m.add_transition(b, b, 0.5)
    m.add_transition(b, m.end, 0.5)
    m.bake()
    ctx, off, obs = m._upload([[0.1, 3.9, 4.2], [-0.3, 0.2, 4.1]], None)
    assert off.tolist() == [0, 3, 6]
    logp0, _, (path0, off0, len0) = ctx.hmm_batch(m._c_model(), _lib.PS_HMM_VITERBI, obs, off)
    logp1, _, (path1, off1, len1) = ctx.hmm_batch(m._c_model(), _lib.PS_HMM_VITERBI, obs, off, path_slots=np.ones(2, dtype=np.int64))
    path0, len0, path1, len1 = path0.cpu().numpy(), len0.cpu().numpy(), path1.cpu().numpy(), len1.cpu().numpy()
    assert len0.tolist() == len1.tolist() and min(len0) > 1                  # (one entry per sequence did not fit: the call ran twice)
    assert np.array_equal(logp0.cpu().numpy(), logp1.cpu().numpy()) and np.all(np.isfinite(logp0.cpu().numpy()))
    # the repeat's slots are the exact lengths, so its path tensor is the default call's paths back to back, element for element
    assert off1.tolist() == np.concatenate(([0], np.cumsum(len0))).tolist() and path1.size == int(off1[-1])
    for q in range(2):
        assert path1[off1[q]:off1[q + 1]].tolist() == path0[off0[q]:off0[q] + len0[q]].tolist()
    states = [s.name for s in m.states]
    assert [states[i] for i in path1[off1[0]:off1[1]] if states[i] in "ab"] == ["a", "b", "b"]
    assert [states[i] for i in path1[off1[1]:off1[2]] if states[i] in "ab"] == ["a", "a", "b"]
