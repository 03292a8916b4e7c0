"""A context owns its GPU resources: whatever its calls reserved comes back when it is closed.

ps_live_bytes (engine.live_bytes) is the library's own count of the device and pinned host bytes that the owning buffers of
all contexts of the process hold -- not the device's free memory, which moves with other people's work -- so every equality
below is exact.  Each test uses a Context of its own: a second one from engine.context() would switch lat_help off on the
shared context for the rest of the process.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pypore_amd import _lib, engine, synth  # noqa: E402
from pypore_amd.hmm import Model, NormalDistribution, State  # noqa: E402

SMALL_TAIL = 64 * 1024          # the status block a context reserves when it is created (csrc/poreseg.hip)
Q = synth.QUANTUM


def P():
    return _lib.split_params(prior_segments_per_second=10.)


def dwell_trace():
    """smoke()'s 300 000-sample dwell trace: several tiles, bridges and the look-ahead helpers."""
    return torch.from_numpy(synth.counts_to_pa(synth.random_dwell_counts(300000, 5))).cuda(), np.array([0, 300000], dtype=np.int64)


def test_create_and_close_return_everything():
    base = engine.live_bytes()
    for _ in range(51):
        cx = engine.Context(0)
        assert engine.live_bytes() >= base + SMALL_TAIL
        cx.close()
        assert engine.live_bytes() == base


def three_state_model():
    m = Model("three")
    a, b, c = (State(NormalDistribution(mu, 1.0), n) for n, mu in (("a", 0.0), ("b", 3.0), ("c", 6.0)))
    for x, y, p in ((m.start, a, 0.6), (m.start, b, 0.4), (a, a, 0.5), (a, b, 0.5), (b, b, 0.4), (b, c, 0.6), (c, c, 0.5),
                    (c, a, 0.2), (c, m.end, 0.3)):
        m.add_transition(x, y, p)
    m.bake()
    return m


def every_entry_family(cx):
    dev = torch.device("cuda", cx.device)
    t, ev = dwell_trace()
    cx.segment_batch(t, ev, P(), Q)
    # the single-pass file route (blk_cls, cls_mm): smoke()'s int16 file trace
    c, _ = synth.file_trace_counts(600000, 41, gap=30011, ev_lo=60000, ev_hi=200000)
    thr, mc = engine.detector_thresholds(Q, 90.0, -0.5)
    st, _, _, _, _ = cx.detect_segment_trace(torch.from_numpy(c.astype(np.int16)).cuda(), Q, P(), thr, 1000, mc)
    assert len(st) >= 2
    rng = np.random.RandomState(3)
    x64 = torch.from_numpy(np.repeat([40.0, 55.0, 47.0, 38.0], 1024) + rng.normal(0, 1, 4096)).to(dev)
    cx.segment_exact_f64(x64, np.zeros(1, np.int64), np.full(1, 4096, np.int64), P())
    f = t[:100000].contiguous()
    cx.filter_bessel(f, Q)
    cx.filter_requantise_batch(f, np.array([0, 50000], np.int64), np.array([50000, 50000], np.int64), Q)
    # two sequences of 16: the profile aligner against a model of 16, and the pair of them through the pairwise aligner
    lv = np.cumsum(rng.uniform(-8, 10, 16)) + 40
    cols = [torch.from_numpy(np.concatenate([lv, lv + 0.1]) if k == 0 else np.full(32, s)).to(dev) for k, s in enumerate((0, 1.0, 0.001))]
    off2 = np.array([0, 16, 32], np.int64)
    cx.align_batch(lv, np.ones(16), np.full(16, 0.001), 0.5, 0.5, cols[0], cols[1], cols[2], off2)
    one = np.zeros(1, np.int32)
    s16 = np.array([0, 16], np.int64)
    cx.pairwise_batch(cols[0][:16].contiguous(), s16, cols[0][16:].contiguous(), s16, one, one, _lib.PS_PW_GLOBAL, -1.0)
    # a three-state model, four sequences of eight observations: every HMM entry
    m = three_state_model()
    cm = m._c_model()
    obs = torch.from_numpy(rng.normal(3.0, 2.0, 32)).to(dev)
    off4 = np.arange(0, 33, 8, dtype=np.int64)
    for mode in (_lib.PS_HMM_VITERBI, _lib.PS_HMM_FORWARD, _lib.PS_HMM_BACKWARD):
        cx.hmm_batch(cm, mode, obs, off4, want_mat=(mode != _lib.PS_HMM_VITERBI))
    cx.hmm_expect(cm, obs, off4)
    cx.hmm_posterior(cm, obs, off4, want_post=True, want_map=True, want_counts=True)
    cx.hmm_sample(cm, m._sample_tables()["c"], 7, 0, 4, want_path=True)
    cx.statsplit_f64(x64, np.array([0, 2048], np.int64), np.full(2, 2048, np.int64), _lib.StatSplitParams(50, 100000, 500, 250.0, 0, 0))
    g = torch.from_numpy(synth.counts_to_pa(synth.random_dwell_counts(4096, 9), np.float64)).to(dev)
    cx.grid_check(g, 0.0, Q)
    cx.grid_counts(g, 0.0, Q, 1500)
    cx.narrow_f64(g)


def test_every_features_buffers_come_back():
    base = engine.live_bytes()
    cx = engine.Context(0)
    created = engine.live_bytes()
    every_entry_family(cx)
    # densely stepped data with one anchor per bridge: seams give up, and the second-chance buffers are reserved
    before = engine.live_bytes()
    dense = torch.from_numpy(synth.random_dwell_counts(300000, 77, 100, 400).astype(np.int16)).cuda()
    cx.set_option("bridge_budget", 1)
    cx.segment_batch(dense, np.array([0, 300000], np.int64), P(), Q, want_stats=False)
    print("live bytes: base %d, created %d, after every family %d, after the second chance %d, seams mended %d"
          % (base, created, before, engine.live_bytes(), cx.timings()["repairs"]))
    assert cx.timings()["repairs"] > 0 and engine.live_bytes() > before
    assert engine.live_bytes() > created
    cx.close()
    assert engine.live_bytes() == base
    again = engine.Context(0)
    t, ev = dwell_trace()
    again.segment_batch(t, ev, P(), Q)
    again.close()
    assert engine.live_bytes() == base


def test_views_count_zero():
    """A call that repeats the layout re-aliases its tables into the upload blob: nothing is allocated, nothing freed."""
    cx = engine.Context(0)
    try:
        t, ev = dwell_trace()
        first = cx.segment_batch(t, ev, P(), Q)[0].cpu().numpy()
        held = engine.live_bytes()
        second = cx.segment_batch(t, ev, P(), Q)[0].cpu().numpy()
        assert engine.live_bytes() == held
        assert first.size > 0 and np.array_equal(first, second)
    finally:
        cx.close()
