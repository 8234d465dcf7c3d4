"""Non-temporal loads of rho in the two fused per-chunk kernels (VBX_OPT_STREAM_LOADS, the STREAM instances of
vbx_amd/csrc/vbx_chunk_loglik.hpp / vbx_chunk_post.hpp) -- -m gpu.

A cache policy changes no arithmetic: with the option forced on, every result must equal the forced-off run bit for bit, at
the smallest shapes at which the changed loads can go wrong, and stay within the bounds tests/test_gpu_split.py holds the
split path to against the float64 oracle.  The automatic choice is a matter of bytes (tests/test_stream_loads_host.py) and
picks "off" for every shape here; the option is what puts these shapes through the streaming instances.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4          # gamma, pi against the oracle (tests/test_gpu_split.py)
LI_RTOL = 2e-6           # Li, relative

SHAPES = [
    (1, 2, 32),          # one frame, one K-block
    (64, 30, 128),       # one half of one tile
    (65, 30, 128),       # ... and one frame of the second half
    (129, 30, 100),      # a second tile of one frame, padded dims
    (777, 10, 128),      # Sp = 16
    (1300, 50, 128),     # Sp = 64
    (900, 30, 160),      # Dp = 160: the second slice of the staged model
]
PRECISIONS = ['fp32-split', 'fp32', 'fp64']


@pytest.fixture(scope='module')
def ctx():
    from vbx_amd import _capi
    return _capi.Context(0)


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def _soft(T, S, seed):
    g = np.random.default_rng(seed).gamma(1.0, size=(T, S))
    return g / g.sum(1, keepdims=True)


def _inputs(T, S, D):
    from vbx_amd.synth import make_recording
    X, Phi, _ = make_recording(T, S, D=D, seed=T + S, kappa=0.05)
    return X, Phi, _soft(T, S, 5)


_ORACLE = {}


def _oracle(T, S, D):
    """Three iterations of the float64 oracle from the soft start of _inputs: computed once per shape, never changed."""
    if (T, S, D) not in _ORACLE:
        from oracle import vbx_oracle
        X, Phi, g0 = _inputs(T, S, D)
        g, pi, Li = vbx_oracle.VBx(X, Phi, loopProb=0.95, Fa=0.3, Fb=17.0, pi=S, gamma=g0, maxIters=3, epsilon=-np.inf)[:3]
        for a in (g, pi):
            a.setflags(write=False)
        _ORACLE[T, S, D] = (g, pi, np.array([x[0] for x in Li]))
    return _ORACLE[T, S, D]


_PLAN = {}                   # the launch plan of the last _run (Batch.plan)


def _run(ctx, recs, precision, mode, shared_from=None, iters=3):
    """recs: list of (X, Phi, g0, lp, Fa, Fb) on the chunked kernels (the fused per-chunk kernels at any T) with
    VBX_OPT_STREAM_LOADS = mode -> (results, did the streaming instances run)."""
    from vbx_amd import _capi
    batch = _capi.Batch(ctx, [r[0].shape[0] for r in recs], [r[2].shape[1] for r in recs], recs[0][0].shape[1],
                        precision=precision, max_iters=iters)
    try:
        batch.set_option(_capi.OPT_FB_ALGO, _capi.FB_CHUNKED)
        if shared_from is not None and batch.streams != 1:
            batch.set_option(_capi.OPT_STREAMS, 1)
        batch.set_stream_loads(mode)
        for k, (X, Phi, g0, lp, fa, fb) in enumerate(recs):
            S = g0.shape[1]
            if shared_from is not None and k != shared_from:
                batch.set_recording_shared(k, shared_from, np.ones(S) / S, g0, lp, fa, fb)
            else:
                batch.set_recording(k, X, Phi, np.ones(S) / S, g0, lp, fa, fb)
        batch.run(iters, -np.inf)
        _PLAN.clear()
        _PLAN.update(batch.plan)
        return [batch.result(k) for k in range(len(recs))], batch.stream_loads
    finally:
        batch.close()


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ('gamma', 'pi', 'Li'))


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('T,S,D', SHAPES)
def test_streaming_loads_change_no_bit(ctx, T, S, D, precision):
    X, Phi, g0 = _inputs(T, S, D)
    rec = (X, Phi, g0, 0.95, 0.3, 17.0)
    (on,), ran_on = _run(ctx, [rec], precision, 'on')
    (off,), ran_off = _run(ctx, [rec], precision, 'off')
    (auto,), ran_auto = _run(ctx, [rec], precision, 'auto')
    # what ran is reported: the split instances stream when asked, the others have no streaming form; a batch of this size
    # never streams by itself
    assert ran_on == (precision == 'fp32-split') and not ran_off and not ran_auto
    for k in ('gamma', 'pi', 'Li'):
        assert np.array_equal(on[k], off[k]), (k, float(np.abs(on[k] - off[k]).max()))
    assert _same(auto, off)
    g, pi, Li = _oracle(T, S, D)
    dg, dp, dl = float(np.abs(on['gamma'] - g).max()), float(np.abs(on['pi'] - pi).max()), rel_err(on['Li'], Li)
    print(f'T={T} S={S} D={D} {precision}: |gamma - oracle| {dg:.2e}  |pi - oracle| {dp:.2e}  Li rel {dl:.2e}')
    assert dg <= FP32_TOL and dp <= FP32_TOL and dl <= LI_RTOL


def test_a_ragged_batch_equals_its_recordings_alone_under_streaming_loads(ctx):
    """Three recordings of 129, 300 and 64 frames in one batch (tails of one frame, of 44 frames, of half a tile): each equal
    to its own single-recording run -- the tile -> rho tile offsets of a batch under the streaming instances."""
    recs = []
    for T in (129, 300, 64):
        X, Phi, g0 = _inputs(T, 30, 128)
        recs.append((X, Phi, g0, 0.95, 0.3, 17.0))
    together, ran = _run(ctx, recs, 'fp32-split', 'on')
    assert ran
    for k, rec in enumerate(recs):
        (alone,), ran = _run(ctx, [rec], 'fp32-split', 'on')
        assert ran and _same(together[k], alone), k


def test_a_sweep_on_a_shared_rho_equals_private_copies_under_streaming_loads(ctx):
    """Three points on one rho read their owner's f16 tiles (rho_tile0 / rho_row0): bit for bit what private copies give."""
    X, Phi, g0 = _inputs(700, 30, 128)
    recs = [(X, Phi, g0, lp, fa, fb) for lp, fa, fb in [(0.9, 0.3, 17.0), (0.9, 0.2, 6.0), (0.8, 0.4, 64.0)]]
    shared, ran_s = _run(ctx, recs, 'fp32-split', 'on', shared_from=0)
    private, ran_p = _run(ctx, recs, 'fp32-split', 'on')
    plain, ran_o = _run(ctx, recs, 'fp32-split', 'off', shared_from=0)
    assert ran_s and ran_p and not ran_o
    for a, b, c in zip(shared, private, plain):
        assert _same(a, b) and _same(a, c)


def test_forced_on_where_chunk_post_would_walk_the_last_level_itself(ctx):
    """One recording of T = 10 000, S = 30: a grouped boundary walk whose last level the small-batch instance of chunk_post
    runs itself (FOLD) under auto / off.  Forced on there is no such streaming instance: the last level becomes a launch of
    its own (scan2, the same arithmetic).  The results must not tell the difference."""
    X, Phi, g0 = _inputs(10000, 30, 128)
    rec = (X, Phi, g0, 0.95, 0.3, 17.0)
    (on,), ran_on = _run(ctx, [rec], 'fp32-split', 'on')
    assert _PLAN['walk_levels'] == 2 and not _PLAN['fold'] and _PLAN['stream']
    (off,), ran_off = _run(ctx, [rec], 'fp32-split', 'off')
    assert _PLAN['walk_levels'] == 2 and _PLAN['fold'] and not _PLAN['stream']
    assert ran_on and not ran_off
    for k in ('gamma', 'pi', 'Li'):
        assert np.array_equal(on[k], off[k]), (k, float(np.abs(on[k] - off[k]).max()))


def test_the_option_takes_three_values_and_refuses_the_rest(ctx):
    from vbx_amd import _capi
    batch = _capi.Batch(ctx, [300], [4], 128, precision='fp32-split', max_iters=2)
    try:
        for bad in (-1, 3, 17):
            with pytest.raises(_capi.VbxError, match='VBX_OPT_STREAM_LOADS'):
                batch.set_option(_capi.OPT_STREAM_LOADS, bad)
        with pytest.raises(ValueError):
            batch.set_stream_loads('always')
        X, Phi, g0 = _inputs(300, 4, 128)
        batch.set_recording(0, X, Phi, np.ones(4) / 4, g0, 0.9, 0.3, 17.0)
        assert not batch.stream_loads                        # (nothing has run yet)
        seen = []
        for mode in ('on', 'off', 'auto', 'on'):             # the option may change between the runs of one batch
            batch.set_stream_loads(mode)
            batch.run(1, -np.inf)
            seen.append(batch.stream_loads)
        assert seen == [True, False, False, True]
    finally:
        batch.close()
