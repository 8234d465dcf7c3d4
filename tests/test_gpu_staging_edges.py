"""The staging loads of the per-chunk kernels at the edges of a tile -- -m gpu.

stage_to_lds (vbx_amd/csrc/vbx_device.hpp) and the alpha staging of the split chunk_loglik instances issue every load of
a round unconditionally -- a slot past the end of a short tile re-reads the tile's last vector -- and predicate only the
store; a full tile takes a path of its own without either.  The shapes are the smallest at which a clamped or predicated
tail can go wrong: recordings of 1, 7, 64, 65, 127 frames (less than one slot per thread, the half-tile cut and its
neighbours, one frame short of a tile), 128 (the full-tile path), 129, 192, 193 (a full tile followed by a tail of one
frame, of half a tile, of half a tile and a frame) and 272 frames (two full tiles and a tail of 16), with 2, 17, 30, 33 and
50 speakers (padded to 16, 32, 32, 64, 64 states: one, two and four vectors of a b row, every instance family), in
the three precisions.

Each recording runs alone and as the LAST member of a batch behind two recordings of 300 frames -- its tiles then sit
at the end of the frame-major arrays, where a load past the end of the tile would leave them, and behind tiles of other
recordings in LDS-sized strides.  The batched result must equal the lone one bit for bit (a recording's arithmetic does
not depend on its neighbours), and three iterations must agree with the float64 oracle at the bounds the existing
tests hold these paths to: fp64 and fp32 at the tolerances of
tests/test_gpu_parity.py::test_chunk_post_tile_shapes_against_the_oracle (imported from its parametrisation, with that
test's factor for more than 30 speakers), the split mode at tests/test_gpu_split.py's FP32_TOL -- test_gpu_parity.py
compares the split mode with nothing but itself --, and the split mode's ELBO at the relative bound
tests/test_gpu_stream_loads.py and test_gpu_split.py hold it to against the oracle (LI_RTOL).  In the split mode every
shape also runs with the streaming loads forced on, which is what puts batches of this size through the chunk_post
instance of the big batches.  (The chunked kernels are forced: the other users of stage_to_lds, scan1 / scan3 and the
wide scan, are exercised by the existing suite.)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = [1, 7, 64, 65, 127, 128, 129, 192, 193, 272]
SPEAKERS = [2, 17, 30, 33, 50]
PRECISIONS = ['fp64', 'fp32', 'fp32-split']
OTHERS = 300                 # frames of the two recordings in front of the one under test
ITERS = 3
LP, FA, FB = 0.95, 0.3, 17.0


def _tolerances():
    """{precision: tol} of test_chunk_post_tile_shapes_against_the_oracle, read from its parametrize mark; the split mode:
    the one bound tests/test_gpu_split.py holds it to; 'Li fp32-split': the split mode's relative bound on the ELBO."""
    import test_gpu_parity
    import test_gpu_split
    import test_gpu_stream_loads
    tol = {}
    for mark in test_gpu_parity.test_chunk_post_tile_shapes_against_the_oracle.pytestmark:
        if mark.name == 'parametrize' and mark.args[0] == 'precision,tol':
            tol.update(dict(mark.args[1]))
    assert set(tol) == {'fp64', 'fp32'}, tol
    assert test_gpu_stream_loads.LI_RTOL < test_gpu_split.FP32_TOL
    tol['fp32-split'] = test_gpu_split.FP32_TOL
    tol['Li fp32-split'] = test_gpu_stream_loads.LI_RTOL
    return tol


@pytest.fixture(scope='module')
def ctx():
    from vbx_amd import _capi
    return _capi.Context(0)


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


_INPUTS, _ORACLE = {}, {}


def _inputs(T, S):
    if (T, S) not in _INPUTS:
        from vbx_amd.synth import make_recording
        X, Phi, _ = make_recording(T, S, seed=1000 * S + T, kappa=0.05)
        g0 = np.random.default_rng(7 * T + S).gamma(1.0, size=(T, S))
        g0 /= g0.sum(1, keepdims=True)
        for a in (X, Phi, g0):
            a.setflags(write=False)
        _INPUTS[T, S] = (X, Phi, g0)
    return _INPUTS[T, S]


def _oracle(T, S):
    """ITERS iterations of the float64 oracle from the soft start of _inputs: computed once per shape, never changed."""
    if (T, S) not in _ORACLE:
        from oracle import vbx_oracle
        X, Phi, g0 = _inputs(T, S)
        g, pi, Li = vbx_oracle.VBx(X, Phi, loopProb=LP, Fa=FA, Fb=FB, pi=S, gamma=g0, maxIters=ITERS, epsilon=-np.inf)[:3]
        Li = np.array([x[0] for x in Li])
        for a in (g, pi, Li):
            a.setflags(write=False)
        _ORACLE[T, S] = (g, pi, Li)
    return _ORACLE[T, S]


def _run(ctx, shapes, precision, stream_loads=None):
    """One batch of the recordings `shapes` = [(T, S), ...] on the chunked kernels -> the result of the LAST one."""
    from vbx_amd import _capi
    batch = _capi.Batch(ctx, [t for t, _ in shapes], [s for _, s in shapes], 128, precision=precision, max_iters=ITERS)
    try:
        batch.set_option(_capi.OPT_FB_ALGO, _capi.FB_CHUNKED)
        if stream_loads is not None:
            batch.set_stream_loads(stream_loads)
        for k, (T, S) in enumerate(shapes):
            X, Phi, g0 = _inputs(T, S)
            batch.set_recording(k, X, Phi, np.ones(S) / S, g0, LP, FA, FB)
        batch.run(ITERS, -np.inf)
        assert stream_loads != 'on' or batch.stream_loads
        return batch.result(len(shapes) - 1)
    finally:
        batch.close()


@pytest.mark.parametrize('S', SPEAKERS)
@pytest.mark.parametrize('precision', PRECISIONS)
def test_tile_edges_alone_and_behind_other_recordings(ctx, precision, S):
    tols = _tolerances()
    tol = tols[precision]
    tol_li = tols.get('Li ' + precision, max(tol, 1e-10))
    # (more than 30 speakers a few iterations into a random start: the EM map amplifies f32 rounding more -- the factor
    #  test_chunk_post_tile_shapes_against_the_oracle gives its own bound; the split mode's bound is flat)
    tol_s = tol if (S <= 30 or precision == 'fp32-split') else 5 * tol
    modes = [None, 'on'] if precision == 'fp32-split' else [None]
    worst = [0.0, 0.0, 0.0]
    for T in FRAMES:
        g, pi, Li = _oracle(T, S)
        for mode in modes:
            alone = _run(ctx, [(T, S)], precision, mode)
            last = _run(ctx, [(OTHERS, S), (OTHERS, S), (T, S)], precision, mode)
            for k in ('gamma', 'pi', 'Li'):
                assert np.array_equal(alone[k], last[k]), (T, mode, k, float(np.abs(np.asarray(alone[k]) - np.asarray(last[k])).max()))
            dg, dp, dl = float(np.abs(alone['gamma'] - g).max()), float(np.abs(alone['pi'] - pi).max()), rel_err(alone['Li'], Li)
            worst = [max(w, d) for w, d in zip(worst, (dg, dp, dl))]
            assert dg <= tol_s and dp <= tol_s and dl <= tol_li, (T, mode, dg, dp, dl)
    print(f'S={S} {precision}: worst |gamma - oracle| {worst[0]:.2e}  |pi - oracle| {worst[1]:.2e}  Li rel {worst[2]:.2e}  (bound {tol_s:.0e})')
