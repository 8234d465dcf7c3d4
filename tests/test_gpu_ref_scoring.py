"""Scoring VB-HMM iterations against reference labels on the device (vbx_score.hpp, vbx_batch_set_reference).

Kernels: vbx_amd.speaker_confusion against the NumPy block, every entry within 1e-12 of the sum of the absolute values of its
terms (the reordering bound T 2^-53 is below 3e-13 for the T used here and `log` is within an ulp on both sides).  Loop: the
history a run leaves, bit for bit against fresh runs, and its DER / cross-entropy against the oracle's DER() of the
responsibilities the same run returns WITHOUT labels."""
import numpy as np
import pytest

from ref_scoring_util import numpy_confusion

pytestmark = pytest.mark.gpu

GROUP = 8 * 128          # frames per partial block (kScoreGroupFrames); the frames go through LDS 32 at a time


@pytest.fixture(scope='module')
def ctx():
    from vbx_amd import _capi
    return _capi.default_context(0)


def _orc():
    from oracle import vbx_oracle
    return vbx_oracle


def _posteriors(T, S, seed, zeros=False):
    rng = np.random.default_rng(seed)
    q = rng.gamma(0.4, size=(T, S)) + 1e-9
    if zeros and S > 1:
        q[rng.random((T, S)) < 0.3] = 0.0
        q[np.arange(T), rng.integers(0, S, T)] += 0.5
        q[T // 2] = 0.0
        q[T // 2, S - 1] = 1.0                             # a row equal to a unit vector
    return q / q.sum(1, keepdims=True)


def _check_block(q, ref, precision, n_ref=None):
    import vbx_amd
    from vbx_amd import _capi
    if n_ref is None:
        got = vbx_amd.speaker_confusion(q, ref, precision=precision)
    else:
        got = _capi.default_context(0).score_posteriors(q, ref, n_ref=n_ref, precision=precision)
    held = q.astype(np.float32).astype(np.float64) if precision == 'fp32' else q
    want = numpy_confusion(held, ref, n_ref)
    onehot = np.zeros((len(ref), want.shape[1]))
    onehot[np.arange(len(ref)), ref] = 1.0
    scale = np.stack([onehot.T @ np.abs(held), onehot.T @ np.abs(np.log(held + np.nextafter(0, 1)))])
    assert got.shape == want.shape
    err = np.abs(got - want)
    print(f'T={len(ref)} S={q.shape[1]} R={want.shape[1]} {precision}: max err / bound = {(err / (1e-12 * scale + 1e-300)).max():.3e}')
    assert (err <= 1e-12 * scale).all(), (len(ref), q.shape[1], precision, float((err - 1e-12 * scale).max()))
    return got


FRAMES = [1, 31, 32, 33, 127, 128, 129, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP - 1, 2 * GROUP, 2 * GROUP + 1]
STATES = [(129, 1), (129, 15), (129, 16), (129, 17), (129, 30), (129, 64), (129, 65), (129, 100), (129, 300), (12, 1025)]


@pytest.mark.parametrize('precision', ['fp64', 'fp32'])
@pytest.mark.parametrize('T', FRAMES)
def test_confusion_block_at_every_frame_boundary(T, precision):
    q = _posteriors(T, 30, seed=T)
    ref = np.random.default_rng(T + 1).integers(0, 5, T)
    _check_block(q, ref, precision)


@pytest.mark.parametrize('precision', ['fp64', 'fp32'])
@pytest.mark.parametrize('T,S', STATES)
def test_confusion_block_at_every_state_count(T, S, precision):
    q = _posteriors(T, S, seed=S)
    ref = np.random.default_rng(S + 1).integers(0, 7, T)
    _check_block(q, ref, precision)


@pytest.mark.parametrize('precision', ['fp64', 'fp32'])
@pytest.mark.parametrize('kind', ['R1', 'R2', 'R64', 'empty_label', 'one_label_of_many', 'zeros_and_unit_row'])
def test_confusion_block_label_counts_and_exact_zeros(kind, precision):
    T, S = 700, 9
    rng = np.random.default_rng(len(kind))
    q = _posteriors(T, S, seed=3, zeros=kind == 'zeros_and_unit_row')
    n_ref = None
    if kind == 'R1':
        ref = np.zeros(T, dtype=int)
    elif kind == 'R2':
        ref = rng.integers(0, 2, T)
    elif kind == 'R64':
        ref = rng.integers(0, 64, T)
        ref[-1] = 63
    elif kind == 'empty_label':
        ref = rng.integers(0, 6, T)
        ref[ref == 2] = 4
        ref[-1] = 5
    elif kind == 'one_label_of_many':                         # all frames one label, the others keep zero rows
        ref, n_ref = np.full(T, 3), 11
    else:
        ref = rng.integers(0, 5, T)
    got = _check_block(q, ref, precision, n_ref)
    if kind == 'empty_label':
        assert not got[:, 2].any()
    if kind == 'one_label_of_many':
        assert got.shape == (2, 11, S) and not got[:, [0, 1, 2, 4, 10]].any()


def test_confusion_block_is_deterministic_and_rejects_what_it_cannot_take():
    import vbx_amd
    from vbx_amd import _capi
    q = _posteriors(2 * GROUP + 77, 30, seed=9, zeros=True)
    ref = np.random.default_rng(10).integers(0, 6, len(q))
    for precision in ('fp64', 'fp32'):
        a = vbx_amd.speaker_confusion(q, ref, precision=precision)
        b = vbx_amd.speaker_confusion(q, ref, precision=precision)
        assert a.tobytes() == b.tobytes()
    with pytest.raises(ValueError, match='64'):
        vbx_amd.speaker_confusion(q, np.full(len(q), 64))
    with pytest.raises(_capi.VbxError, match='n_ref'):
        _capi.default_context(0).score_posteriors(q, ref, n_ref=65)
    with pytest.raises(_capi.VbxError, match='outside'):
        _capi.default_context(0).score_posteriors(q, ref, n_ref=3)


# ------------------------------------------------------------------------------------ the iteration loop
SHAPES = [(700, 9), (129, 4), (1, 3), (1500, 14), (128, 16)]       # of test_ragged_batch_equals_individual_runs
LABELLED = (0, 3, 4)                                                # recordings 1 and 2 have no labels
MODES = [('fp64', 0), ('fp32', 0), ('fp32-split', 0), ('fp64', 3)]  # (precision, streams forced)


@pytest.fixture(scope='module')
def recordings():
    from vbx_amd.synth import make_recording
    recs = []
    for k, (T, S) in enumerate(SHAPES):
        X, Phi, labels = make_recording(T, S, seed=40 + k, kappa=0.1)
        g = np.random.default_rng(k).gamma(1.0, size=(T, S))
        recs.append((X, Phi, g / g.sum(1, keepdims=True), labels))
    return recs


def _batch(ctx, recordings, mode, which=None, labelled=LABELLED, max_iters=6, fb_algo=None):
    from vbx_amd import _capi
    which = list(range(len(SHAPES))) if which is None else which
    precision, streams = mode
    batch = _capi.Batch(ctx, [SHAPES[k][0] for k in which], [SHAPES[k][1] for k in which], 128, precision=precision,
                        max_iters=max_iters, streams=streams)
    if streams:
        assert batch.streams == min(streams, len(which))
    if fb_algo is not None:
        batch.set_option(_capi.OPT_FB_ALGO, fb_algo)
    for j, k in enumerate(which):
        X, Phi, g, labels = recordings[k]
        batch.set_recording(j, X, Phi, np.ones(SHAPES[k][1]) / SHAPES[k][1], g, 0.9, 0.3, 17.0)
        if k in labelled:
            batch.set_reference(j, labels)
    return batch


def _run(ctx, recordings, mode, runs, **kw):
    """results and score histories (None without labels) of every recording after run(n) for n in runs, on one batch"""
    batch = _batch(ctx, recordings, mode, **kw)
    try:
        for n in runs:
            batch.run(n, -np.inf)
        which = kw.get('which') or list(range(len(SHAPES)))
        res = [batch.result(j, want_model=False) for j in range(len(which))]
        conf = [batch.scores(j) if k in kw.get('labelled', LABELLED) else None for j, k in enumerate(which)]
        return res, conf
    finally:
        batch.close()


@pytest.fixture(scope='module')
def six(ctx, recordings):
    """ONE run(6) with labels per mode, shared by the tests below"""
    return {mode: _run(ctx, recordings, mode, [6]) for mode in MODES}


@pytest.mark.parametrize('mode', MODES, ids=str)
def test_labels_do_not_change_the_iteration(ctx, recordings, six, mode):
    from vbx_amd import _capi
    res, conf = six[mode]
    plain, none = _run(ctx, recordings, mode, [6], labelled=())
    assert none == [None] * len(SHAPES)
    for k in range(len(SHAPES)):
        for name in ('gamma', 'pi', 'Li'):
            assert res[k][name].tobytes() == plain[k][name].tobytes(), (mode, k, name)
        if k in LABELLED:
            R = int(recordings[k][3].max()) + 1
            assert conf[k].shape == (6, 2, R, SHAPES[k][1])
    batch = _batch(ctx, recordings, mode)
    try:
        with pytest.raises(_capi.VbxError, match='no reference labels'):
            batch.scores(1)
    finally:
        batch.close()


@pytest.mark.parametrize('mode', MODES, ids=str)
def test_every_slot_is_that_of_a_fresh_run_and_scores_what_that_run_returns(ctx, recordings, six, mode):
    _, conf6 = six[mode]
    from vbx_amd import der_from_confusion
    for n in range(1, 7):
        _, conf = _run(ctx, recordings, mode, [n])
        plain, _ = _run(ctx, recordings, mode, [n], labelled=())          # the responsibilities of the path without labels
        for k in LABELLED:
            assert len(conf[k]) == n
            assert conf[k][n - 1].tobytes() == conf6[k][n - 1].tobytes(), (mode, k, n)
            labels, T = recordings[k][3], SHAPES[k][0]
            for xent in (False, True):
                want = _orc().DER(plain[k]['gamma'], labels, xentropy=xent)
                got = der_from_confusion(conf6[k][n - 1], T, xentropy=xent)
                np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=str((mode, k, n, xent)))


@pytest.mark.parametrize('mode', MODES, ids=str)
def test_history_survives_between_runs(ctx, recordings, six, mode):
    _, conf = _run(ctx, recordings, mode, [2, 3])
    _, conf5 = _run(ctx, recordings, mode, [5])
    for k in LABELLED:
        assert len(conf[k]) == 5 and conf[k].tobytes() == conf5[k].tobytes(), (mode, k)
        assert conf5[k].tobytes() == six[mode][1][k][:5].tobytes(), (mode, k)


@pytest.mark.parametrize('mode', MODES, ids=str)
def test_a_recording_alone_gives_the_bits_it_gives_in_the_batch(ctx, recordings, six, mode):
    """The forward-backward algorithm follows the LONGEST recording of a (sub-)batch: the one-tile recording alone walks its
    frames sequentially, beside a long one it runs the chunked scan, and its responsibilities differ in the last bit between the
    two -- and with them the blocks.  So the algorithm is pinned (VBX_OPT_FB_ALGO) on both sides, on the batch of five -- on one
    stream and forced onto three, where each sub-batch would choose for itself -- and on the recording alone: then gamma AND the
    history are the same bits."""
    from vbx_amd import _capi
    res5, conf5 = _run(ctx, recordings, mode, [6], fb_algo=_capi.FB_CHUNKED)
    if not mode[1]:                                          # (one stream: the batch of five runs the chunked scan by itself)
        for k in LABELLED:
            assert conf5[k].tobytes() == six[mode][1][k].tobytes(), (mode, k)
    for k in LABELLED:
        res, conf = _run(ctx, recordings, mode, [6], which=[k], fb_algo=_capi.FB_CHUNKED)
        assert res[0]['gamma'].tobytes() == res5[k]['gamma'].tobytes(), (mode, k)
        assert conf[0].tobytes() == conf5[k].tobytes(), (mode, k)
        # measured, not asserted: each side left to choose its algorithm
        auto, conf_auto = _run(ctx, recordings, mode, [6], which=[k])
        print(mode, k, 'automatic choice, alone == in the batch: gamma', auto[0]['gamma'].tobytes() == six[mode][0][k]['gamma'].tobytes(),
              'history', conf_auto[0].tobytes() == six[mode][1][k].tobytes())


@pytest.mark.parametrize('mode', MODES, ids=str)
def test_the_batch_scores_what_the_stand_alone_step_scores(six, recordings, mode):
    """the last slot of every labelled recording, whatever batch and stream it ran in, against the same two kernels on the
    responsibilities the run returned: identical bits"""
    import vbx_amd
    res, conf = six[mode]
    for k in LABELLED:
        alone = vbx_amd.speaker_confusion(res[k]['gamma'], recordings[k][3], precision='fp64' if mode[0] == 'fp64' else 'fp32')
        assert alone.tobytes() == conf[k][5].tobytes(), (mode, k)


def test_batch_rows_have_three_columns_only_where_there_are_labels(recordings):
    from vbx_amd.batch import VBx_batch
    recs = []
    for k, (X, Phi, g, labels) in enumerate(recordings):
        rec = dict(X=X, Phi=Phi, pi=SHAPES[k][1], gamma=g)
        if k in LABELLED:
            rec['ref'] = labels
        recs.append(rec)
    out = VBx_batch(recs, maxIters=4, epsilon=-np.inf, loopProb=0.9, Fa=0.3, Fb=17.0)
    for k, (gamma, pi, Li) in enumerate(out):
        assert len(Li) == 4 and all(len(row) == (3 if k in LABELLED else 1) for row in Li), k
        if k in LABELLED:
            Lr = _orc().VBx(recordings[k][0], recordings[k][1], loopProb=0.9, Fa=0.3, Fb=17.0, pi=SHAPES[k][1], gamma=recordings[k][2],
                            maxIters=4, epsilon=-1e300, ref=recordings[k][3])[2]
            np.testing.assert_allclose(np.array(Li), np.array(Lr), rtol=1e-7, atol=1e-9)


def test_a_recording_that_stops_early_has_a_row_per_iteration_it_ran(ctx):
    import vbx_amd
    from vbx_amd import _capi
    from vbx_amd.synth import make_recording
    Xa, Phi, la = make_recording(450, 9, seed=14, kappa=0.3)
    Xb, _, lb = make_recording(600, 12, seed=3, kappa=0.05)
    ga = np.random.default_rng(20).gamma(1.0, size=(450, 9)); ga /= ga.sum(1, keepdims=True)
    gb = np.random.default_rng(11).gamma(1.0, size=(600, 12)); gb /= gb.sum(1, keepdims=True)
    kw = dict(loopProb=0.9, Fa=0.3, Fb=17.0, pi=9, gamma=ga, maxIters=30, epsilon=0.5)
    gr, pr, Lr = _orc().VBx(Xa, Phi, ref=la, **kw)
    assert 2 < len(Lr) < 30                                              # (it does stop early: 6 rows)
    gamma, pi, Li = vbx_amd.VBx(Xa, Phi, ref=la, **kw)
    assert len(Li) == len(Lr) and all(len(r) == 3 for r in Li)
    np.testing.assert_allclose(np.array(Li), np.array(Lr), rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(gamma, gr, rtol=0, atol=1e-7)
    # beside a recording that keeps iterating: as many valid slots as iterations it ran, the bits of the recording alone
    def scores(pair, eps):
        batch = _capi.Batch(ctx, [len(x) for x, *_ in pair], [g.shape[1] for _, g, _ in pair], 128, precision='fp64', max_iters=30)
        try:
            for j, (X, g, lab) in enumerate(pair):
                batch.set_recording(j, X, Phi, np.ones(g.shape[1]) / g.shape[1], g, 0.9, 0.3, 17.0)
                batch.set_reference(j, lab)
            batch.run(30, eps)
            return [(batch.n_iters(j), batch.scores(j)) for j in range(len(pair))]
        finally:
            batch.close()
    (n_alone, alone), = scores([(Xa, ga, la)], 0.5)
    assert n_alone == len(Lr) == len(alone)
    (na, ca), (nb, cb) = scores([(Xa, ga, la), (Xb, gb, lb)], 1e-4)
    assert len(ca) == na and len(cb) == nb and na != nb
    assert ca[:n_alone].tobytes() == alone.tobytes()
    # the one that stopped first kept rewriting its last slot with the same bits while the other went on
    (nb_alone, b_alone), = scores([(Xb, gb, lb)], 1e-4)
    assert nb_alone == nb and cb.tobytes() == b_alone.tobytes()


def test_set_reference_rejects_bad_labels_and_times_under_post(ctx, recordings):
    from vbx_amd import _capi
    X, Phi, g, labels = recordings[0]
    batch = _capi.Batch(ctx, [700], [9], 128, precision='fp32', max_iters=3)
    try:
        with pytest.raises(_capi.VbxError, match='has not been set'):
            batch.set_reference(0, labels)
        batch.set_recording(0, X, Phi, np.ones(9) / 9, g, 0.9, 0.3, 17.0)
        with pytest.raises(_capi.VbxError, match='n_ref'):
            batch.set_reference(0, labels, n_ref=65)
        with pytest.raises(_capi.VbxError, match='outside'):
            batch.set_reference(0, labels, n_ref=int(labels.max()))
        batch.profile_kernels()
        batch.run(3, -np.inf)
        plain = batch.kernel_times()['post'][1]
        batch.set_reference(0, labels)
        batch.run(3, -np.inf)
        assert batch.kernel_times()['post'][1] > plain
        assert len(_capi.K_NAMES) == 10
        batch.set_reference(0, None)                                     # cleared: the batch runs as it did before
        batch.run(3, -np.inf)
        assert batch.kernel_times()['post'][1] == plain
    finally:
        batch.close()


# ------------------------------------------------------------------------------------ sweeps
@pytest.mark.parametrize('streams', [None, '2'])
def test_sweep_points_are_scored_like_separate_calls_on_the_host(recordings, monkeypatch, streams):
    import vbx_amd
    from vbx_amd.batch import VBx_sweep
    X, Phi, g, labels = recordings[3]                                    # T = 1500, S = 14
    points = [dict(Fa=0.3, Fb=17.0, loopProb=0.9), dict(Fa=0.4, Fb=17.0, loopProb=0.9), dict(Fa=0.3, Fb=11.0, loopProb=0.99),
              dict(Fa=0.2, Fb=25.0, loopProb=0.8)]
    if streams:
        monkeypatch.setenv('VBX_AMD_SWEEP_STREAMS', streams)
    out = VBx_sweep(X, Phi, points, maxIters=5, epsilon=-np.inf, pi=14, gamma=g, ref=labels)
    monkeypatch.setenv('VBX_AMD_REF_SCORING', 'host')
    for p, (gamma, pi, Li) in zip(points, out):
        gs, ps, Ls = vbx_amd.VBx(X, Phi, pi=14, gamma=g, maxIters=5, epsilon=-np.inf, ref=labels, **p)
        assert len(Li) == len(Ls) == 5 and all(len(r) == 3 for r in Li)
        np.testing.assert_allclose(np.array(Li)[:, 1:], np.array(Ls)[:, 1:], rtol=1e-12, atol=0, err_msg=str(p))
        np.testing.assert_allclose(np.array(Li)[:, 0], np.array(Ls)[:, 0], rtol=1e-9, atol=0, err_msg=str(p))
