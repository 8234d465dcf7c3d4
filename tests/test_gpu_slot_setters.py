"""The seams between the six ways a batch slot is set (-m gpu): every setter over every setter, with a run in between and
with the first setting still enqueued; the device-side setters in a stream group on the clone route, the "already holds a
copy" route and on rows of their own; a refused call followed by a good one.

Every comparison is ``==`` on gamma, pi and the ELBOs of the slot against a FRESH batch of the same shape that was given the
final setting directly.  Shapes: T = 300 (three tiles of 128 frames, the last one partial), S = 3, D = 8, two iterations, fp64
and fp32.  Each setter has hyper-parameters and priors of its own, so that anything an earlier setting leaves behind shows.
The host stand-in of a device-side setter is the upload of the same rows and of the responsibilities the referees give
(tests/frontend_ref.py, tests/random_init_ref.py; for the turns ``turn_weights``, whose kernel the setter runs).
"""
import numpy as np
import pytest

import frontend_ref as fr
import random_init_ref as ref

pytestmark = pytest.mark.gpu

T, S, D, ITERS = 300, 3, 8, 2
SMOOTHING, SEED, NAME = 5.0, 11, 'recS'
PRECISIONS = ['fp64', 'fp32']
SETTERS = ['host', 'shared', 'resident', 'random_own', 'random_shared', 'turns']
DEVICE_SIDE = ['resident', 'random_own', 'random_shared', 'turns']
# (loopProb, Fa, Fb) of each setter, and of the source slot
HYPER = dict(host=(0.9, 0.3, 17.0), shared=(0.8, 0.4, 11.0), resident=(0.7, 0.5, 7.0), random_own=(0.6, 0.6, 5.0),
             random_shared=(0.5, 0.7, 3.0), turns=(0.4, 0.8, 2.0), source=(0.95, 1.0, 1.0))
UNIFORM = np.full(S, 1.0 / S)


@pytest.fixture(scope='module')
def ctx():
    from vbx_amd import _capi
    return _capi.default_context(0)


@pytest.fixture(scope='module')
def data(ctx):
    """Two recordings' rows resident on the device (the source slot reads the first T, a slot with rows of its own the
    second T) and everything the setters are fed with: made once, read only."""
    from vbx_amd import _capi
    c = fr.make_case((2 * T, 40, 16, D, np.float64), seed=2601)
    rng = np.random.default_rng(2602)
    spk = np.repeat(rng.integers(0, 4, size=2 * T // 10), 10)
    c['x'] = rng.standard_normal((4, 40))[spk] + 0.3 * rng.standard_normal((2 * T, 40))
    xv = _capi.XVectors(ctx, c['x'], c['mean1'], c['lda'], c['mean2'], c['plda_mu'], c['plda_tr'], c['fea_dim'])
    d = dict(xv=xv, Phi=rng.uniform(0.5, 3.0, D), fea=[xv.get('fea', 0, T), xv.get('fea', T, T)])
    for key in ('q_source', 'q_host', 'q_shared'):
        q = rng.gamma(1.0, size=(T, S))
        d[key] = q / q.sum(axis=1, keepdims=True)
    d['pi_host'], d['pi_shared'] = np.array([0.5, 0.3, 0.2]), np.array([0.2, 0.2, 0.6])
    d['labels'] = rng.integers(0, S, size=T).astype(np.int32)
    # windows of 1.44 s every 0.24 s; turns of 1 - 4 s, every second one running 0.5 s into the next, sorted by (speaker, start)
    a = np.arange(T, dtype=np.int64) * 240000
    cuts = np.concatenate([[0], np.cumsum(rng.integers(1000, 4000, size=60)) * 1000])
    u, v = cuts[:-1], cuts[1:] + 500000 * (np.arange(60) % 2)
    tspk = (np.arange(60) % S).astype(np.int32)
    order = np.lexsort((u, tspk))
    d['turns'] = (a, a + 1440000, u[order].astype(np.int64), v[order].astype(np.int64), tspk[order])
    d['q_turns'] = _capi.turn_weights(ctx, *d['turns'], S, SMOOTHING)[2]
    d['q_resident'] = fr.qinit_ref(d['labels'], S, SMOOTHING)[0]
    d['q_random'] = [fr.qinit_ref(ref.labels(SEED, NAME, r, T, S), S, SMOOTHING)[0] for r in range(4)]
    yield d
    xv.close()


def set_source(batch, d, slot=0, how='resident'):
    lp, fa, fb = HYPER['source']
    if how == 'resident':
        batch.set_recording_resident(slot, d['xv'], 0, d['labels'][::-1].copy(), SMOOTHING, d['Phi'], lp, fa, fb)
    else:
        batch.set_recording(slot, d['fea'][0], d['Phi'], UNIFORM, d['q_source'], lp, fa, fb)


def set_slot(how, batch, d, slot=1, src=0, restart=1, Fa=None):
    """Slot ``slot`` by the setter ``how``: rows of its own are the second T resident rows, a source is slot ``src``."""
    lp, fa, fb = HYPER[how]
    fa = fa if Fa is None else Fa
    if how == 'host':
        batch.set_recording(slot, d['fea'][1], d['Phi'], d['pi_host'], d['q_host'], lp, fa, fb)
    elif how == 'shared':
        batch.set_recording_shared(slot, src, d['pi_shared'], d['q_shared'], lp, fa, fb)
    elif how == 'resident':
        batch.set_recording_resident(slot, d['xv'], T, d['labels'], SMOOTHING, d['Phi'], lp, fa, fb)
    elif how == 'random_own':
        batch.set_recording_random(slot, d['xv'], T, -1, SEED, ref.name_hash(NAME), 0, SMOOTHING, d['Phi'], lp, fa, fb)
    elif how == 'random_shared':
        batch.set_recording_random(slot, None, 0, src, SEED, ref.name_hash(NAME), restart, SMOOTHING, None, lp, fa, fb)
    else:
        batch.set_recording_turns(slot, d['xv'], T, *d['turns'], SMOOTHING, d['Phi'], lp, fa, fb)


def set_slot_from_host(how, batch, d, slot, src=0, restart=1):
    """What the device-side setter ``how`` puts into a slot, uploaded through the two host setters."""
    lp, fa, fb = HYPER[how]
    if how == 'random_shared':
        batch.set_recording_shared(slot, src, UNIFORM, d['q_random'][restart], lp, fa, fb)
    else:
        q = dict(resident=d['q_resident'], random_own=d['q_random'][0], turns=d['q_turns'])[how]
        batch.set_recording(slot, d['fea'][1], d['Phi'], UNIFORM, q, lp, fa, fb)


def fetch(batch, slot):
    res = batch.result(slot, want_model=False)
    assert res['n_iters'] == ITERS
    return res


def assert_same_bits(got, want, tag):
    for key in ('gamma', 'pi', 'Li'):
        assert np.array_equal(got[key], want[key]), (tag, key, float(np.abs(got[key] - want[key]).max()))


@pytest.fixture(scope='module')
def fresh(ctx, data):
    """(precision, how the source slot is set, setter) -> slot 1 of a fresh batch after the run; each computed once."""
    from vbx_amd import _capi
    cache = {}

    def get(precision, source, how):
        key = (precision, source, how)
        if key not in cache:
            batch = _capi.Batch(ctx, [T, T], [S, S], D, precision=precision, max_iters=ITERS)
            try:
                set_source(batch, data, how=source)
                set_slot(how, batch, data)
                batch.run(ITERS, -np.inf)
                cache[key] = fetch(batch, 1)
            finally:
                batch.close()
        return cache[key]
    return get


def test_the_settings_differ_so_that_a_stale_one_would_show(fresh):
    runs = [fresh('fp64', 'resident', how) for how in SETTERS]
    assert len({float(r['Li'][-1]) for r in runs}) == len(SETTERS)


@pytest.mark.parametrize('first', SETTERS)
@pytest.mark.parametrize('precision', PRECISIONS)
def test_every_setter_over_every_setter_with_a_run_in_between(precision, first, ctx, data, fresh):
    from vbx_amd import _capi
    batch = _capi.Batch(ctx, [T, T], [S, S], D, precision=precision, max_iters=ITERS)
    try:
        set_source(batch, data)
        for second in SETTERS:
            set_slot(first, batch, data)
            batch.run(ITERS, -np.inf)
            assert_same_bits(fetch(batch, 1), fresh(precision, 'resident', first), (first, 'alone'))
            set_slot(second, batch, data)
            batch.run(ITERS, -np.inf)
            assert_same_bits(fetch(batch, 1), fresh(precision, 'resident', second), (first, second))
    finally:
        batch.close()


@pytest.mark.parametrize('first', SETTERS)
@pytest.mark.parametrize('precision', PRECISIONS)
def test_every_setter_over_every_setter_while_the_first_is_still_enqueued(precision, first, ctx, data, fresh):
    """Asynchronous uploads and no run in between: the source slot and the first setting of slot 1 are (where they are host
    uploads) still on their way when the second setting lands."""
    from vbx_amd import _capi
    batch = _capi.Batch(ctx, [T, T], [S, S], D, precision=precision, max_iters=ITERS)
    try:
        batch.set_async_upload(True)
        for second in SETTERS:
            set_source(batch, data, how='host')
            set_slot(first, batch, data)
            set_slot(second, batch, data)
            batch.run(ITERS, -np.inf)
            assert_same_bits(fetch(batch, 1), fresh(precision, 'host', second), (first, second))
    finally:
        batch.close()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_the_device_side_setters_in_a_stream_group_equal_the_uploads_of_their_responsibilities(precision, ctx, data):
    """Two streams, four slots.  Random labels on the rows of a source in the other sub-batch (a copy of the rows is made),
    then on a second slot of that sub-batch (which shares the copy), and beside the source; then the setters that bring rows
    of their own over those slots -- against the same group set through the host setters."""
    from vbx_amd import _capi
    runs = {}
    for side in ('device', 'host'):
        put = set_slot if side == 'device' else set_slot_from_host
        batch = _capi.Batch(ctx, [T] * 4, [S] * 4, D, precision=precision, max_iters=ITERS, streams=2)
        try:
            assert batch.streams == 2
            near = [i for i in range(4) if batch.stream_of(i) == 0]
            far = [i for i in range(4) if batch.stream_of(i) == 1]
            assert len(near) == len(far) == 2
            src, beside, (clone, sharer) = near[0], near[1], far
            set_source(batch, data, slot=src)
            put('random_shared', batch, data, slot=clone, src=src, restart=1)
            put('random_shared', batch, data, slot=sharer, src=src, restart=2)
            put('random_shared', batch, data, slot=beside, src=src, restart=3)
            batch.run(ITERS, -np.inf)
            runs[side, 'shared'] = [fetch(batch, i) for i in (clone, sharer, beside)]
            put('resident', batch, data, slot=clone)             # (the sharer loses the copy it read and is set again)
            put('turns', batch, data, slot=sharer)
            put('random_own', batch, data, slot=beside)
            batch.run(ITERS, -np.inf)
            runs[side, 'own'] = [fetch(batch, i) for i in (clone, sharer, beside)]
        finally:
            batch.close()
    for phase in ('shared', 'own'):
        for k in range(3):
            assert_same_bits(runs['device', phase][k], runs['host', phase][k], (phase, k))
    assert len({float(r['Li'][-1]) for r in runs['device', 'shared'] + runs['device', 'own']}) == 6


@pytest.mark.parametrize('how', SETTERS)
@pytest.mark.parametrize('precision', PRECISIONS)
def test_a_refused_call_leaves_the_slot_usable(precision, how, ctx, data, fresh):
    from vbx_amd import _capi
    batch = _capi.Batch(ctx, [T, T], [S, S], D, precision=precision, max_iters=ITERS)
    try:
        set_source(batch, data)
        with pytest.raises(_capi.VbxError, match='must be positive'):
            set_slot(how, batch, data, Fa=0.0)
        set_slot(how, batch, data)
        batch.run(ITERS, -np.inf)
        assert_same_bits(fetch(batch, 1), fresh(precision, 'resident', how), how)
    finally:
        batch.close()
