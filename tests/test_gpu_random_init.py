"""``--init random_N`` on the device (-m gpu): the label kernel against the referee of tests/random_init_ref.py bit for bit, the
batch entry against ``set_recording_resident`` fed with the referee's labels bit for bit, the restarts and their winner, and the
three command lines in fresh child processes.

The recordings of the batch tests: T = 17, 257 and 1025 rows of D = 128 from ``frontend_ref.make_case`` (seeded), its input
rows replaced by six seeded speaker centres plus noise in turns of a few rows -- six speakers for four states, so the restarts
end in different optima whose ELBOs lie far apart (CPU oracle, oracle/vbx_oracle.py, on the float64 projection of these rows
when the test was written: the best two of the five restarts differ by 9.6, 752 and 2720; the bound below is 1e-9).  Purely
random rows would not do: every restart then collapses onto one speaker and all five ELBOs agree to rounding.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import diarize_util as du
import frontend_ref as fr
import random_init_ref as ref
import tune_util as tu

pytestmark = pytest.mark.gpu
REPO = du.REPO
ENV = dict(os.environ, PYTHONPATH=REPO)

# ---- the kernel ------------------------------------------------------------------------------------------------------
KERNEL_T = [1, 3, 4, 5, 1023, 1024, 1025, 4099]
KERNEL_N = [1, 2, 3, 7, 16, 64, 65, 1000]
KERNEL_SEEDS = [7, (1 << 32) + 0x9E3779B9]
KERNEL_RESTARTS = [0, 3]
KERNEL_NAMES = ['recA', 'dev000']                            # hashes with the top bit clear and set
GUARD, SENTINEL = 32, -0x5A5A5A5B


@pytest.fixture(scope='module')
def ctx():
    from vbx_amd import _capi
    return _capi.default_context(0)


def test_the_names_of_the_kernel_test_hash_either_side_of_the_top_bit():
    assert [ref.name_hash(n) >> 63 for n in KERNEL_NAMES] == [0, 1] and KERNEL_SEEDS[1] >= 1 << 32


@pytest.mark.parametrize('T', KERNEL_T)
def test_labels_equal_the_referees_and_the_guard_bands_stay_untouched(T, ctx):
    from vbx_amd import _capi
    for seed in KERNEL_SEEDS:
        for name in KERNEL_NAMES:
            h = ref.name_hash(name)
            for restart in KERNEL_RESTARTS:
                w = ref.words(seed, h, restart, T)
                for N in KERNEL_N:
                    want = np.array([(x * N) >> 64 for x in w], dtype=np.int32)
                    buf = np.full(T + 2 * GUARD, SENTINEL, dtype=np.int32)
                    got = _capi.random_labels(ctx, seed, h, restart, T, N, out=buf[GUARD:GUARD + T])
                    assert np.array_equal(got, want), (seed, name, restart, N, int(np.argmax(got != want)))
                    assert np.all(buf[:GUARD] == SENTINEL) and np.all(buf[GUARD + T:] == SENTINEL), (seed, name, restart, N)
                    assert np.array_equal(buf[GUARD:GUARD + T], want)


def test_a_call_without_out_returns_the_same_labels(ctx):
    from vbx_amd import _capi
    got = _capi.random_labels(ctx, 7, ref.name_hash('recA'), 1, 1025, 4)
    assert got.dtype == np.int32 and np.array_equal(got, ref.labels(7, 'recA', 1, 1025, 4))


# ---- the batch entry -------------------------------------------------------------------------------------------------
REC_T = [17, 257, 1025]
REC_NAMES = ['recA', 'recB', 'recC']
N_STATES, SEED, SMOOTHING = 4, 7, 5.0
HYPER = dict(loopProb=0.5, Fa=1.0, Fb=1.0)
CASE_SEED, N_SPEAKERS, NOISE = 2308, 6, 0.2
SWEEP_BOUND = 1e-12          # tests/test_gpu_parity.py::test_python_sweep_api_equals_one_call_per_point: rtol=0, atol=1e-12


def make_recordings_case():
    """The inputs of ``XVectors``: make_case's transforms; x = speaker centre + noise, turns of 2-3 rows in the short
    recording and 3-11 rows in the others, never the same speaker twice in a row."""
    c = fr.make_case((sum(REC_T), 40, 128, 128, np.float64), seed=CASE_SEED)
    rng = np.random.default_rng(CASE_SEED + 1)
    centers = rng.standard_normal((N_SPEAKERS, 40))
    spk = []
    for t in REC_T:
        s, last = [], -1
        while len(s) < t:
            v = int(rng.integers(0, N_SPEAKERS))
            if v == last:
                continue
            last = v
            s += [v] * int(rng.integers(2, 4) if t < 100 else rng.integers(3, 12))
        spk += s[:t]
    c['x'] = centers[np.array(spk)] + NOISE * rng.standard_normal((sum(REC_T), 40))
    return c


@pytest.fixture(scope='module')
def recs(ctx):
    """The three recordings resident on the device, the driver's stages on them, and every referee label: made once, read only."""
    from vbx_amd import _capi, vbhmm
    c = make_recordings_case()
    xv = _capi.XVectors(ctx, c['x'], c['mean1'], c['lda'], c['mean2'], c['plda_mu'], c['plda_tr'], c['fea_dim'])
    Phi = np.random.default_rng(128).uniform(0.5, 3.0, 128)
    stages = vbhmm.DeviceStages(0)
    stages.project_device(REC_T, xv, dict(plda_psi=Phi), 128)
    row0 = np.concatenate([[0], np.cumsum(REC_T)])
    labels = {(k, r): ref.labels(SEED, REC_NAMES[k], r, REC_T[k], N_STATES) for k in range(3) for r in range(5)}
    yield dict(xv=xv, Phi=Phi, stages=stages, row0=row0, labels=labels)
    stages.close()


def _fetch(batch, slots):
    out = []
    for b in slots:
        res = batch.result(b, want_model=False)
        first, second = batch.labels(b)
        out.append(dict(gamma=res['gamma'], pi=res['pi'], Li=res['Li'], n_iters=res['n_iters'], first=first, second=second))
    return out


def _assert_same_bits(got, want, tag):
    for key in ('gamma', 'pi', 'Li', 'first', 'second'):
        assert np.array_equal(got[key], want[key]), (tag, key)
    assert got['n_iters'] == want['n_iters'], tag


@pytest.fixture(scope='module')
def resident_run(ctx, recs):
    """One batch of the three recordings set with ``set_recording_resident`` from the referee's labels of restart 0, run as
    the driver runs it: the reference of the one-restart tests."""
    from vbx_amd import _capi
    batch = _capi.Batch(ctx, REC_T, [N_STATES] * 3, 128, precision='fp64', max_iters=40)
    try:
        for k in range(3):
            batch.set_recording_resident(k, recs['xv'], recs['row0'][k], recs['labels'][k, 0], SMOOTHING, recs['Phi'],
                                         HYPER['loopProb'], HYPER['Fa'], HYPER['Fb'])
        before = _fetch(batch, range(3))
        batch.run(40, 1e-6)
        return before, _fetch(batch, range(3))
    finally:
        batch.close()


def test_one_restart_is_the_resident_setter_with_the_referees_labels_bit_for_bit(ctx, recs, resident_run):
    from vbx_amd import _capi
    want0, want = resident_run
    batch = _capi.Batch(ctx, REC_T, [N_STATES] * 3, 128, precision='fp64', max_iters=40)
    try:
        for k in range(3):
            batch.set_recording_random(k, recs['xv'], recs['row0'][k], -1, SEED, ref.name_hash(REC_NAMES[k]), 0, SMOOTHING,
                                       recs['Phi'], HYPER['loopProb'], HYPER['Fa'], HYPER['Fb'])
        got0 = _fetch(batch, range(3))
        batch.run(40, 1e-6)
        got = _fetch(batch, range(3))
    finally:
        batch.close()
    for k in range(3):
        q0, _, _ = fr.qinit_ref(recs['labels'][k, 0], N_STATES, SMOOTHING)
        assert np.array_equal(got0[k]['gamma'], q0) and got0[k]['n_iters'] == 0          # gamma0 over exactly N states
        assert np.array_equal(got0[k]['first'], recs['labels'][k, 0])
        _assert_same_bits(got0[k], want0[k], ('before', k))
        _assert_same_bits(got[k], want[k], ('after', k))
        assert 1 < got[k]['n_iters'] < 40 and len(set(got[k]['first'].tolist())) >= 2     # (the run is not a trivial one)


def test_the_driver_with_one_restart_reports_that_run(recs, resident_run):
    _, want = resident_run
    out = recs['stages'].vb_random([0, 1, 2], N_STATES, 1, SEED, REC_NAMES, init_smoothing=SMOOTHING, maxIters=40, epsilon=1e-6,
                                   precision='fp64', **HYPER)
    assert len(out) == 3
    for k, (first, second, n_iters, win, elbos) in enumerate(out):
        assert np.array_equal(first, want[k]['first']) and np.array_equal(second, want[k]['second'])
        assert n_iters == want[k]['n_iters'] and win == 0 and elbos == [want[k]['Li'][-1]]
    # a subset in another order: every recording keeps its result (one batch of other members: the same bits are not promised
    # for gamma by the forward-backward choice, so this holds the labels of the longest recording only)
    sub = recs['stages'].vb_random([2], N_STATES, 1, SEED, ['recC'], init_smoothing=SMOOTHING, maxIters=40, epsilon=1e-6,
                                   precision='fp64', **HYPER)
    assert np.array_equal(sub[0][0], want[2]['first']) and sub[0][2] == want[2]['n_iters']


@pytest.mark.parametrize('streams', [1, 2, 3])
def test_restarts_share_one_rho_as_shared_slots_fed_with_the_referees_responsibilities(streams, ctx, recs):
    """Recordings x restarts in one batch, on one stream and on stream groups (where a sub-batch without the owner gets a copy
    of its rows): restart 0 owns, the others share -- against the same batch set with ``set_recording_resident`` and
    ``set_recording_shared`` from the referee's labels and responsibilities, bit for bit."""
    from vbx_amd import _capi
    R, ks = 3, [0, 1, 2]
    T = [REC_T[k] for k in ks for _ in range(R)]
    runs = {}
    for how in ('random', 'host'):
        batch = _capi.Batch(ctx, T, [N_STATES] * len(T), 128, precision='fp64', max_iters=40, streams=streams)
        try:
            assert batch.streams == streams
            for j, k in enumerate(ks):
                for r in range(R):
                    b = j * R + r
                    if how == 'random':
                        batch.set_recording_random(b, recs['xv'], recs['row0'][k], -1 if r == 0 else j * R, SEED,
                                                   ref.name_hash(REC_NAMES[k]), r, SMOOTHING, recs['Phi'], HYPER['loopProb'],
                                                   HYPER['Fa'], HYPER['Fb'])
                    elif r == 0:
                        batch.set_recording_resident(b, recs['xv'], recs['row0'][k], recs['labels'][k, 0], SMOOTHING, recs['Phi'],
                                                     HYPER['loopProb'], HYPER['Fa'], HYPER['Fb'])
                    else:
                        q0, _, _ = fr.qinit_ref(recs['labels'][k, r], N_STATES, SMOOTHING)
                        batch.set_recording_shared(b, j * R, np.full(N_STATES, 1.0 / N_STATES), q0, HYPER['loopProb'], HYPER['Fa'],
                                                   HYPER['Fb'])
            batch.run(40, 1e-6)
            runs[how] = _fetch(batch, range(len(T)))
        finally:
            batch.close()
    for b in range(len(T)):
        _assert_same_bits(runs['random'][b], runs['host'][b], (streams, b))
    assert len({runs['random'][b]['Li'][-1] for b in range(R)}) > 1          # (the restarts are different runs)


def test_bad_arguments_are_refused_and_the_batch_stays_usable(ctx, recs):
    from vbx_amd import _capi
    batch = _capi.Batch(ctx, [17, 17, 257], [N_STATES] * 3, 128, precision='fp64', max_iters=2)
    try:
        args = (SEED, 5, 0, SMOOTHING, recs['Phi'], 0.5, 1.0, 1.0)
        with pytest.raises(_capi.VbxError, match='has not been set'):
            batch.set_recording_random(1, None, 0, 0, *args)
        batch.set_recording_random(0, recs['xv'], 0, -1, *args)
        with pytest.raises(_capi.VbxError, match='out of range'):
            batch.set_recording_random(0, None, 0, 0, *args)                         # itself
        with pytest.raises(_capi.VbxError, match='not in the resident'):
            batch.set_recording_random(2, recs['xv'], sum(REC_T) - 100, -1, *args)   # rows past the end
        with pytest.raises(_capi.VbxError, match='negative'):
            batch.set_recording_random(1, None, 0, 0, SEED, 5, -1, SMOOTHING, None, 0.5, 1.0, 1.0)
        with pytest.raises(_capi.VbxError, match='frames'):
            batch.set_recording_random(2, None, 0, 0, *args)                         # 257 frames on a source of 17
        batch.set_recording_random(1, None, 0, 0, SEED, 5, 1, SMOOTHING, None, 0.5, 1.0, 1.0)
        batch.set_recording_random(2, recs['xv'], 17, -1, *args)
        batch.run(2, -np.inf)
        assert [batch.n_iters(b) for b in range(3)] == [2, 2, 2]
    finally:
        batch.close()


# ---- restarts --------------------------------------------------------------------------------------------------------
def test_five_restarts_the_winner_and_every_restarts_stand_alone_run(ctx, recs):
    import vbx_amd
    from vbx_amd import _capi
    R = 5
    out = recs['stages'].vb_random([0, 1, 2], N_STATES, R, SEED, REC_NAMES, init_smoothing=SMOOTHING, maxIters=40, epsilon=1e-6,
                                   precision='fp64', **HYPER)
    # the batch itself, as the driver builds it: what it returns is what the driver must have judged by
    T = [REC_T[k] for k in range(3) for _ in range(R)]
    batch = _capi.Batch(ctx, T, [N_STATES] * len(T), 128, precision='fp64', max_iters=40)
    try:
        for k in range(3):
            for r in range(R):
                batch.set_recording_random(k * R + r, recs['xv'], recs['row0'][k], -1 if r == 0 else k * R, SEED,
                                           ref.name_hash(REC_NAMES[k]), r, SMOOTHING, recs['Phi'], HYPER['loopProb'], HYPER['Fa'],
                                           HYPER['Fb'])
        batch.run(40, 1e-6)
        slots = _fetch(batch, range(len(T)))
    finally:
        batch.close()
    failures = []
    for k, (first, second, n_iters, win, elbos) in enumerate(out):
        mine = slots[k * R:(k + 1) * R]
        final = [float(s['Li'][-1]) for s in mine]
        print(f'{REC_NAMES[k]}: final ELBOs {final}, iterations {[s["n_iters"] for s in mine]}, winner {win}')
        assert elbos == final and win == ref.best_restart(final)
        assert np.array_equal(first, mine[win]['first']) and np.array_equal(second, mine[win]['second']) and n_iters == mine[win]['n_iters']
        top = sorted(final)
        gap = top[-1] - top[-2]
        print(f'{REC_NAMES[k]}: the best two restarts differ by {gap:.3e}')
        assert gap >= 1000 * SWEEP_BOUND, (k, gap)                # the winner is no rounding accident
        fea = recs['xv'].get('fea', int(recs['row0'][k]), REC_T[k])
        for r in range(R):
            q0, _, _ = fr.qinit_ref(recs['labels'][k, r], N_STATES, SMOOTHING)
            _g, _pi, Li = vbx_amd.VBx(fea, recs['Phi'], pi=N_STATES, gamma=q0, maxIters=40, epsilon=1e-6, precision='fp64', **HYPER)
            alone = float(np.asarray(Li)[-1][0]) if np.ndim(Li[-1]) else float(Li[-1])
            print(f'{REC_NAMES[k]} restart {r}: in the batch {final[r]!r}, alone {alone!r}, difference {abs(final[r] - alone):.3e}')
            if not abs(final[r] - alone) <= SWEEP_BOUND:
                failures.append((REC_NAMES[k], r, final[r], alone))
    assert not failures, failures


# ---- the command lines, in fresh child processes ---------------------------------------------------------------------
def _child(module_argv, timeout=300):
    res = subprocess.run([sys.executable, '-m'] + module_argv, env=ENV, cwd=REPO, capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-3000:]
    return res


@pytest.fixture(scope='module')
def dev_set(tmp_path_factory):
    """Three recordings of 150 x-vectors with reference turns (tests/tune_util.py), and the same archive in reverse order."""
    from vbx_amd import kaldi_formats as kf
    tmp = tmp_path_factory.mktemp('random_init')
    p = tu.make_dev_set(tmp, 3, 150, seed=5)
    groups = kf.read_vec_flt_ark_grouped(p['ark'])
    assert [g[0] for g in groups] == p['names']
    p['ark_reversed'] = os.path.join(str(tmp), 'dev_reversed.ark')
    kf.write_vec_flt_ark(p['ark_reversed'], [(key, x) for _name, keys, xs in reversed(groups) for key, x in zip(keys, xs)])
    assert [g[0] for g in kf.read_vec_flt_ark_grouped(p['ark_reversed'])] == p['names'][::-1]
    p['tmp'] = str(tmp)
    return p


# Fa 0.3, Fb 1: at the recipes' Fb 17 the best restart of 150 x-vectors from random labels is the one that puts everything
# on one speaker (CPU oracle); with the speaker prior this weak the restarts keep three or four and differ from each other
def _vbhmm(p, ark, out, extra, hyper=('--Fa', '0.3', '--Fb', '1', '--loopP', '0.9')):
    return _child(['vbx_amd.vbhmm', '--out-rttm-dir', out, '--xvec-ark-file', ark, '--segments-file', p['seg'], '--xvec-transform',
                   p['transform'], '--plda-file', p['plda'], '--threshold', '-0.015', '--lda-dim', '128'] + list(hyper) + list(extra))


def test_vbhmm_writes_the_same_bytes_twice_and_with_the_archive_reversed(dev_set, tmp_path):
    extra = ['--init', 'random_4', '--random-restarts', '3', '--seed', '7', '--output-2nd', 'True']
    outs = []
    for tag, ark in (('a', dev_set['ark']), ('b', dev_set['ark']), ('r', dev_set['ark_reversed'])):
        res = _vbhmm(dev_set, ark, str(tmp_path / tag), extra)
        assert res.stderr.count('runs no AHC') == 1
        outs.append((du.rttm_dir(str(tmp_path / tag)), du.rttm_dir(str(tmp_path / tag) + '2nd')))
    first, second = outs[0]
    assert sorted(first) == [n + '.rttm' for n in dev_set['names']] and sorted(second) == sorted(first)
    assert all(du.rttm_speakers_and_lines(data)[0] >= 2 for data in first.values())
    assert any(second[f] != first[f] for f in first)
    assert outs[1] == outs[0] and outs[2] == outs[0]


def test_diarize_writes_the_bytes_of_predict_and_vbhmm(tmp_path):
    p = du.write_corpus(tmp_path, du.standard_corpus())
    p.update(du.write_models(tmp_path), ckpt=du.write_checkpoint(tmp_path))
    ark, seg, two, one = (str(tmp_path / f) for f in ('x.ark', 'x.seg', 'two', 'one'))
    hyper = ['--threshold', '0.0', '--lda-dim', '128', '--Fa', '4.0', '--Fb', '1.0', '--loopP', '0.99']
    extra = ['--init', 'random_4', '--random-restarts', '2', '--seed', '3', '--output-2nd', 'True']
    _child(['vbx_amd.predict', '--gpus', '0', '--checkpoint', p['ckpt'], '--in-file-list', p['list'], '--in-lab-dir', p['lab'],
            '--in-wav-dir', p['wav'], '--out-ark-fn', ark, '--out-seg-fn', seg, '--batch-size', '16'])
    _child(['vbx_amd.vbhmm', '--out-rttm-dir', two, '--xvec-ark-file', ark, '--segments-file', seg, '--xvec-transform', p['transform'],
            '--plda-file', p['plda']] + hyper + extra)
    _child(['vbx_amd.diarize', '--gpus', '0', '--checkpoint', p['ckpt'], '--in-file-list', p['list'], '--in-lab-dir', p['lab'],
            '--in-wav-dir', p['wav'], '--batch-size', '16', '--out-rttm-dir', one, '--xvec-transform', p['transform'], '--plda-file',
            p['plda']] + hyper + extra)
    want, want2 = du.rttm_dir(two), du.rttm_dir(two + '2nd')
    assert sorted(want) == ['recA.rttm', 'recB.rttm', 'recC.rttm'] and sorted(want2) == sorted(want)
    assert du.rttm_dir(one) == want and du.rttm_dir(one + '2nd') == want2


TUNE_GRID = ['--Fa', '0.3', '1.0', '--Fb', '1', '17', '--loopP', '0.9']


def test_tune_scores_the_labels_vbhmm_writes_at_the_best_point(dev_set, tmp_path):
    extra = ['--init', 'random_3', '--random-restarts', '2', '--seed', '7']
    res = _child(['vbx_amd.tune'] + tu.data_argv(dev_set) + TUNE_GRID + extra + ['--best-rttm-dir', str(tmp_path / 'best')])
    lines = res.stdout.splitlines()
    assert len(lines) == 1 + 4 + 1 and lines[0].split() == ['Fa', 'Fb', 'loopP', 'DER', 'Miss', 'FA', 'Conf']
    assert res.stderr.count('runs no AHC') == 1
    m = re.fullmatch(r'best: Fa=(\S+) Fb=(\S+) loopP=(\S+) DER=(\S+)', lines[-1])
    assert m, lines[-1]
    _vbhmm(dev_set, dev_set['ark'], str(tmp_path / 'out'), extra, hyper=('--Fa', m.group(1), '--Fb', m.group(2), '--loopP', m.group(3)))
    want = du.rttm_dir(str(tmp_path / 'out'))
    assert sorted(want) == [n + '.rttm' for n in dev_set['names']] and du.rttm_dir(str(tmp_path / 'best')) == want


def test_tune_without_init_prints_what_it_printed_before_the_flag_existed(dev_set):
    """tests/golden/tune_table_before_random_init.txt: the standard output of ``python -m vbx_amd.tune`` with these arguments on
    this development set from the commit before ``--init`` existed, captured on the device in the job that first ran this test."""
    want = open(os.path.join(REPO, 'tests', 'golden', 'tune_table_before_random_init.txt')).read()
    res = _child(['vbx_amd.tune'] + tu.data_argv(dev_set) + TUNE_GRID)
    assert res.stdout == want and 'warning' not in res.stderr
    same = _child(['vbx_amd.tune'] + tu.data_argv(dev_set) + TUNE_GRID + ['--init', 'AHC+VB'])
    assert same.stdout == want
