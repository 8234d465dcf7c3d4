"""``--init RTTM`` / ``--init RTTM+VB`` on the device (-m gpu): ``vbx_turn_weights`` against the referee of
tests/turn_init_ref.py (labels and weights bit for bit, responsibilities within Q_TOL), ``Batch.set_recording_turns`` against the
upload of the referee's responsibilities through ``set_recording``, and the driver: the round trip on the example recording,
``--init RTTM`` alone, and ``tune`` without AHC.

Q_TOL = 1e-13 absolute: an entry of q is at most S + 2 correctly rounded float64 operations, entries are <= 1 and S <= 64
(64 * 2^-53 = 7e-15); the device's exp is not correctly rounded but within an ulp or two, which the bound still holds with room.
The largest difference is printed by every test that compares q; measured on one MI355X: 2.9e-15.
"""
import argparse
import os
import shutil

import numpy as np
import pytest

import frontend_ref as fr
import tune_util as tu
import turn_init_ref as ref
from test_turn_init_host import HAND, hand_case

pytestmark = pytest.mark.gpu
REPO = tu.REPO
GOLDEN = os.path.join(REPO, 'tests', 'golden')
Q_TOL = 1e-13
SMOOTHING = 5.0
TILE = 256                                                   # turns per LDS tile, windows per workgroup (vbx_turn_init.hpp)
GRID = 10000                                                 # the 10 ms grid of the random cases, in ticks

KERNEL_T = [1, 255, 256, 257]
KERNEL_N = [1, TILE, TILE + 1, 3 * TILE + 1]
KERNEL_S = [1, 2, 33, 64]
CASE_SEED = 2411


@pytest.fixture(scope='module')
def ctx():
    from vbx_amd import _capi
    return _capi.default_context(0)


def random_case(rng, T, N, S):
    """Windows and turns on the 10 ms grid: N turns dealt to the S speakers (a speaker may get none, turns of one speaker may
    overlap), sorted by (speaker, start); windows of 10 ms to 300 ms anywhere in a span the turns cover only in part."""
    span = max(60, 3 * N)
    spk = np.sort(rng.integers(0, S, size=N)).astype(np.int32)
    u = rng.integers(0, span, size=N)
    order = np.lexsort((u, spk))
    u = u[order].astype(np.int64) * GRID
    v = u + rng.integers(1, 12, size=N).astype(np.int64) * GRID
    a = rng.integers(0, span + 20, size=T).astype(np.int64) * GRID
    b = a + rng.integers(1, 31, size=T).astype(np.int64) * GRID
    return a, b, u, v, spk


def census(a, b, u, v, spk, S):
    """(rows with a tie for the largest d, rows with D == 0, windows that end where a turn begins)"""
    _labels, _w, d = ref.weights(a, b, u, v, spk, S)
    top = d.max(axis=1)
    ties = int(np.count_nonzero((top > 0) & ((d == top[:, None]).sum(axis=1) > 1)))
    return ties, int(np.count_nonzero(d.sum(axis=1) == 0)), int(np.count_nonzero(np.isin(b, u)))


def compare(ctx, a, b, u, v, spk, S, tag):
    """One call of the device entry against the referee.  -> the largest |q - q_ref|."""
    from vbx_amd import _capi
    labels, w, q = _capi.turn_weights(ctx, a, b, u, v, spk, S, SMOOTHING)
    want_labels, want_w, _d = ref.weights(a, b, u, v, spk, S)
    want_q = ref.qinit(want_w, SMOOTHING)
    assert labels.dtype == np.int32 and w.shape == q.shape == (len(a), S)
    assert np.array_equal(labels, want_labels), (tag, int(np.argmax(labels != want_labels)))
    assert np.array_equal(w, want_w), (tag, np.argwhere(w != want_w)[:3].tolist())
    diff = float(np.abs(q - want_q).max())
    assert diff <= Q_TOL, (tag, diff)
    return diff


@pytest.mark.parametrize('T', KERNEL_T)
def test_turn_weights_equal_the_referees_at_every_block_tile_and_padding_edge(T, ctx):
    rng = np.random.default_rng(CASE_SEED + T)
    worst, seen = 0.0, np.zeros(3, dtype=np.int64)
    for N in KERNEL_N:
        for S in KERNEL_S:
            a, b, u, v, spk = random_case(rng, T, N, S)
            if N > TILE and S <= 2:                          # a speaker whose turns span a tile boundary
                assert spk[TILE - 1] == spk[TILE]
            seen += census(a, b, u, v, spk, S)
            worst = max(worst, compare(ctx, a, b, u, v, spk, S, (T, N, S)))
    print(f'T={T}: max |q - q_ref| = {worst:.3e}; rows with a tie in d: {seen[0]}, with D == 0: {seen[1]}, with b_i == u_j: {seen[2]}')
    if T >= 255:                                             # (one window cannot show all three)
        assert np.all(seen > 0), seen.tolist()


def test_the_drawn_set_holds_ties_uncovered_windows_and_touching_edges():
    """The census of the whole drawn set, on the host: what the random cases are there for actually occurs in them."""
    seen = np.zeros(3, dtype=np.int64)
    for T in KERNEL_T:
        rng = np.random.default_rng(CASE_SEED + T)
        for N in KERNEL_N:
            for S in KERNEL_S:
                a, b, u, v, spk = random_case(rng, T, N, S)
                seen += census(a, b, u, v, spk, S)
    print('rows with a tie in d, with D == 0, with b_i == u_j:', seen.tolist())
    assert np.all(seen > 0)


@pytest.mark.parametrize('name', sorted(HAND))
def test_the_hand_worked_rows_at_the_first_and_the_last_window_of_a_block(name, ctx):
    from vbx_amd import _capi
    c = HAND[name]
    a1, b1, u, v, spk, S = hand_case(name)
    rng = np.random.default_rng(7)
    T = 2 * TILE
    a = rng.integers(0, 900, size=T).astype(np.int64) * GRID
    b = a + rng.integers(1, 200, size=T).astype(np.int64) * GRID
    at = [0, TILE - 1, TILE, T - 1]
    a[at], b[at] = a1[0], b1[0]
    labels, w, q = _capi.turn_weights(ctx, a, b, u, v, spk, S, SMOOTHING)
    for i in at:
        assert labels[i] == c['label'] and w[i].tolist() == c['w'], (name, i)
    worst = compare(ctx, a, b, u, v, spk, S, name)
    print(f'{name}: max |q - q_ref| = {worst:.3e}')


def test_outputs_may_be_left_out_and_bad_input_is_refused_with_a_device(ctx):
    from vbx_amd import _capi
    a, b, u, v, spk = random_case(np.random.default_rng(3), 300, 40, 5)
    full = _capi.turn_weights(ctx, a, b, u, v, spk, 5, SMOOTHING)
    for want in (('labels',), ('w',), ('q',), ('labels', 'q')):
        got = _capi.turn_weights(ctx, a, b, u, v, spk, 5, SMOOTHING, want=want)
        for key, x, y in zip(('labels', 'w', 'q'), got, full):
            assert (x is None) if key not in want else np.array_equal(x, y), (want, key)
    with pytest.raises(_capi.VbxError, match='out of order'):
        _capi.turn_weights(ctx, a, b, u[::-1], v[::-1], spk[::-1], 5, SMOOTHING)
    with pytest.raises(_capi.VbxError, match='outside'):
        _capi.turn_weights(ctx, a, b, u, v, spk, 4, SMOOTHING)
    assert np.array_equal(_capi.turn_weights(ctx, a, b, u, v, spk, 5, SMOOTHING)[2], full[2])


# ---- the batch entry -------------------------------------------------------------------------------------------------------
REC_T, REC_S, REC_TURN_MS = [257, 300], [3, 33], [(2000, 9000), (800, 2400)]
# (at the recipes' Fa 0.3, Fb 17 five iterations put all 300 windows of the 33-speaker recording on one speaker -- CPU oracle --
#  and equal labels would show little; with these every given speaker keeps windows: 3 and 33 first labels after 5 iterations)
HYPER = dict(loopProb=0.5, Fa=1.0, Fb=1.0)
ELBO_RTOL = 1e-9             # the fp64 path's bound on an ELBO (tests/test_gpu_ref_scoring.py holds trajectories to rtol 1e-7 / 1e-9)


def first_pass(T, S, rng, turn_ms):
    """Windows of 1.44 s every 0.24 s and a first-pass diarization of them: speakers in turns of ``turn_ms``, every second turn
    running 0.5 s into the next one (overlapped speech), and one stretch of 6 s that no turn covers."""
    a = (np.arange(T, dtype=np.int64) * 240000)
    b = a + 1440000
    end = int(b[-1])
    hole = (end // 3, end // 3 + 6000000)
    lines, t, k = [], 0, 0
    while t < end:
        dur = int(rng.integers(*turn_ms)) * 1000
        s = k % S if k < 2 * S else int(rng.integers(0, S))
        over = 500000 if k % 2 else 0
        lo, hi = t, min(t + dur + over, end)
        if lo < hole[1] and hi > hole[0]:                    # cut around the uncovered stretch
            hi = hole[0]
            t = hole[1] - dur
        if hi > lo:
            lines.append((lo / 1e6, (hi - lo) / 1e6, f'spk{s}'))
        t += dur
        k += 1
    u, v, spk, n = ref.prepare(lines)
    return a, b, u, v, spk.astype(np.int32), n


@pytest.fixture(scope='module')
def recs(ctx):
    from vbx_amd import _capi
    c = fr.make_case((sum(REC_T), 40, 128, 128, np.float64), seed=2412)
    rng = np.random.default_rng(2413)
    given = [first_pass(T, S, rng, ms) for T, S, ms in zip(REC_T, REC_S, REC_TURN_MS)]
    centers = rng.standard_normal((max(REC_S), 40))
    rows = []
    for (a, b, u, v, spk, S) in given:
        rows.append(centers[ref.weights(a, b, u, v, spk, S)[0]])
    c['x'] = np.concatenate(rows) + 0.3 * rng.standard_normal((sum(REC_T), 40))
    xv = _capi.XVectors(ctx, c['x'], c['mean1'], c['lda'], c['mean2'], c['plda_mu'], c['plda_tr'], c['fea_dim'])
    Phi = np.random.default_rng(128).uniform(0.5, 3.0, 128)
    yield dict(xv=xv, Phi=Phi, given=given, row0=[0, REC_T[0]])
    xv.close()


@pytest.mark.parametrize('k', [0, 1])
def test_set_recording_turns_is_the_upload_of_the_referees_responsibilities(k, ctx, recs):
    from vbx_amd import _capi
    a, b, u, v, spk, S = recs['given'][k]
    T = REC_T[k]
    assert S == REC_S[k]
    _labels, w, d = ref.weights(a, b, u, v, spk, S)
    assert np.count_nonzero((d > 0).sum(axis=1) > 1) > 0 and np.count_nonzero(d.sum(axis=1) == 0) > 0     # overlapped, uncovered
    q0 = ref.qinit(w, SMOOTHING)
    fea = recs['xv'].get('fea', recs['row0'][k], T)
    batch = _capi.Batch(ctx, [T, T], [S, S], 128, precision='fp64', max_iters=5)
    try:
        batch.set_recording_turns(0, recs['xv'], recs['row0'][k], a, b, u, v, spk, SMOOTHING, recs['Phi'], **HYPER)
        batch.set_recording(1, fea, recs['Phi'], np.full(S, 1.0 / S), q0, **HYPER)
        before = [batch.result(s, want_model=False)['gamma'] for s in (0, 1)]
        batch.run(5, -np.inf)
        res = [batch.result(s, want_model=False) for s in (0, 1)]
        lab = [batch.labels(s) for s in (0, 1)]
    finally:
        batch.close()
    diff = float(np.abs(before[0] - q0).max())
    print(f'T={T} S={S}: max |q - q_ref| in the batch = {diff:.3e}')
    assert diff <= Q_TOL and np.array_equal(before[1], q0)
    assert res[0]['n_iters'] == res[1]['n_iters'] == 5
    assert np.array_equal(lab[0][0], lab[1][0]) and np.array_equal(lab[0][1], lab[1][1])
    assert len(set(lab[0][0].tolist())) >= 2
    rel = np.abs(res[0]['Li'] - res[1]['Li']) / np.abs(res[1]['Li'])
    print(f'T={T} S={S}: ELBOs {res[0]["Li"].tolist()}, relative differences {rel.tolist()}')
    assert np.all(rel <= ELBO_RTOL)


def test_the_batch_entry_refuses_what_the_kernel_cannot_take(ctx, recs):
    from vbx_amd import _capi
    a, b, u, v, spk, S = recs['given'][0]
    batch = _capi.Batch(ctx, [REC_T[0]], [2], 128, precision='fp64', max_iters=2)
    try:
        with pytest.raises(_capi.VbxError, match='outside'):                       # three speakers into two states
            batch.set_recording_turns(0, recs['xv'], 0, a, b, u, v, spk, SMOOTHING, recs['Phi'], **HYPER)
        with pytest.raises(ValueError, match='windows'):
            batch.set_recording_turns(0, recs['xv'], 0, a[:-1], b[:-1], u, v, spk, SMOOTHING, recs['Phi'], **HYPER)
        two = np.minimum(spk, 1)
        order = np.lexsort((u, two))
        batch.set_recording_turns(0, recs['xv'], 0, a, b, u[order], v[order], two[order], SMOOTHING, recs['Phi'], **HYPER)
        batch.run(2, -np.inf)
        assert batch.n_iters(0) == 2
    finally:
        batch.close()


# ---- the driver on the example recording ---------------------------------------------------------------------------------
NAME = 'ES2005a'


@pytest.fixture(scope='module')
def example(es2005a_files):
    """The example recording behind the driver's stages.  es2005a.npz holds the PLDA projection ``fea`` and ahc_cases.npz the
    x-vectors after vbhmm.py:129; the maps between them are not committed, so the stages get stand-ins that give the same
    rows: identity transforms in front (the rows are unit vectors already) and the affine map x -> fea, which least squares
    recovers from the 1025 pairs to 1e-13."""
    from vbx_amd import vbhmm
    g, x = es2005a_files
    W = np.linalg.lstsq(np.hstack([x, np.ones((len(x), 1))]), g['fea'], rcond=None)[0]
    A = W[:128].T
    models = dict(mean1=np.zeros(128), lda=np.eye(128), mean2=np.zeros(128), plda_mu=-np.linalg.solve(A, W[128]), plda_tr=A,
                  plda_psi=g['Phi'])
    seg_names = np.array([f'{NAME}_{i:04d}' for i in range(len(x))])
    recordings = [(NAME, seg_names, x)]
    segs = {NAME: (seg_names, g['seg_times'])}
    stages = vbhmm.DeviceStages(0)

    def run(init, out, init_rttm_dir=None):
        args = argparse.Namespace(init=init, init_rttm_dir=init_rttm_dir, threshold=-0.015, lda_dim=128, Fa=float(g['Fa']),
                                  Fb=float(g['Fb']), loopP=float(g['loopProb']), init_smoothing=SMOOTHING, output_2nd=False,
                                  out_rttm_dir=str(out))
        if stages.xv is not None:                                # (injected stages: their rows are the caller's to release)
            stages.xv.close()
            stages.xv = None
        state, _timing = vbhmm.diarize_recordings(recordings, segs, models, args, stages, log=lambda *a: None)
        return state[NAME]

    yield dict(run=run, stages=stages, g=g)
    stages.close()


@pytest.fixture(scope='module')
def es2005a_files():
    return dict(np.load(os.path.join(GOLDEN, 'es2005a.npz'))), np.load(os.path.join(GOLDEN, 'ahc_cases.npz'))['es2005a/x']


def test_round_trip_ahc_rttm_then_rttm_vb_writes_what_ahc_vb_writes(example, tmp_path):
    """--init AHC, --init AHC+VB, then --init RTTM+VB from the AHC output: the third RTTM against the second, byte for byte
    AFTER RENAMING the second's speakers by their first appearance in the AHC output.  It is the renamed comparison because
    the AHC labels of this recording do not come out in order of first appearance (the first window is in cluster 22 of 31).

    The windows of this recording overlap (1.44 s every 0.24 s) and the written turns meet in the middle of an overlap
    (merge_adjacent_labels), so they do NOT coincide with window edges: of the 1025 rows 700 are one-hot and 7 resampled labels
    differ from the AHC labels (referee, on the host).  The VB-HMM still ends in the same labels from either start (CPU
    oracle: 12 iterations against 13, final ELBO -73432.62626823 against -73432.62626820)."""
    ahc = example['run']('AHC', tmp_path / 'ahc')
    assert np.abs(example['stages'].xv.get('fea', 0, 1025) - example['g']['fea']).max() < 1e-9        # the stand-in transforms
    vb = example['run']('AHC+VB', tmp_path / 'vb')
    again = example['run']('RTTM+VB', tmp_path / 'again', init_rttm_dir=str(tmp_path / 'ahc'))
    text = {k: open(tmp_path / k / f'{NAME}.rttm').read() for k in ('ahc', 'vb', 'again')}
    rename = ref.rename_by_first_appearance([l.split()[7] for l in text['ahc'].splitlines()])
    in_order = list(rename) == [str(i + 1) for i in range(len(rename))]
    print(f'AHC: {len(rename)} speakers, in order of first appearance: {in_order}; iterations {vb["n_iters"]} and {again["n_iters"]}')
    assert len(rename) == int(np.max(ahc['labels1st'])) + 1 > 2 and again['thr'] != again['thr'] and again['n_iters'] > 1
    renamed = []
    for line in text['vb'].splitlines(keepends=True):
        f = line.split(' ')
        f[7] = str(rename[f[7]] + 1)
        renamed.append(' '.join(f))
    assert text['again'] == ''.join(renamed)
    assert np.array_equal(again['labels1st'], np.array([rename[str(int(s) + 1)] for s in vb['labels1st']]))


def test_init_rttm_alone_writes_the_referees_labels_and_the_result_can_be_scored(example, tmp_path, capsys):
    import io
    from vbx_amd import score
    from vbx_amd.kaldi_formats import write_rttm
    from vbx_amd.vbhmm import merge_adjacent_labels
    first = tmp_path / 'first'
    first.mkdir()
    shutil.copy(os.path.join(GOLDEN, 'es2005a_ref.rttm'), first / f'{NAME}.rttm')
    st = example['run']('RTTM', tmp_path / 'out', init_rttm_dir=str(first))
    u, v, spk, S = ref.read(str(first), NAME)
    a, b = ref.windows(example['g']['seg_times'])
    want = ref.weights(a, b, u, v, spk, S)[0]
    assert S == 4 and len(set(want.tolist())) == 4
    assert np.array_equal(st['labels1st'], want) and st['labels2nd'] is None and st['n_iters'] == 0
    expected = io.StringIO()                                 # the referee's labels, written as the driver writes labels
    start, end = example['g']['seg_times'].T
    starts, ends, out_labels = merge_adjacent_labels(start, end, want)
    write_rttm(expected, NAME, out_labels, starts, ends)
    assert open(tmp_path / 'out' / f'{NAME}.rttm').read() == expected.getvalue() and expected.getvalue().count('SPEAKER') > 4
    capsys.readouterr()
    assert score.main(['-r', os.path.join(GOLDEN, 'es2005a_ref.rttm'), '-s', str(tmp_path / 'out' / f'{NAME}.rttm'), '--device', '0']) == 0
    table = capsys.readouterr().out
    assert NAME in table and 'OVERALL' in table


# ---- tune ------------------------------------------------------------------------------------------------------------------
def test_tune_searches_its_grid_from_the_given_diarization_without_ahc(tmp_path, monkeypatch, capsys):
    from vbx_amd import tune, vbhmm
    p = tu.make_dev_set(tmp_path, 2, 64, seed=9)
    first = tmp_path / 'first'
    first.mkdir()
    for name in p['names']:                                  # two speakers, 16 windows (3.84 s) each in turn
        (first / f'{name}.rttm').write_text(''.join(
            f'SPEAKER {name} 1 {3.84 * i:.3f} 3.840 <NA> <NA> {"ab"[i % 2]} <NA> <NA>\n' for i in range(5)))

    def no_ahc(self, *a, **k):
        raise AssertionError('--init RTTM+VB must not run AHC')
    monkeypatch.setattr(vbhmm.DeviceStages, 'ahc', no_ahc)
    rc = tune.main(tu.data_argv(p) + ['--Fa', '0.3', '1.0', '--Fb', '17', '--loopP', '0.9', '--init', 'RTTM+VB', '--init-rttm-dir',
                                      str(first)])
    out = capsys.readouterr()
    assert rc == 0, out.err
    lines = out.out.splitlines()
    assert len(lines) == 1 + 2 + 1 and lines[0].split() == ['Fa', 'Fb', 'loopP', 'DER', 'Miss', 'FA', 'Conf']
    assert [l.split()[:3] for l in lines[1:3]] == [['0.3', '17', '0.9'], ['1', '17', '0.9']]       # one row per grid point
    assert all(len(l.split()) == 7 and float(l.split()[3]) == float(l.split()[3]) for l in lines[1:3])
    assert lines[-1].startswith('best: ') and out.err.count('runs no AHC') == 1
