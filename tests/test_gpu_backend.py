"""Backend training end to end on the device (-m gpu): ``train_backend`` against the numpy recipe of tests/backend_ref.py on a
synthetic two-covariance training set, the trained files through the chain's own stages on a held-out recording, the command
line, and the refusal of a row without length.

The training set: K = 60 speakers with 1 ... 12 rows each (N = 390), Din = 24, lda_dim = 8 (backend_ref.World, seed
backend_ref.E2E_SEED: chosen on the CPU, where tests/test_backend_host.py holds the host chain to zero errors on it).

Tolerance of the model comparison, computed here and never taken from the code under test: 32 * e0 + C_TOL * N * 2^-53, where
e0 is the largest relative distance between the reference trained on the rows and on three random permutations of them (its own
sensitivity through the eigensolvers: 1.4e-14 ... 3.8e-14 on this generator, depending on seed and host) and the second term is the statistics bound of
tests/test_gpu_backend_kernels.py for a sum of N terms, relative to the sum of the terms' magnitudes (8.7e-14).
Measured on one MI355X: DESIGN section 25.
"""
import argparse

import numpy as np
import pytest

import backend_ref as ref
from test_gpu_backend_kernels import C_TOL, U

pytestmark = pytest.mark.gpu
FIELDS = ('mean1', 'lda', 'mean2', 'mean', 'W', 'B')


@pytest.fixture(scope='module')
def trained():
    """The training set, the held-out recording, the reference's model and the device's."""
    from vbx_amd import backend
    world = ref.World(ref.E2E_SEED)
    x, spk = world.training_set()
    rec, truth = world.recording()
    want = ref.train(x, spk, ref.LDA_DIM)
    got = backend.train_backend(x, spk, ref.LDA_DIM, device=0)
    return dict(x=x, spk=spk, rec=rec, truth=truth, want=want, got=got)


def as_fields(m):
    return dict(mean1=m.mean1, lda=m.lda, mean2=m.mean2, mean=m.plda_mean, W=m.stats['W'], B=m.stats['B'])


def test_the_device_model_is_the_references_within_the_references_own_sensitivity(trained):
    x, spk, want = trained['x'], trained['spk'], trained['want']
    rng = np.random.default_rng(99)
    e0 = 0.0
    for _ in range(3):
        order = rng.permutation(len(x))
        other = ref.train(x[order], [spk[i] for i in order], ref.LDA_DIM)
        e0 = max(e0, max(ref.rel_dist(other[f], want[f]) for f in FIELDS))
    tol = 32 * e0 + C_TOL * len(x) * U
    got = as_fields(trained['got'])
    dist = {f: ref.rel_dist(got[f], want[f]) for f in FIELDS}
    print(f'e0 = {e0:.2e}, tolerance = {tol:.2e}, device against reference: ' + ', '.join(f'{f} {d:.2e}' for f, d in dist.items()))
    assert 0 < e0 < 1e-12
    assert max(dist.values()) <= tol, (dist, tol)
    m = trained['got']
    tr, psi = m.plda_transform, m.plda_psi
    assert tr.shape == (ref.LDA_DIM, ref.LDA_DIM) and np.all(np.diff(psi) <= 0) and np.all(psi >= 0)
    assert ref.rel_dist(np.linalg.inv(tr.T.dot(tr)), want['W']) <= tol + 1e-10
    assert ref.rel_dist(np.linalg.inv((tr.T / psi).dot(tr)), want['B']) <= tol + 1e-10
    top = np.abs(m.lda).argmax(axis=0)
    assert np.all(m.lda[top, np.arange(ref.LDA_DIM)] > 0)
    st = m.stats
    assert st['N'] == len(x) and st['K'] == ref.K_TRAIN and st['speakers'] == list(dict.fromkeys(spk))
    assert st['kernel_ms']['stage1'] > 0 and st['kernel_ms']['stage2'] > 0


def test_training_twice_gives_the_same_bits(trained):
    from vbx_amd import backend
    again = backend.train_backend(trained['x'], trained['spk'], ref.LDA_DIM, device=0)
    for a, b in zip(again.arrays(), trained['got'].arrays()):
        assert np.array_equal(a, b)


def chain_labels(tmp, tag, rec, save):
    """The driver's stages (AHC+VB) on the held-out recording with the backend files that ``save`` writes."""
    from vbx_amd import vbhmm
    out = tmp / tag
    out.mkdir()
    save(out / 'transform.npz', out / 'plda')
    models = vbhmm.load_models(str(out / 'transform.npz'), str(out / 'plda'))
    names = np.array([f'rec_{i:04d}' for i in range(len(rec))])
    times = np.stack([0.25 * np.arange(len(rec)), 0.25 * np.arange(len(rec)) + 1.5], axis=1)
    args = argparse.Namespace(init='AHC+VB', init_rttm_dir=None, threshold=0.0, lda_dim=ref.LDA_DIM, Fa=0.3, Fb=17.0, loopP=0.9,
                              init_smoothing=5.0, output_2nd=False, out_rttm_dir=str(out / 'rttm'))
    stages = vbhmm.DeviceStages(0)
    try:
        state, _timing = vbhmm.diarize_recordings([('rec', names, rec)], {'rec': (names, times)}, models, args, stages,
                                                  log=lambda *a: None)
    finally:
        stages.close()
    return np.asarray(state['rec']['labels1st'])


def test_the_trained_files_diarize_a_held_out_recording_as_the_references_do_and_without_error(trained, tmp_path):
    from vbx_amd import backend
    want = trained['want']
    reference = backend.Backend(want['mean1'], want['lda'], want['mean2'], want['mean'], want['transform'], want['psi'], {})
    ours = chain_labels(tmp_path, 'device', trained['rec'], trained['got'].save)
    theirs = chain_labels(tmp_path, 'reference', trained['rec'], reference.save)
    assert len(ours) == 150
    assert np.array_equal(ours, theirs)
    assert ref.same_partition(ours, trained['truth']) and len(set(ours.tolist())) == 3


def test_the_command_line_writes_the_files_train_backend_gives(trained, tmp_path, capsys):
    from vbx_amd import backend
    from vbx_amd import kaldi_formats as kf
    x, spk = trained['x'], trained['spk']
    keys = [f'utt{i:04d}' for i in range(len(x))]
    kf.write_vec_flt_ark(tmp_path / 'x.ark', zip(keys, x))
    (tmp_path / 'utt2spk').write_text(''.join(f'{k} {s}\n' for k, s in zip(reversed(keys), reversed(spk))))
    rc = backend.main(['--xvec-ark-file', str(tmp_path / 'x.ark'), '--utt2spk', str(tmp_path / 'utt2spk'), '--lda-dim',
                       str(ref.LDA_DIM), '--out-transform', str(tmp_path / 't.npz'), '--out-plda', str(tmp_path / 'plda'),
                       '--device', '0', '--timing'])
    text = capsys.readouterr().out
    assert rc == 0 and '390 x-vectors of 60 speakers, 24 -> 8 dimensions' in text and 'kernels' in text
    m = trained['got']
    mean1, mean2, lda = kf.read_xvec_transform(str(tmp_path / 't.npz'))
    mean, tr, psi = kf.read_plda(str(tmp_path / 'plda'))
    for a, b in zip((mean1, lda, mean2, mean, tr, psi), m.arrays()):
        assert np.array_equal(a, b)
    # --min-utts 2 drops the five singletons: another model, of 55 speakers
    rc = backend.main(['--xvec-ark-file', str(tmp_path / 'x.ark'), '--utt2spk', str(tmp_path / 'utt2spk'), '--lda-dim',
                       str(ref.LDA_DIM), '--out-transform', str(tmp_path / 't2.npz'), '--out-plda', str(tmp_path / 'plda2'),
                       '--min-utts', '2'])
    assert rc == 0 and '385 x-vectors of 55 speakers' in capsys.readouterr().out


def test_a_row_without_length_after_centring_is_refused_with_its_index():
    """Rows 2 and 3 equal the mean of the four (exactly: 1.5 and 3.0 are the midpoints); the reference's l2_norm would write NaN."""
    from vbx_amd import _capi
    ctx = _capi.default_context(0)
    x = np.array([[1.0, 2.0], [2.0, 4.0], [1.5, 3.0], [1.5, 3.0]], dtype=np.float32)
    be = _capi.BackendStats(ctx, x, [0, 0, 1, 1], 2)
    try:
        with pytest.raises(_capi.VbxError, match='row 2 has no length after centring'):
            be.stage1()
        with pytest.raises(_capi.VbxError, match='stage 1 has not run'):
            be.stage2(np.ones((2, 1)), np.zeros(1))
    finally:
        be.close()
