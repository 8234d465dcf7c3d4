"""Backend training on the host (no GPU): ``estimate_plda`` (grouped by class size) against Kaldi's class-by-class loop of
tests/backend_ref.py, the sign-free invariants of the written model, ``estimate_lda``, the files and every refusal of the command
line, and the C ABI."""
import os
import re

import numpy as np
import pytest

import backend_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- estimate_plda ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def plda_case():
    """K = 40 classes of 1 ... 6 rows (singletons included) in d = 8, with between- and within-class spread."""
    rng = np.random.default_rng(40)
    K, d = 40, 8
    counts = 1 + np.arange(K) % 6
    cls = rng.permutation(np.repeat(np.arange(K), counts)).astype(np.int32)
    cls, _ = ref.first_appearance(cls.tolist())
    counts = np.bincount(cls, minlength=K)
    centres = rng.standard_normal((K, d)) * np.linspace(2.0, 0.5, d)
    u = centres[cls] + 0.4 * rng.standard_normal((len(cls), d)) + 0.3
    mu, counts, scatter = ref.plda_stats(u, cls, K)
    return dict(u=u, cls=cls, K=K, d=d, mu=mu, counts=counts, scatter=scatter, N=len(cls))


def grouped_model(case, iters=10):
    from vbx_amd import backend
    mu, counts = case['mu'], case['counts']
    mean = mu.sum(axis=0) / case['K']
    order, n, off = backend.count_groups(counts)
    G, _ = ref.second_moments(mu[order] - mean, off)
    return backend.estimate_plda(n, np.diff(off), G, case['scatter'], case['N'], mean, iters)


def test_estimate_plda_agrees_with_the_class_loop_within_the_loops_own_rounding_noise(plda_case):
    """Tolerance: 100 x the relative distance between two runs of the class loop that visit the classes in opposite orders (the
    reference's own rounding noise; the factor allows for the different order of the products in the grouped form)."""
    c = plda_case
    mean, W, B = ref.plda_class_loop(c['mu'], c['counts'], c['scatter'], 10)
    _m, Wr, Br = ref.plda_class_loop(c['mu'], c['counts'], c['scatter'], 10, visit=range(c['K'] - 1, -1, -1))
    noise = max(ref.rel_dist(Wr, W), ref.rel_dist(Br, B))
    got = grouped_model(c)
    dist = dict(W=ref.rel_dist(got['W'], W), B=ref.rel_dist(got['B'], B), mean=ref.rel_dist(got['mean'], mean))
    print(f'class loop forwards against backwards: {noise:.2e}; grouped form against the loop: {dist}')
    assert noise > 0
    assert max(dist.values()) <= 100 * noise, (dist, noise)


def test_the_written_model_gives_back_W_and_B_whatever_the_eigenvectors_signs(plda_case):
    got = grouped_model(plda_case)
    tr, psi = got['transform'], got['psi']
    assert np.all(np.diff(psi) <= 0) and np.all(psi >= 0)
    assert ref.rel_dist(np.linalg.inv(tr.T.dot(tr)), got['W']) < 1e-10
    assert ref.rel_dist(np.linalg.inv((tr.T / psi).dot(tr)), got['B']) < 1e-10
    want_tr, want_psi = ref.plda_output(got['W'], got['B'])
    assert np.allclose(psi, want_psi, rtol=1e-12, atol=0)
    assert np.allclose(np.abs(tr), np.abs(want_tr), rtol=0, atol=1e-10)


def test_estimate_plda_refuses_a_training_set_of_singletons():
    from vbx_amd import backend
    with pytest.raises(ValueError, match='two rows'):
        backend.estimate_plda([1], [5], np.zeros((1, 3, 3)), np.zeros((3, 3)), 5, np.zeros(3))


# ---- estimate_lda ----------------------------------------------------------------------------------------------------------
def test_estimate_lda_whitens_Sw_diagonalises_Sb_and_fixes_the_signs():
    from vbx_amd import backend
    world = ref.World(7)
    x, spk = world.training_set()
    cls, names = ref.first_appearance(spk)
    y = ref.l2_norm(x.astype(np.float64) - x.astype(np.float64).mean(axis=0))
    ybar, St, Sb = ref.lda_scatters(y, cls, len(names))
    lda, mean2 = backend.estimate_lda(ybar, St, Sb, ref.LDA_DIM)
    assert lda.shape == (ref.DIN, ref.LDA_DIM)
    assert np.abs(lda.T.dot(St - Sb).dot(lda) - np.eye(ref.LDA_DIM)).max() < 1e-10
    between = lda.T.dot(Sb).dot(lda)
    assert np.abs(between - np.diag(np.diag(between))).max() < 1e-9 * np.diag(between).max()
    assert np.all(np.diff(np.diag(between)) < 0)
    top = np.abs(lda).argmax(axis=0)
    assert np.all(lda[top, np.arange(ref.LDA_DIM)] > 0)
    assert np.allclose(mean2, lda.T.dot(ybar), rtol=0, atol=1e-15)
    want, want2 = ref.lda(ybar, St, Sb, ref.LDA_DIM)
    assert np.array_equal(lda, want) and np.allclose(mean2, want2, rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match='lda_dim'):
        backend.estimate_lda(ybar, St, Sb, ref.DIN + 1)


def test_the_sign_convention_makes_the_largest_entry_of_every_column_positive():
    from vbx_amd import backend
    v = np.array([[1.0, -3.0, 0.5], [-2.0, 1.0, 0.25]])
    assert np.array_equal(backend.sign_convention(v), [[-1.0, 3.0, 0.5], [2.0, -1.0, 0.25]])


def test_classes_are_numbered_in_order_of_first_appearance_and_grouped_by_size():
    from vbx_amd import backend
    cls, names = backend.class_index(['b', 'a', 'b', 'c', 'a', 'b'])
    assert cls.tolist() == [0, 1, 0, 2, 1, 0] and cls.dtype == np.int32 and names == ['b', 'a', 'c']
    order, n, off = backend.count_groups([3, 1, 2, 1, 3])
    assert order.tolist() == [1, 3, 2, 0, 4] and n.tolist() == [1, 2, 3] and off.tolist() == [0, 2, 3, 5]


# ---- files and the command line --------------------------------------------------------------------------------------------
def test_read_utt2spk_keeps_file_order_and_refuses_what_it_cannot_read(tmp_path):
    from vbx_amd import backend
    p = tmp_path / 'utt2spk'
    p.write_text('u2 spkB\nu1 spkA\n\nu3 spkB\n')
    assert list(backend.read_utt2spk(p).items()) == [('u2', 'spkB'), ('u1', 'spkA'), ('u3', 'spkB')]
    p.write_text('u1 spkA extra\n')
    with pytest.raises(ValueError, match='utt2spk:1'):
        backend.read_utt2spk(p)
    p.write_text('u1 spkA\nu1 spkB\n')
    with pytest.raises(ValueError, match='twice'):
        backend.read_utt2spk(p)


@pytest.fixture()
def training_files(tmp_path):
    from vbx_amd import kaldi_formats as kf
    rng = np.random.default_rng(3)
    spk = ['a', 'b', 'a', 'c', 'b', 'a', 'd']
    x = rng.standard_normal((len(spk), 5)).astype(np.float32)
    keys = [f'utt{i}' for i in range(len(spk))]
    kf.write_vec_flt_ark(tmp_path / 'x.ark', zip(keys, x))
    (tmp_path / 'utt2spk').write_text(''.join(f'{k} {s}\n' for k, s in zip(keys, spk)))
    return dict(dir=tmp_path, x=x, spk=spk, keys=keys)


def test_load_training_set_pairs_rows_with_speakers_and_filters_by_min_utts(training_files):
    from vbx_amd import backend
    d = training_files['dir']
    x, spk = backend.load_training_set(d / 'x.ark', d / 'utt2spk')
    assert np.array_equal(x, training_files['x']) and spk == training_files['spk']
    x, spk = backend.load_training_set(d / 'x.ark', d / 'utt2spk', min_utts=2)
    assert spk == ['a', 'b', 'a', 'b', 'a'] and np.array_equal(x, training_files['x'][[0, 1, 2, 4, 5]])
    x, spk = backend.load_training_set(d / 'x.ark', d / 'utt2spk', min_utts=4)
    assert len(x) == 0 and spk == []


def run_cli(d, *extra, utt2spk='utt2spk', lda_dim=2, transform='t.npz'):
    from vbx_amd import backend
    return backend.main(['--xvec-ark-file', str(d / 'x.ark'), '--utt2spk', str(d / utt2spk), '--lda-dim', str(lda_dim),
                         '--out-transform', str(d / transform), '--out-plda', str(d / 'plda'), *extra])


def test_the_command_line_refuses_with_a_message_before_any_device_work(training_files, capsys):
    """Every refusal of the issue; none of them reaches the device (this test runs without one)."""
    d = training_files['dir']
    (d / 'short').write_text(''.join(f'{k} s\n' for k in training_files['keys'][:-2]))
    assert run_cli(d, utt2spk='short') == 2
    assert re.search(r'2 of the 7 x-vectors .* have no speaker .*utt5, utt6', capsys.readouterr().err)
    (d / 'one').write_text(''.join(f'{k} s\n' for k in training_files['keys']))
    assert run_cli(d, utt2spk='one') == 2
    assert 'at least two' in capsys.readouterr().err
    assert run_cli(d, lda_dim=4) == 2                            # K - 1 = 3
    assert 'lda_dim=4 outside [1, min(Din=5, K - 1=3)]' in capsys.readouterr().err
    (d / 'all').write_text(''.join(f'{k} s{i}\n' for i, k in enumerate(training_files['keys'])))
    assert run_cli(d, utt2spk='all') == 2
    assert 'no within-speaker covariance' in capsys.readouterr().err
    assert run_cli(d, '--min-utts', '9') == 2
    assert 'no speaker has 9' in capsys.readouterr().err
    assert run_cli(d, transform='t.txt') == 2
    assert '.npz' in capsys.readouterr().err
    assert not (d / 'plda').exists()


def test_train_backend_refuses_the_same_without_a_device():
    from vbx_amd import backend
    x = np.zeros((4, 3), dtype=np.float32)
    with pytest.raises(ValueError, match='at least two'):
        backend.train_backend(x, ['a'] * 4, 1)
    with pytest.raises(ValueError, match='within-speaker'):
        backend.train_backend(x, list('abcd'), 1)
    with pytest.raises(ValueError, match='lda_dim=2'):
        backend.train_backend(x, list('aabb'), 2)
    with pytest.raises(ValueError, match='do not match'):
        backend.train_backend(x, list('aab'), 1)


def test_saved_files_come_back_through_the_chains_readers(tmp_path):
    from vbx_amd import backend
    from vbx_amd import kaldi_formats as kf
    rng = np.random.default_rng(5)
    m = backend.Backend(rng.standard_normal(6), rng.standard_normal((6, 3)), rng.standard_normal(3), rng.standard_normal(3),
                        rng.standard_normal((3, 3)), np.array([3.0, 2.0, 0.5]), {})
    m.save(tmp_path / 't.npz', tmp_path / 'plda')
    mean1, mean2, lda = kf.read_xvec_transform(str(tmp_path / 't.npz'))
    assert np.array_equal(mean1, m.mean1) and np.array_equal(mean2, m.mean2) and np.array_equal(lda, m.lda)
    mean, tr, psi = kf.read_plda(str(tmp_path / 'plda'))
    assert np.array_equal(mean, m.plda_mean) and np.array_equal(tr, m.plda_transform) and np.array_equal(psi, m.plda_psi)
    try:
        import h5py                                              # noqa: F401
    except ImportError:
        with pytest.raises(ValueError, match=r'h5py.*\.npz'):
            m.save(tmp_path / 't.h5', tmp_path / 'plda2')
        assert not (tmp_path / 'plda2').exists()
    else:
        m.save(tmp_path / 't.h5', tmp_path / 'plda2')
        mean1, mean2, lda = kf.read_xvec_transform(str(tmp_path / 't.h5'))
        assert np.array_equal(mean1, m.mean1) and np.array_equal(mean2, m.mean2) and np.array_equal(lda, m.lda)
    with pytest.raises(ValueError, match='.npz'):
        m.save(tmp_path / 't.mat', tmp_path / 'plda3')


def test_the_reference_recipe_separates_the_synthetic_world_it_was_trained_on():
    """The generator and the host chain of the end-to-end GPU test, on the seed recorded there: trained on the host, the chain
    through oracle/ alone makes no error on the held-out recording."""
    world = ref.World(ref.E2E_SEED)
    x, spk = world.training_set()
    rec, truth = world.recording()
    model = ref.train(x, spk, ref.LDA_DIM)
    labels = ref.host_chain(rec, model, ref.LDA_DIM)
    assert len(x) == 390 and len(set(spk)) == ref.K_TRAIN and x.dtype == np.float32
    assert ref.same_partition(labels, truth) and len(set(labels.tolist())) == 3


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
NEW_ABI = ['vbx_backend_class_sums', 'vbx_backend_second_moments', 'vbx_backend_create', 'vbx_backend_stage1',
           'vbx_backend_stage2', 'vbx_backend_destroy']


def test_the_header_still_says_abi_7_and_the_library_exports_the_new_entry_points():
    from vbx_amd import _capi
    header = open(os.path.join(REPO, 'include', 'vbx_hip.h')).read()
    assert re.search(r'#define\s+VBX_ABI_VERSION\s+7\b', header)
    for sym in NEW_ABI:
        assert re.search(rf'\bint {sym}\s*\(', header) and sym in _capi.ABI_SYMBOLS
    lib = _capi.load()
    assert lib.vbx_abi_version() == 7
    for sym in NEW_ABI:
        assert getattr(lib, sym).argtypes
