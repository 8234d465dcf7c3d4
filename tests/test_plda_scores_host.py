"""Host side of the Kaldi-recipe PLDA similarity (vbx_amd.diarization_lib: plda_pca_dim, plda_projection) against what the
reference computed for tests/golden/plda_cases.npz, the rule for target_energy >= 1, the warning in the region where the
reference's result is not determined by its input, and the ABI's new names.  No GPU."""
import os
import re
import warnings

import numpy as np
import pytest

import plda_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ABI = ['vbx_plda_covariance', 'vbx_plda_covariance_resident', 'vbx_plda_scores', 'vbx_plda_scores_resident', 'vbx_plda_score_lda']


@pytest.mark.parametrize('name', plda_golden.CASES)
def test_host_functions_reproduce_the_reference_pca_dim_and_acvar(name):
    """Covariance by NumPy here (the device's is tested on the GPU); rule, projection and variances by the two pure
    functions.  The scores NumPy gets from (M, acvar) stay within the fixture's measured tolerance of the reference's."""
    from scipy.linalg import eigh
    from vbx_amd.diarization_lib import plda_pca_dim, plda_projection
    plda, cases = plda_golden.load()
    c = cases[name]
    x, D = c['x'], c['x'].shape[1]
    if c['target_energy'] is None:
        assert c['pca_dim'] == D
        M, acvar = plda_projection(plda, None)
    else:
        energy, PCA = eigh(np.cov(x.T, bias=True))
        with warnings.catch_warnings():
            warnings.simplefilter('error')                        # the fixture stays outside the undetermined region
            pca_dim = plda_pca_dim(c['target_energy'], D, energy, len(x))
        assert pca_dim == c['pca_dim'] and isinstance(pca_dim, int)
        M, acvar = plda_projection(plda, PCA[:, :-pca_dim - 1:-1])
    assert M.shape == (D, c['pca_dim']) and acvar.shape == (c['pca_dim'],)
    np.testing.assert_allclose(acvar, c['acvar'], rtol=1e-9)
    err = np.abs(plda_golden.dense_scores(x, plda[0], M, acvar) - c['scr']).max()
    print(f'{name}: max|S - reference| = {err:.2e}, tol = {c["tol"]:.2e}')
    assert err <= c['tol']


def test_target_energy_of_one_keeps_every_dimension_without_a_covariance():
    from vbx_amd.diarization_lib import plda_pca_dim
    for te in (1.0, 1.5):
        assert plda_pca_dim(te, 128) == 128 and plda_pca_dim(te, 7, energy=None, n_rows=2) == 7
    with pytest.raises(ValueError):
        plda_pca_dim(0.999, 128)                                   # below one the rule needs the eigenvalues


def test_warning_where_the_kept_subspace_is_not_determined():
    """Three x-vectors span two directions; target_energy = 0.9 asks for more (T = 3 of the issue's measurements)."""
    from scipy.linalg import eigh
    from vbx_amd.diarization_lib import plda_pca_dim
    _plda, cases = plda_golden.load()
    x = cases['T17_full']['x'][:3]
    energy = eigh(np.cov(x.T, bias=True))[0]
    with pytest.warns(RuntimeWarning, match='undetermined'):
        pca_dim = plda_pca_dim(0.9, x.shape[1], energy, 3)
    assert 2 < pca_dim < x.shape[1]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert plda_pca_dim(0.3, 128, [1e-3] * 120 + [1.0] * 8, 65) == 4


def test_new_abi_names_are_declared_and_bound():
    from vbx_amd import _capi
    text = open(os.path.join(REPO, 'include', 'vbx_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(vbx_[a-z_0-9]+)\s*\(', text))
    for name in NEW_ABI:
        assert name in declared and name in _capi.ABI_SYMBOLS, name
    assert re.search(r'#define VBX_ABI_VERSION 7\b', text)
    assert 'vbx_plda_score.hpp' in __import__('vbx_amd.build', fromlist=['HEADERS']).HEADERS
    kernels = open(os.path.join(REPO, 'vbx_amd', 'csrc', 'vbx_plda_score.hpp')).read()
    assert f'kCovChunk = {_capi.PLDA_COV_CHUNK};' in kernels and f'kPldaMaxTiles = {_capi.PLDA_MAX_DIM // 16};' in kernels


def test_mirror_keeps_the_reference_signatures():
    import inspect
    from vbx_amd import diarization_lib as dl
    sig = inspect.signature(dl.kaldi_ivector_plda_scoring_dense)
    assert list(sig.parameters) == ['kaldi_plda', 'x', 'target_energy', 'pca_dim', 'device']
    assert sig.parameters['target_energy'].default == 0.1 and sig.parameters['pca_dim'].default is None
    assert sig.parameters['device'].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(dl.PLDA_scoring_in_LDA_space)
    assert list(sig.parameters) == ['Fe', 'Ft', 'diagAC', 'device'] and sig.parameters['device'].kind is inspect.Parameter.KEYWORD_ONLY
    src = open(os.path.join(REPO, 'vbx_drop_in', 'diarization_lib.py')).read()
    assert 'PLDA_scoring_in_LDA_space' in src and 'kaldi_ivector_plda_scoring_dense' in src


def test_driver_flag_and_keyword(tmp_path):
    from vbx_amd import vbhmm
    base = ['--init', 'AHC', '--out-rttm-dir', 'o', '--xvec-ark-file', 'a', '--segments-file', 's', '--xvec-transform', 't',
            '--plda-file', 'p', '--threshold', '0', '--lda-dim', '128', '--Fa', '0.3', '--Fb', '17', '--loopP', '0.99']
    args = vbhmm.build_parser().parse_args(base)
    assert args.ahc_scores == 'cos' and args.target_energy == 1.0
    assert vbhmm.build_parser().parse_args(base + ['--ahc-scores', 'plda', '--target-energy', '0.5']).ahc_scores == 'plda'
    with pytest.raises(SystemExit):
        vbhmm.build_parser().parse_args(base + ['--ahc-scores', 'euclid'])
    with pytest.raises(ValueError, match='ahc_scores'):
        vbhmm.diarize(args, stages=object(), ahc_scores='euclid')
    # load_models hands the raw Kaldi model on, next to the diagonalised one
    from vbx_amd import kaldi_formats as kf
    plda, _ = plda_golden.load()
    kf.write_plda(str(tmp_path / 'plda'), *plda)
    np.savez(str(tmp_path / 'transform.npz'), mean1=np.zeros(4), mean2=np.zeros(4), lda=np.eye(4))
    models = vbhmm.load_models(str(tmp_path / 'transform.npz'), str(tmp_path / 'plda'))
    assert all(np.array_equal(a, b) for a, b in zip(models['kaldi_plda'], plda))
