"""The Kaldi-recipe PLDA similarity of the AHC stage on the GPU (vbx_plda_score.hpp through the C ABI):

  * every case of tests/golden/plda_cases.npz against what the reference computed, within the tolerance the generator
    measured on the reference itself; exact symmetry, run-to-run and resident-vs-host bit equality; calibration, device
    and host linkage and the cut on the resulting vbx_scores;
  * kernel edges (tile, padding and chunk boundaries) against NumPy restatements, with bounds from the rounding of the
    sums involved (u = 2^-53; a sum of n products in any order is within n u sum|a b| of the exact one);
  * the driver with ahc_scores='plda' on a three-recording archive made of fixture rows.
"""
import os

import numpy as np
import pytest

import plda_golden

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
PAD = 3                     # rows in front of the fixture's in the resident copy: row0 != 0


@pytest.fixture(scope='module')
def ctx():
    from vbx_amd import _capi
    return _capi.default_context(None)


@pytest.fixture(scope='module')
def resident(ctx):
    """The fixture's 200 rows as resident xproj rows (identity transform: unit-length rows come back as themselves up to
    rounding) behind PAD other rows.  -> (XVectors, the rows as the device holds them)"""
    from vbx_amd import _capi
    plda, cases = plda_golden.load()
    x = cases['T200_full']['x']
    D = x.shape[1]
    xv = _capi.XVectors(ctx, np.concatenate([x[7:7 + PAD], x]), np.zeros(D), np.eye(D), np.zeros(D), plda[0], np.eye(D), D)
    rows = xv.get('xproj', PAD, len(x))
    assert np.abs(rows - x).max() < 1e-15
    yield xv, rows
    xv.close()


@pytest.mark.parametrize('name', plda_golden.CASES)
def test_fixture_case(name, ctx, resident):
    from vbx_amd import _capi
    from vbx_amd import diarization_lib as dl
    from vbx_amd.vbhmm import cut_linkage
    plda, cases = plda_golden.load()
    c = cases[name]
    T, kw = c['T'], plda_golden.score_kw(c)
    xv, rows = resident
    sc, pca_dim = dl.plda_dense_scores(ctx, plda, c['x'], **kw)
    try:
        assert len(sc) == T * T
        S = sc.get().reshape(T, T)
        err = np.abs(S - c['scr']).max()
        print(f'{name}: max|S - reference| = {err:.2e}, tol = {c["tol"]:.2e}, pca_dim {pca_dim}')
        assert pca_dim == c['pca_dim']
        assert err <= c['tol']
        assert np.array_equal(S, S.T)
        sc2, _ = dl.plda_dense_scores(ctx, plda, c['x'], **kw)                     # the same bits on every run
        try:
            assert np.array_equal(sc2.get().reshape(T, T), S)
        finally:
            sc2.close()
        # resident rows and the same rows from the host: the same bits, covariance and scores
        sc_h, dim_h = dl.plda_dense_scores(ctx, plda, rows[:T], **kw)
        sc_r, dim_r = dl.plda_dense_scores(ctx, plda, resident=(xv, PAD, T), **kw)
        try:
            S_r = sc_r.get().reshape(T, T)
            assert dim_h == dim_r == c['pca_dim']
            assert np.array_equal(S_r, sc_h.get().reshape(T, T)) and np.array_equal(S_r, S_r.T)
            print(f'{name}: resident rows, max|S - reference| = {np.abs(S_r - c["scr"]).max():.2e}')
        finally:
            sc_h.close()
            sc_r.close()
        mean_h, cov_h = _capi.plda_covariance(ctx, rows[:T])
        mean_r, cov_r = _capi.plda_covariance_resident(ctx, xv, PAD, T)
        assert np.array_equal(mean_h, mean_r) and np.array_equal(cov_h, cov_r)
        # what follows the scores in the driver works on them as on cosine scores
        thr, _ = sc.two_gmm_calib(20, want_llr=False)
        print(f'{name}: thr {thr!r}, reference {c["thr"]!r}')
        np.testing.assert_allclose(thr, c['thr'], rtol=1e-9)
        Z_host = _capi.linkage_average(sc.get_condensed(T, -1.0))
        Z_dev = sc.linkage_average(T)                                              # (consumes the scores)
        assert np.array_equal(Z_dev, Z_host)
        assert np.array_equal(cut_linkage(Z_dev.copy(), thr, 0.0), c['labels'])
    finally:
        sc.close()


def test_public_functions_return_what_the_reference_returns(ctx, capsys):
    from vbx_amd import diarization_lib as dl
    plda, cases = plda_golden.load()
    c = cases['T65_e0.5']
    x = c['x'].copy()
    S = dl.kaldi_ivector_plda_scoring_dense(plda, x, target_energy=0.5)
    assert capsys.readouterr().out == f'pca_dim: {c["pca_dim"]}\n'                # diarization_lib.py:85
    assert np.array_equal(x, c['x']), 'input mutated'
    assert isinstance(S, np.ndarray) and S.dtype == np.float64 and S.shape == (65, 65) and S.flags.writeable
    assert np.abs(S - c['scr']).max() <= c['tol']
    S_all = dl.kaldi_ivector_plda_scoring_dense(plda, x, target_energy=1.0)        # every dimension, no covariance
    assert capsys.readouterr().out == 'pca_dim: 128\n'
    assert np.abs(S_all - cases['T65_full']['scr']).max() <= cases['T65_full']['tol']
    assert np.array_equal(S_all, dl.kaldi_ivector_plda_scoring_dense(plda, x, pca_dim=128))


def _model(rng, D, d):
    """A well-conditioned random model: (mu, proj [D][d], acvar [d])"""
    return 0.1 * rng.standard_normal(D), rng.standard_normal((D, d)) / np.sqrt(D), rng.uniform(0.05, 20.0, d)


def _dense_bound(x, mu, proj, acvar):
    """First-order rounding bound of the dense scores.  The projection is a sum of D products: |dy| <= D u ya with
    ya = |x - mu| |proj|.  The length normalisation s = sqrt(d / sum w y^2) moves by |ds| / s <= D u r, r = sum w |y| ya /
    sum w y^2, so z = s y moves by |dz| <= D u e, e = s ya + r |z|.  A score is bilinear in z_i, z_j and itself a sum of d
    products plus three terms: |dS_ij| <= (e_i L).|z_j| + (|z_i| L).e_j + 2 G.(|z_i| e_i) + 2 G.(|z_j| e_j) + (d + 8) u A_ij,
    A the score formula on absolute values.  (Second-order terms are D u r ~ 1e-12 of that.)  The factor 4 in front covers
    NumPy's own rounding and the transcendental functions of the constant."""
    D, d = proj.shape
    y = (x - mu) @ proj
    ya = np.abs(x - mu) @ np.abs(proj)
    w = 1.0 / (acvar + 1.0)
    s = np.sqrt(d / ((y ** 2) @ w))
    r = ((np.abs(y) * ya) @ w) / ((y ** 2) @ w)
    za = np.abs(y) * s[:, None]
    e = D * U * (ya * s[:, None] + r[:, None] * za)
    Lambda, Gamma = acvar / (1.0 + 2.0 * acvar), np.abs(-0.25 * (1.0 / (1.0 + 2.0 * acvar) + 1.0 - 2.0 / (1.0 + acvar)))
    k = np.abs(np.log(1.0 + 2.0 * acvar)).sum() + 2.0 * np.abs(np.log(1.0 + acvar)).sum()
    q, dq = (za ** 2) @ Gamma, 2.0 * ((za * e) @ Gamma)
    cross = (e * Lambda) @ za.T
    A = (za * Lambda) @ za.T + q[:, None] + q[None, :] + k
    return 4.0 * (cross + cross.T + dq[:, None] + dq[None, :] + (d + 8.0) * U * A).max()


@pytest.mark.parametrize('T,D,d', [(2, 24, 24), (63, 24, 24), (64, 24, 24), (65, 24, 24), (129, 24, 24),
                                    (70, 130, 2), (70, 130, 15), (70, 130, 16), (70, 130, 17), (70, 130, 128)])
def test_score_gemm_and_projection_edges(T, D, d, ctx):
    from vbx_amd import _capi
    rng = np.random.default_rng(1000 * T + d)
    mu, proj, acvar = _model(rng, D, d)
    x = rng.standard_normal((T, D)) + mu
    sc = _capi.Scores.plda(ctx, x, mu, proj, acvar)
    try:
        S = sc.get().reshape(T, T)
    finally:
        sc.close()
    want, tol = plda_golden.dense_scores(x, mu, proj, acvar), _dense_bound(x, mu, proj, acvar)
    err = np.abs(S - want).max()
    print(f'T={T} D={D} d={d}: max|S - numpy| = {err:.2e}, bound = {tol:.2e}, max|S| = {np.abs(want).max():.1f}')
    assert np.isfinite(S).all() and err <= tol
    assert np.array_equal(S, S.T)


@pytest.mark.parametrize('N,M', [(3, 130), (65, 64), (1, 1)])
def test_rectangular_scores_in_lda_space(N, M, ctx):
    """A sum of D products and three more terms per entry: within 2 (D + 8) u of the formula on absolute values (NumPy's
    share included)."""
    from vbx_amd.diarization_lib import PLDA_scoring_in_LDA_space
    D = 20
    rng = np.random.default_rng(N * 1000 + M)
    Fe, Ft, ac = rng.standard_normal((N, D)), rng.standard_normal((M, D)), rng.uniform(0.05, 20.0, D)
    S = PLDA_scoring_in_LDA_space(Fe, Ft, ac)
    assert S.shape == (N, M) and S.dtype == np.float64
    want = plda_golden.lda_space_scores(Fe, Ft, ac)
    Lambda, Gamma = ac / (1.0 + 2.0 * ac), np.abs(-0.25 * (1.0 / (1.0 + 2.0 * ac) + 1.0 - 2.0 / (1.0 + ac)))
    k = np.log(1.0 + 2.0 * ac).sum() + 2.0 * np.log(1.0 + ac).sum()
    A = ((np.abs(Fe) * Lambda) @ np.abs(Ft).T + ((Fe ** 2) @ Gamma)[:, None] + ((Ft ** 2) @ Gamma)[None, :] + k).max()
    err, tol = np.abs(S - want).max(), 2.0 * (D + 8) * U * A
    print(f'N={N} M={M}: max|S - numpy| = {err:.2e}, bound = {tol:.2e}')
    assert err <= tol
    if N == 65:                                    # the same rows on both sides: the dense path's symmetry argument
        S2 = PLDA_scoring_in_LDA_space(Ft, Ft, ac)
        assert np.abs(S2 - S2.T).max() <= tol      # (a = Ft Lambda against b = Ft: equal to rounding, not to the bit)


def _cov_shapes():
    from vbx_amd._capi import PLDA_COV_CHUNK
    return [(2, 24), (65, 24), (PLDA_COV_CHUNK, 24), (PLDA_COV_CHUNK + 1, 24), (70, 100), (70, 128), (70, 256)]


@pytest.mark.parametrize('T,D', _cov_shapes())
def test_covariance_edges(T, D, ctx):
    """Mean: a sum of T terms.  Covariance: a sum of T products of differences that each carry one rounding, and the
    mean's own error enters squared: within (T + 4) u of the sums of absolute values, twice for NumPy's share."""
    from vbx_amd import _capi
    rng = np.random.default_rng(T * 1000 + D)
    x = rng.standard_normal((T, D)) * rng.uniform(0.5, 2.0, D) + rng.standard_normal(D)
    mean, cov = _capi.plda_covariance(ctx, x)
    mean2, cov2 = _capi.plda_covariance(ctx, x)
    assert np.array_equal(mean, mean2) and np.array_equal(cov, cov2)              # no atomics: the same bits
    assert np.array_equal(cov, cov.T)
    m_err, m_tol = np.abs(mean - x.mean(0)).max(), 2.0 * (T + 4) * U * np.abs(x).mean(0).max()
    xc = np.abs(x - x.mean(0))
    c_err, c_tol = np.abs(cov - np.cov(x.T, bias=True)).max(), 2.0 * (T + 4) * U * ((xc.T @ xc) / T + np.abs(x).mean(0).max() ** 2).max()
    print(f'T={T} D={D}: mean err {m_err:.2e} (bound {m_tol:.2e}), cov err {c_err:.2e} (bound {c_tol:.2e})')
    assert m_err <= m_tol and c_err <= c_tol


def test_driver_with_plda_scores(tmp_path):
    """Three recordings of fixture rows, one of a single x-vector, through diarize(..., ahc_scores='plda', init='AHC'):
    the fixture's labels, at target_energy 0.5 and with every dimension kept (the driver's default)."""
    from vbx_amd import kaldi_formats as kf
    from vbx_amd import vbhmm
    plda, cases = plda_golden.load()
    x = cases['T200_full']['x']
    D = x.shape[1]
    recs = [('recA', x[:65]), ('recB', x[70:71]), ('recC', x[:131])]
    keys = [(f'{rec}_{i:04d}', rec, row) for rec, rows in recs for i, row in enumerate(rows)]
    paths = {k: str(tmp_path / k) for k in ('ark', 'seg', 'plda', 'transform.npz', 'out')}
    kf.write_vec_flt_ark(paths['ark'], [(key, row) for key, _, row in keys], dtype=np.float64)
    kf.write_segments(paths['seg'], [(key, rec, 0.25 * i, 0.25 * i + 1.5) for i, (key, rec, _) in enumerate(keys)])
    kf.write_plda(paths['plda'], *plda)
    np.savez(paths['transform.npz'], mean1=np.zeros(D), mean2=np.zeros(D), lda=np.eye(D))
    for target_energy, tag in ((0.5, 'e0.5'), (None, 'full')):
        argv = ['--init', 'AHC', '--out-rttm-dir', paths['out'], '--xvec-ark-file', paths['ark'], '--segments-file', paths['seg'],
                '--xvec-transform', paths['transform.npz'], '--plda-file', paths['plda'], '--threshold', '0', '--lda-dim', str(D),
                '--Fa', '0.3', '--Fb', '17', '--loopP', '0.99'] + ([] if target_energy is None else ['--target-energy', str(target_energy)])
        args = vbhmm.build_parser().parse_args(argv)
        state, _timing = vbhmm.diarize(args, log=lambda *_: None, ahc_scores='plda')
        assert list(state) == ['recA', 'recB', 'recC']
        assert np.array_equal(state['recA']['labels1st'], cases['T65_' + tag]['labels'])
        assert np.array_equal(state['recB']['labels1st'], [0])
        assert np.array_equal(state['recC']['labels1st'], cases['T131_' + tag]['labels'])
        np.testing.assert_allclose(state['recC']['thr'], cases['T131_' + tag]['thr'], rtol=1e-9)
        assert sorted(os.listdir(paths['out'])) == ['recA.rttm', 'recB.rttm', 'recC.rttm']
    args = vbhmm.build_parser().parse_args(argv + ['--ahc-scores', 'plda'])         # the flag is the keyword's default
    state2, _ = vbhmm.diarize(args, log=lambda *_: None)
    assert all(np.array_equal(state2[r]['labels1st'], state[r]['labels1st']) for r in state)
