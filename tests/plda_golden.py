"""Reader of tests/golden/plda_cases.npz (tests/golden/make_golden_plda.py) and the NumPy restatements the PLDA score
tests compare kernels with.  Loaded once per process; nobody writes to what it returns."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = [f'T{T}_{tag}' for T in (17, 65, 131, 200) for tag in ('e0.3', 'e0.5', 'full')]


@functools.lru_cache(maxsize=None)
def load():
    """-> (kaldi_plda = (mu, tr, psi), {case: dict(x, T, target_energy | None, pca_dim, acvar, scr, thr, labels, tol)})"""
    model = np.load(os.path.join(GOLDEN, 'driver_split3.npz'))
    plda = (model['plda_mean'], model['plda_trans'], model['plda_psi'])
    npz = np.load(os.path.join(GOLDEN, 'plda_cases.npz'))
    x = npz['x']
    cases = {}
    for name in CASES:
        T = int(name[1:].split('_')[0])
        tag = name.split('_')[1]
        iu = np.triu_indices(T)
        upper = npz[name + '/scr_upper']
        scr = np.empty((T, T))
        scr.T[iu] = upper + npz[name + '/scr_lower_diff'].astype(np.float64)       # the lower triangle, bit for bit
        scr[iu] = upper
        cases[name] = dict(x=x[:T], T=T, target_energy=None if tag == 'full' else float(tag[1:]), pca_dim=int(npz[name + '/pca_dim']),
                           acvar=npz[name + '/acvar'], scr=scr, thr=float(npz[name + '/thr']), labels=npz[name + '/labels'],
                           tol=float(npz[name + '/tol']))
        for v in cases[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    assert set(CASES) == {k.split('/')[0] for k in npz.files if '/' in k}
    return plda, cases


def score_kw(case):
    """keywords of kaldi_ivector_plda_scoring_dense for a case"""
    return dict(pca_dim=case['x'].shape[1]) if case['target_energy'] is None else dict(target_energy=case['target_energy'])


def lda_space_scores(Fe, Ft, diagAC):
    """PLDA scores of rows in LDA space, from Burget et al., ICASSP 2011, eq. (7-8): within-class covariance I,
    across-class covariance diag(diagAC)."""
    tot, wc2ac = 1.0 + diagAC, 1.0 + 2.0 * diagAC
    Lambda = 0.5 * (1.0 - 1.0 / wc2ac)
    Gamma = -0.25 * (1.0 / wc2ac + 1.0 - 2.0 / tot)
    k = -0.5 * (np.log(wc2ac).sum() - 2.0 * np.log(tot).sum())
    return (Fe * Lambda) @ Ft.T + ((Fe ** 2) @ Gamma)[:, None] + ((Ft ** 2) @ Gamma)[None, :] + k


def dense_scores(x, mu, proj, acvar):
    """Projection, Kaldi length normalisation and scores of the rows x under (mu, proj [D][d], acvar [d])."""
    y = (x - mu) @ proj
    y = y * np.sqrt(y.shape[1] / ((y ** 2) @ (1.0 / (acvar + 1.0))))[:, None]
    return lda_space_scores(y, y, acvar)
