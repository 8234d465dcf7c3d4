#!/usr/bin/env python
"""Golden fixture for the Kaldi-recipe PLDA similarity of the AHC stage, generated FROM THE REFERENCE (authoring
container only).

Imports /root/reference/VBx/diarization_lib.py (numpy + scipy only) and records what its
kaldi_ivector_plda_scoring_dense() gives for the first T projected x-vectors of ES2005a (make_golden_ahc.es2005a_x)
under the 16 kHz PLDA model, T in TS, for target_energy in ENERGIES and for pca_dim = D:

    tests/golden/plda_cases.npz
        x [200][128]                       the rows; a case takes the first T
        <case>/pca_dim                     the dimension the reference printed
        <case>/acvar                       the across-class variances the reference scored with
        <case>/scr_upper, scr_lower_diff   the reference's score matrix: upper triangle with the diagonal, row by row, and
                                           S[j][i] - S[i][j] for the same entries in float32 (the reference's matrix is not
                                           exactly symmetric; the difference is a few ulp and the sum restores every bit:
                                           tests/plda_golden.py; asserted below)
        <case>/thr                         the reference's twoGMMcalib_lin threshold of the scores
        <case>/labels                      SciPy average linkage of -S cut like vbhmm.py:139-146 with --threshold 0
        <case>/tol                         100 x the largest change of the reference's own scores when x is multiplied by
                                           1 + 1e-15 N(0, 1) (seeded): the bound a different summation order is held to
        <case>/margins                     (distance of the nearest energy ratio from target_energy, distance of the cut
                                           from the nearest merge height); both must exceed 1e-6, asserted here

The Kaldi PLDA model (mu, tr, psi, as read_plda loads it) is the one tests/golden/driver_split3.npz already holds as
plda_mean / plda_trans / plda_psi (asserted below): with a second copy of its 128 x 128 doubles this file would pass
the size a committed file may have, so tests/plda_golden.py takes the model from there.

case = T<T>_e<target_energy> or T<T>_full.  Every case has pca_dim <= T - 1 or pca_dim = D: outside the region where the
reference's result is not determined by its input (asserted).
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from make_golden_ahc import es2005a_x, ref_lib      # noqa: E402
from vbx_amd import kaldi_formats as kf             # noqa: E402

TS = (17, 65, 131, 200)
ENERGIES = (0.3, 0.5)
MARGIN = 1e-6


def score(lib, plda, x, **kw):
    """-> (scores, pca_dim the reference printed, diagAC it scored with)"""
    seen = {}
    inner = lib.PLDA_scoring_in_LDA_space

    def spy(Fe, Ft, diagAC):
        seen['acvar'] = np.array(diagAC)
        return inner(Fe, Ft, diagAC)
    lib.PLDA_scoring_in_LDA_space = spy
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            scr = lib.kaldi_ivector_plda_scoring_dense(plda, x.copy(), **kw)
    finally:
        lib.PLDA_scoring_in_LDA_space = inner
    word, value = out.getvalue().split()
    assert word == 'pca_dim:'
    return scr, int(value), seen['acvar']


def main():
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.linalg import eigh
    from scipy.spatial.distance import squareform
    lib = ref_lib()
    plda = kf.read_plda(f'{REF}/VBx/models/ResNet101_16kHz/plda')
    X = es2005a_x(lib)[:max(TS)]
    D = X.shape[1]
    held = np.load(os.path.join(HERE, 'driver_split3.npz'))
    assert all(np.array_equal(a, held[k]) for a, k in zip(plda, ('plda_mean', 'plda_trans', 'plda_psi')))
    out = dict(x=X)
    for T in TS:
        x = X[:T]
        energy = np.cumsum(eigh(np.cov(x.T, bias=True))[0][::-1])
        ratios = energy / energy[-1]
        for te in ENERGIES + (None,):
            name = f'T{T}_full' if te is None else f'T{T}_e{te}'
            kw = dict(pca_dim=D) if te is None else dict(target_energy=te)
            scr, pca_dim, acvar = score(lib, plda, x, **kw)
            assert pca_dim == D if te is None else pca_dim <= T - 1, (name, pca_dim)
            e_margin = np.inf if te is None else np.abs(ratios - te).min()
            noise = np.random.default_rng(1000 * T + pca_dim).standard_normal(x.shape)
            moved, pca_dim2, _ = score(lib, plda, x * (1.0 + 1e-15 * noise), **kw)
            assert pca_dim2 == pca_dim
            tol = 100.0 * np.abs(moved - scr).max()
            thr, _ = lib.twoGMMcalib_lin(scr.ravel())
            lin_mat = linkage(squareform(-scr, checks=False), method='average')         # vbhmm.py:139-141
            adjust = abs(lin_mat[:, 2].min())
            lin_mat[:, 2] += adjust
            cut = -(thr + 0.0) + adjust
            labels = fcluster(lin_mat, cut, criterion='distance') - 1                   # vbhmm.py:142-146
            h_margin = np.abs(lin_mat[:, 2] - cut).min()
            assert e_margin > MARGIN and h_margin > MARGIN, (name, e_margin, h_margin)
            iu = np.triu_indices(T)
            upper, diff = scr[iu], (scr.T[iu] - scr[iu]).astype(np.float32)
            assert np.array_equal(upper + diff.astype(np.float64), scr.T[iu])           # every bit of the lower triangle
            out.update({f'{name}/pca_dim': np.array(pca_dim), f'{name}/acvar': acvar, f'{name}/scr_upper': upper,
                        f'{name}/scr_lower_diff': diff, f'{name}/thr': np.array(thr), f'{name}/labels': labels.astype(np.int32),
                        f'{name}/tol': np.array(tol), f'{name}/margins': np.array([e_margin, h_margin])})
            print(f'{name}: pca_dim {pca_dim}  max|S| {np.abs(scr).max():.1f}  asym {np.abs(scr - scr.T).max():.1e}  tol {tol:.1e}  '
                  f'thr {thr:.4f}  clusters {labels.max() + 1}  margins {e_margin:.1e} {h_margin:.1e}')
    path = os.path.join(HERE, 'plda_cases.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
