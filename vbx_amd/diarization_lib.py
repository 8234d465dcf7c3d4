"""Host-side mirror of the score stage of the reference's AHC initialisation on top of libvbx_hip.so.

``vbhmm.py:135-138`` computes, right before it calls ``VBx()``::

    scr_mx = cos_similarity(x)                       # diarization_lib.py:190-213, T x T float64
    thr, _ = twoGMMcalib_lin(scr_mx.ravel())         # diarization_lib.py:13-31, 20 EM passes over T*T scores

Both functions keep the reference's signatures, return types and error behaviour; the work runs in HIP
kernels (f64 MFMA for the similarity matrix, one streaming kernel per EM pass).  ``cos_similarity`` returns an
ordinary, writable ndarray like the reference's (callers edit it in place: ``np.fill_diagonal``, ``scr_mx *= -1``,
masks), and ``twoGMMcalib_lin`` uploads whatever vector it is handed: the host array is the only truth, so an in-place
edit between the two calls cannot go unnoticed.  (Round 2 kept the device copy of the matrix alive behind a read-only
array and spot-checked it; a full check costs more than the 8 T^2 bytes over PCIe it saved.)  Callers that want the
matrix to stay in HBM between the two steps use ``vbx_amd._capi.Scores`` directly, as ``vbx_amd.vbhmm`` does.
There is no CPU fallback.

The reference's alternative similarity for the AHC stage, the Kaldi-recipe PLDA scoring, is mirrored as well:
``PLDA_scoring_in_LDA_space`` (diarization_lib.py:34-56) and ``kaldi_ivector_plda_scoring_dense`` (:59-93).  Its two
``eigh`` calls, the ``inv`` and the energy rule work on D x D matrices and stay on the host, as two pure functions
(``plda_pca_dim``, ``plda_projection``); the covariance of the rows, the projection with Kaldi's length normalisation and
the T x T scores run in HIP kernels (vbx_plda_score.hpp).  ``vbx_amd.vbhmm --ahc-scores plda`` scores the resident rows
with ``plda_dense_scores`` and keeps the matrix in HBM for calibration and linkage.
"""
from __future__ import annotations

import warnings

import numpy as np

from . import _capi

__all__ = ['cos_similarity', 'twoGMMcalib_lin', 'PLDA_scoring_in_LDA_space', 'kaldi_ivector_plda_scoring_dense',
           'plda_pca_dim', 'plda_projection', 'plda_dense_scores']


def cos_similarity(x, *, device=None):
    """Cosine similarity matrix of the rows of ``x`` (T x D) -> T x T float64.  diarization_lib.py:190-213."""
    x = np.asarray(x)
    assert x.ndim == 2, f'x has {x.ndim} dimensions, it must be matrix'
    x = np.ascontiguousarray(x, dtype=np.float64)
    # the reference asserts that every row normalises to unit length (diarization_lib.py:201-202)
    norm = np.sqrt(np.sum(np.square(x), axis=1, keepdims=True))
    xn_sq = np.sum(np.square(x / (norm + 1.0e-32)), axis=1)
    assert np.allclose(np.ones_like(xn_sq), xn_sq)
    scores = _capi.Scores.cos_similarity(_capi.default_context(device), x)
    try:
        out = np.empty((x.shape[0], x.shape[0]))
        scores.get(out=out)
    finally:
        scores.close()
    return out


def twoGMMcalib_lin(s, niters=20, *, device=None):
    """Two-Gaussian GMM with shared variance over the scores ``s``: returns the threshold that separates
    the two Gaussians and the linearly calibrated log-odds of every score.  diarization_lib.py:13-31."""
    s = np.asarray(s)
    if s.ndim != 1:
        raise ValueError('twoGMMcalib_lin expects a vector of scores')     # the reference's s[:, np.newaxis] needs 1-D
    scores = _capi.Scores.upload(_capi.default_context(device), s)
    try:
        threshold, llr = scores.two_gmm_calib(niters)
    finally:
        scores.close()
    return np.float64(threshold), llr


def PLDA_scoring_in_LDA_space(Fe, Ft, diagAC, *, device=None):
    """N x M matrix of PLDA log-likelihood-ratio scores of the enrollment vectors ``Fe`` (N x D) against the test vectors
    ``Ft`` (M x D), both centred and in the LDA space where the within-class covariance is the identity and the
    across-class covariance is ``diag(diagAC)``.  diarization_lib.py:34-56."""
    Fe, Ft, diagAC = np.asarray(Fe, dtype=np.float64), np.asarray(Ft, dtype=np.float64), np.asarray(diagAC, dtype=np.float64)
    if Fe.ndim != 2 or Ft.ndim != 2 or diagAC.ndim != 1 or not Fe.shape[1] == Ft.shape[1] == diagAC.size:
        raise ValueError(f'PLDA_scoring_in_LDA_space: shapes {Fe.shape}, {Ft.shape}, {diagAC.shape} do not go together')
    return _capi.plda_score_lda(_capi.default_context(device), Fe, Ft, diagAC)


def plda_pca_dim(target_energy, dim, energy=None, n_rows=None):
    """The PCA dimension ``kaldi_ivector_plda_scoring_dense`` keeps (diarization_lib.py:79-82): the number of leading
    principal directions whose share of the variance stays within ``target_energy``, plus two.  ``energy``: eigenvalues of
    the covariance in ascending order (``scipy.linalg.eigh``); ``dim``: its dimension D; ``n_rows``: rows the covariance
    was taken over.

    ``target_energy >= 1`` keeps all D dimensions and needs no eigenvalues: what the reference's rule gives wherever it
    is determinate (with fewer than D + 1 rows it counts the rounding noise of eigenvalues that are zero).  A result
    above ``min(n_rows - 1, dim)`` but below ``dim`` asks for directions in the covariance's null space, which ``eigh``
    picks arbitrarily; the rule is applied literally, as in the reference, and a warning says so."""
    if target_energy >= 1.0:
        return int(dim)
    if energy is None:
        raise ValueError('plda_pca_dim: target_energy < 1 needs the eigenvalues of the covariance')
    cum = np.cumsum(np.asarray(energy, dtype=np.float64)[::-1])
    pca_dim = int(np.sum(cum / cum[-1] <= target_energy) + 2)      # (at least 2 dimensions: 2 more are always added)
    _warn_if_undetermined(pca_dim, dim, n_rows)
    return pca_dim


def _warn_if_undetermined(pca_dim, dim, n_rows):
    if n_rows is not None and min(n_rows - 1, dim) < pca_dim < dim:
        warnings.warn(f'PLDA scoring: pca_dim = {pca_dim} of {dim} dimensions from {n_rows} x-vectors: their covariance has '
                      f'rank {min(n_rows - 1, dim)} at most, the remaining directions are arbitrary and the scores undetermined',
                      RuntimeWarning, stacklevel=3)


def plda_projection(kaldi_plda, PCA):
    """``(M, acvar)`` of diarization_lib.py:87-91 from the Kaldi PLDA model ``(mu, tr, psi)`` and the kept principal
    directions ``PCA`` (D x d, or None for all D: the identity): ``(x - mu).dot(M)`` takes x-vectors into the space
    where the PLDA's within-class covariance is the identity and the across-class covariance is ``diag(acvar)``."""
    from scipy.linalg import eigh
    _mu, plda_tr, plda_psi = kaldi_plda
    plda_tr_inv = np.linalg.inv(np.asarray(plda_tr, dtype=np.float64))
    plda_tr_inv_pca = plda_tr_inv if PCA is None else np.asarray(PCA).T.dot(plda_tr_inv)
    W = plda_tr_inv_pca.dot(plda_tr_inv_pca.T)
    B = (plda_tr_inv_pca * plda_psi).dot(plda_tr_inv_pca.T)
    acvar, wccn = eigh(B, W)
    return (wccn if PCA is None else np.asarray(PCA).dot(wccn)), acvar


def plda_dense_scores(ctx, kaldi_plda, x=None, *, resident=None, target_energy=0.1, pca_dim=None, full_projection=None):
    """The device-resident score matrix (``_capi.Scores``) of ``kaldi_ivector_plda_scoring_dense`` and the PCA dimension
    used.  The rows are the host array ``x`` or, with ``resident = (xvectors, row0, T)``, projected x-vectors already in
    HBM.  ``full_projection``: a cached ``plda_projection(kaldi_plda, None)`` for callers that score many recordings with
    all dimensions kept."""
    if resident is None:
        x = np.ascontiguousarray(x, dtype=np.float64)
        n_rows, dim = x.shape
    else:
        xv, row0, n_rows = resident
        dim = xv.dl
    keep_all = (pca_dim is None and target_energy >= 1.0) or (pca_dim is not None and pca_dim >= dim)
    if keep_all:             # every dimension: the scores do not depend on the basis, no covariance is needed
        pca_dim = dim if pca_dim is None else pca_dim
        M, acvar = full_projection if full_projection is not None else plda_projection(kaldi_plda, None)
    else:
        from scipy.linalg import eigh
        _mean, cov = (_capi.plda_covariance(ctx, x) if resident is None
                      else _capi.plda_covariance_resident(ctx, xv, row0, n_rows))
        energy, PCA = eigh(cov)
        if pca_dim is None:
            pca_dim = plda_pca_dim(target_energy, dim, energy, n_rows)
        else:
            _warn_if_undetermined(pca_dim, dim, n_rows)
        M, acvar = plda_projection(kaldi_plda, PCA[:, :-pca_dim - 1:-1])
    mu = np.asarray(kaldi_plda[0], dtype=np.float64)
    if resident is None:
        return _capi.Scores.plda(ctx, x, mu, M, acvar), pca_dim
    return _capi.Scores.plda_resident(ctx, xv, row0, n_rows, mu, M, acvar), pca_dim


def kaldi_ivector_plda_scoring_dense(kaldi_plda, x, target_energy=0.1, pca_dim=None, *, device=None):
    """N x N matrix of pairwise PLDA similarity scores of the x-vectors ``x`` (N x R) for the AHC that follows, the
    scores of the standard Kaldi diarization recipe.  diarization_lib.py:59-93.

    ``kaldi_plda`` is the model ``(mu, tr, psi)`` as ``read_plda`` loads it.  A PCA estimated on ``x`` keeps at least
    ``target_energy`` of its variability (``pca_dim`` overrides that and names the dimension directly); x-vectors and
    model are projected into that space, length-normalised the Kaldi way and scored.

    Two things differ from a literal run of the reference, both where its result is not defined by its input:
    ``target_energy >= 1`` (or ``pca_dim`` >= R) keeps all R dimensions without estimating a covariance -- equal to the
    reference wherever the reference's own energy rule is determinate; and when the kept dimension exceeds the rank
    ``min(N - 1, R)`` of the covariance while staying below R, the extra directions come from the covariance's null
    space: the reference's scores then change by O(1) under perturbations of 1e-15, this function does literally the
    same and issues a ``RuntimeWarning``.  The returned matrix is symmetric to the last bit."""
    x = np.asarray(x)
    assert x.ndim == 2, f'x has {x.ndim} dimensions, it must be matrix'
    scores, pca_dim = plda_dense_scores(_capi.default_context(device), kaldi_plda, x, target_energy=target_energy, pca_dim=pca_dim)
    print("pca_dim:", pca_dim)
    try:
        out = np.empty((x.shape[0], x.shape[0]))
        scores.get(out=out)
    finally:
        scores.close()
    return out
