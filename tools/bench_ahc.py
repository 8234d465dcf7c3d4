#!/usr/bin/env python
"""Timing of the AHC score stage (vbhmm.py:135-138) on the GPU next to the CPU oracle (NumPy restatement of
diarization_lib.cos_similarity / twoGMMcalib_lin).  One JSON line per size.  Not the headline bench.

``--scores plda``: the Kaldi-recipe PLDA similarity instead (diarization_lib.kaldi_ivector_plda_scoring_dense): the stage
as ``vbhmm --ahc-scores plda`` runs it -- resident rows in, T x T scores resident in HBM out -- next to the only route
there was without it: the same scores computed by NumPy on the host and pushed through ``Scores.upload``.  Medians of
repeated runs after a warm-up; both routes end in a device synchronise."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_plda_scores(plda, x, target_energy):
    """kaldi_ivector_plda_scoring_dense on the host: NumPy / SciPy, the operations the reference runs."""
    from scipy.linalg import eigh
    from vbx_amd.diarization_lib import plda_pca_dim, plda_projection
    energy, PCA = eigh(np.cov(x.T, bias=True))
    pca_dim = plda_pca_dim(target_energy, x.shape[1], energy, len(x))
    M, acvar = plda_projection(plda, PCA[:, :-pca_dim - 1:-1])
    y = (x - plda[0]).dot(M)
    y *= np.sqrt(y.shape[1] / np.dot(y ** 2, 1.0 / (acvar + 1.0)))[:, np.newaxis]
    wc2ac = 1.0 / (1.0 + 2.0 * acvar)
    Gamma, Lambda = -0.25 * (wc2ac + 1.0 - 2.0 / (1.0 + acvar)), -0.5 * (wc2ac - 1.0)
    k = -0.5 * (np.sum(np.log(1.0 + 2.0 * acvar)) - 2.0 * np.sum(np.log(1.0 + acvar)))
    q = (y ** 2).dot(Gamma)
    return np.dot(y * Lambda, y.T) + q[:, np.newaxis] + q + k


def median_ms(fn, reps):
    fn()                                                              # warm-up: code objects, allocator, BLAS pool
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times)), times


def bench_plda(sizes, target_energy, reps):
    from vbx_amd import _capi
    from vbx_amd.diarization_lib import plda_dense_scores, plda_projection
    ctx = _capi.default_context(0)
    rng = np.random.default_rng(0)
    D = 128
    q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    plda = (0.05 * rng.standard_normal(D), q * rng.uniform(0.5, 2.0, D)[:, None], np.sort(rng.uniform(0.05, 20.0, D))[::-1].copy())
    full = plda_projection(plda, None) if target_energy >= 1.0 else None      # (the driver computes it once per archive)
    for T in sizes:
        centres = rng.standard_normal((6, D))
        x = centres[rng.integers(0, 6, T)] + 0.8 * rng.standard_normal((T, D))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        xv = _capi.XVectors(ctx, x, np.zeros(D), np.eye(D), np.zeros(D), plda[0], np.eye(D), D)      # xproj = x up to rounding
        rows = xv.get('xproj')
        keep = {}

        def device():
            sc, keep['pca_dim'] = plda_dense_scores(ctx, plda, resident=(xv, 0, T), target_energy=target_energy, full_projection=full)
            sc.close()                                                # (every entry point ends in a stream synchronise)

        def host():
            sc = _capi.Scores.upload(ctx, host_plda_scores(plda, rows, target_energy))
            sc.close()

        def host_compute_only():
            keep['host'] = host_plda_scores(plda, rows, target_energy)

        dev_ms, dev_all = median_ms(device, reps)
        host_ms, host_all = median_ms(host, max(3, reps // 3))
        comp_ms, _ = median_ms(host_compute_only, max(3, reps // 3))
        sc, _ = plda_dense_scores(ctx, plda, resident=(xv, 0, T), target_energy=target_energy, full_projection=full)
        S = sc.get().reshape(T, T)
        sc.close()
        xv.close()
        print(json.dumps({'scores': 'plda', 'T': T, 'D': D, 'target_energy': target_energy, 'pca_dim': int(keep['pca_dim']),
                          'gpu_resident_rows_to_scores_ms': dev_ms, 'gpu_min_max_ms': [min(dev_all), max(dev_all)], 'gpu_reps': reps,
                          'host_numpy_plus_upload_ms': host_ms, 'host_min_max_ms': [min(host_all), max(host_all)],
                          'host_numpy_only_ms': comp_ms, 'speedup': host_ms / dev_ms,
                          'max_abs_diff_to_host': float(np.abs(S - keep['host']).max()), 'max_abs_score': float(np.abs(S).max()),
                          'symmetric': bool(np.array_equal(S, S.T))}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--scores', choices=['cos', 'plda'], default='cos')
    ap.add_argument('--sizes', type=int, nargs='+', default=None, help='numbers of x-vectors (plda: 1025 4000 10000)')
    ap.add_argument('--target-energy', type=float, default=0.5, help='plda: share of the variability the PCA keeps (>= 1: all of it)')
    ap.add_argument('--reps', type=int, default=15, help='plda: timed repetitions of the device route (the host route runs a third)')
    opts = ap.parse_args()
    if opts.scores == 'plda':
        return bench_plda(opts.sizes or [1025, 4000, 10000], opts.target_energy, opts.reps)
    from vbx_amd import _capi
    from vbx_amd.diarization_lib import cos_similarity, twoGMMcalib_lin
    from oracle import ahc_oracle
    ctx = _capi.default_context(0)
    rng = np.random.default_rng(0)
    for T in opts.sizes or (1025, 10000):
        centres = rng.standard_normal((6, 128))
        x = centres[rng.integers(0, 6, T)] + 0.8 * rng.standard_normal((T, 128))
        cos_similarity(x[:64])                                        # warm-up
        t0 = time.perf_counter()
        sc = _capi.Scores.cos_similarity(ctx, x)                       # device only (H2D of x included)
        t1 = time.perf_counter()
        thr, _ = sc.two_gmm_calib(20, want_llr=False)
        t2 = time.perf_counter()
        scr = cos_similarity(x)                                        # as vbhmm.py calls it: + D2H of T*T doubles
        t3 = time.perf_counter()
        thr2, llr = twoGMMcalib_lin(scr.ravel())                       # resident matrix, + D2H of the LLRs
        t4 = time.perf_counter()
        out = {'T': T, 'D': 128, 'gpu_cos_similarity_ms': 1e3 * (t1 - t0), 'gpu_twoGMMcalib_20_ms': 1e3 * (t2 - t1),
               'api_cos_similarity_ms_with_d2h': 1e3 * (t3 - t2), 'api_twoGMMcalib_ms_with_llr_d2h': 1e3 * (t4 - t3),
               'gmm_pass_GBs': 20 * 8 * T * T / (t2 - t1) / 1e9, 'threshold': float(thr)}
        if T <= 10000:
            c0 = time.perf_counter()
            so = ahc_oracle.cos_similarity(x)
            c1 = time.perf_counter()
            to, _ = ahc_oracle.twoGMMcalib_lin(so.ravel(), niters=20 if T < 5000 else 2)
            c2 = time.perf_counter()
            out.update({'cpu_oracle_cos_similarity_ms': 1e3 * (c1 - c0),
                        'cpu_oracle_twoGMMcalib_ms_per_pass': 1e3 * (c2 - c1) / (20 if T < 5000 else 2)})
        print(json.dumps(out))
        sc.close()


if __name__ == '__main__':
    main()
