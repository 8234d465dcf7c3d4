#!/usr/bin/env python
"""Backend training: the two statistics stages on the device beside the same statistics in NumPy on the host.

    python tools/bench_backend.py --rows 1000000 --dims 256 --speakers 7000 --lda-dim 128 --runs 3

Generated data: ``--speakers`` speaker means of standard deviation 1 plus unit noise, float32, the speakers' sizes spread
exponentially about rows / speakers and interleaved.  The device stages are timed between HIP events around their
kernels (``vbx_backend_stage1`` / ``_stage2``: centring and normalisation, class sums and the second moment; for stage 2 the
projection as well), ``--runs`` times after one warm-up; the upload of the rows and the D x D host algebra (the generalised
eigenproblem, the PLDA's EM) are timed once by the wall clock.  The NumPy side computes what the two stages return -- mean1, y,
class sums and second moment of y, then u and its class sums and second moment with the device's lda -- once, with the BLAS of
the host as it is.  One JSON line; appended to ``--out``.

For orientation: the Din = 256 second moment of 1e6 rows is 131 GFLOP in float64 and the float64 rows are 2 GB; at 79 TF/s
of float64 matrix peak and 5 TB/s of HBM that is a floor of about 2 ms for stage 1.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_data(N, D, K, rng):
    """-> (x [N][D] f32, class of every row, numbered by first appearance): speakers of exponentially spread sizes, interleaved."""
    p = rng.exponential(size=K) + 0.05
    cls = rng.choice(K, size=N, p=p / p.sum())
    _, first, cls = np.unique(cls, return_index=True, return_inverse=True)      # (without the speakers that drew no row)
    cls = np.argsort(np.argsort(first))[cls].astype(np.int32)
    means = rng.standard_normal((int(cls.max()) + 1, D), dtype=np.float32)
    x = rng.standard_normal((N, D), dtype=np.float32)
    x += means[cls]
    return x, cls


def class_sums_numpy(r, order, starts):
    return np.add.reduceat(r[order], starts, axis=0)


def numpy_stages(x, cls, lda, mean2):
    """What the two device stages return, in float64 NumPy.  -> (results, seconds per stage)"""
    order = np.argsort(cls, kind='stable')
    starts = np.concatenate([[0], np.cumsum(np.bincount(cls))[:-1]])
    t0 = time.perf_counter()
    x64 = x.astype(np.float64)
    mean1 = x64.mean(axis=0)
    y = x64 - mean1
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    ysum, ymom = class_sums_numpy(y, order, starts), y.T.dot(y)
    t1 = time.perf_counter()
    u = y.dot(lda) - mean2
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    usum, umom = class_sums_numpy(u, order, starts), u.T.dot(u)
    t2 = time.perf_counter()
    return dict(mean1=mean1, ysum=ysum, ymom=ymom, usum=usum, umom=umom), (t1 - t0, t2 - t1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rows', type=int, default=1000000)
    ap.add_argument('--dims', type=int, default=256)
    ap.add_argument('--speakers', type=int, default=7000)
    ap.add_argument('--lda-dim', type=int, default=128)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bench_backend.jsonl'))
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    from vbx_amd import _capi, backend
    rng = np.random.default_rng(25)
    x, cls = make_data(a.rows, a.dims, a.speakers, rng)
    N, D, K = x.shape[0], x.shape[1], int(cls.max()) + 1
    counts = np.bincount(cls).astype(np.int64)
    ctx = _capi.default_context(0)
    print(f'{N} rows x {D}, {K} speakers of {counts.min()} ... {counts.max()} rows', flush=True)

    t0 = time.perf_counter()
    be = _capi.BackendStats(ctx, x, cls, K)
    upload_s = time.perf_counter() - t0
    ms1, ms2, wall1, wall2 = [], [], [], []
    try:
        for run in range(a.runs + 1):
            t0 = time.perf_counter()
            mean1, ysum, ymom = be.stage1()
            t1 = time.perf_counter()
            if run == 0:
                ybar = ysum.sum(axis=0) / N
                St = ymom - N * np.outer(ybar, ybar)
                Sb = _capi.backend_second_moments(ctx, np.sqrt(counts)[:, None] * (ysum / counts[:, None] - ybar), [0, K])[0]
                lda, mean2 = backend.estimate_lda(ybar, St, Sb, a.lda_dim)
                lda_s = time.perf_counter() - t1
            t1 = time.perf_counter()
            usum, umom = be.stage2(lda, mean2)
            t2 = time.perf_counter()
            if run:
                ms1.append(be.kernel_ms[0])
                ms2.append(be.kernel_ms[1])
                wall1.append((t1 - t0) * 1e3)
                wall2.append((t2 - t1) * 1e3)
            print(f'run {run}: stage 1 {be.kernel_ms[0]:.2f} ms, stage 2 {be.kernel_ms[1]:.2f} ms on the device', flush=True)
    finally:
        be.close()
    t0 = time.perf_counter()
    mu = usum / counts[:, None]
    mean = mu.sum(axis=0) / K
    between = _capi.backend_second_moments(ctx, np.sqrt(counts)[:, None] * mu, [0, K])[0]
    order, n, off = backend.count_groups(counts)
    G = _capi.backend_second_moments(ctx, mu[order] - mean, off)
    scatters_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    backend.estimate_plda(n, np.diff(off), G, umom - between, N, mean, 10)
    em_s = time.perf_counter() - t0

    ref, (np1, np2) = numpy_stages(x, cls, lda, mean2)
    rel = lambda got, want: float(np.abs(got - want).max() / np.abs(want).max())
    diffs = dict(mean1=rel(mean1, ref['mean1']), y_class_sums=rel(ysum, ref['ysum']), y_moment=rel(ymom, ref['ymom']),
                 u_class_sums=rel(usum, ref['usum']), u_moment=rel(umom, ref['umom']))
    stage1 = statistics.median(ms1)
    flop, row_bytes = 2.0 * N * D * D, 8.0 * N * D
    floor_ms = max(flop / 79e12, row_bytes / 5e12) * 1e3
    line = {
        'metric': 'backend training, the two statistics stages on the device: median kernel time of stage 1 (centre + normalise, '
                  'class sums, second moment of y) between HIP events',
        'unit': 'ms', 'value': stage1,
        'config': {'rows': N, 'dims': D, 'speakers': K, 'lda_dim': a.lda_dim, 'runs': a.runs, 'distinct_class_sizes': int(len(n)),
                   'device': ctx.device_info()['name']},
        'stage1_kernel_ms': stage1, 'stage2_kernel_ms': statistics.median(ms2),
        'stage1_call_ms': statistics.median(wall1), 'stage2_call_ms': statistics.median(wall2),
        'all_kernel_ms': {'stage1': [round(v, 3) for v in ms1], 'stage2': [round(v, 3) for v in ms2]},
        'upload_s': upload_s, 'lda_host_s': lda_s, 'class_mean_scatters_s': scatters_s, 'plda_em_host_s': em_s,
        'numpy_stage1_ms': np1 * 1e3, 'numpy_stage2_ms': np2 * 1e3,
        'speedup_stage1': np1 * 1e3 / stage1, 'speedup_stage2': np2 * 1e3 / statistics.median(ms2),
        'stage1_floor_ms': floor_ms, 'stage1_over_floor': stage1 / floor_ms,
        'moment_tflops_if_all_of_stage1': flop / (stage1 * 1e-3) / 1e12,
        'max_rel_diff_to_numpy': diffs,
    }
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as fd:
        fd.write(text + '\n')


if __name__ == '__main__':
    main()
