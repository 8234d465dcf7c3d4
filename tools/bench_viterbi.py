#!/usr/bin/env python3
"""Device time of the Viterbi decode (vbx_batch_get_path) beside the vbx_batch_run it follows, and the NumPy referee's time.

Shapes: 64 recordings of T = 10 000, S = 30; one recording of T = 200 000, S = 50; one recording of
S = 1024, T = 2 000.  Per shape: a warm-up, then three runs; the run's device time is vbx_batch_last_run_ms, the decode's the
sum over the recordings of vbx_viterbi_last_ms (the decode kernel and the second-speaker kernel between two events on the
stream).  Cycles per frame = decode time of one recording x clock / T.  One JSON record per shape is appended to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

SHAPES = [dict(name='64 x T=10000 S=30', n=64, T=10000, S=30), dict(name='1 x T=200000 S=50', n=1, T=200000, S=50),
          dict(name='1 x T=2000 S=1024', n=1, T=2000, S=1024)]


def bench_shape(ctx, shape, iters, precision, clock_mhz, runs=3):
    from vbx_amd import _capi
    from vbx_amd.synth import make_recording
    import viterbi_ref as vr
    n, T, S, D = shape['n'], shape['T'], shape['S'], 128
    X, Phi, _ = make_recording(T, min(S, 30), D=D, seed=1, kappa=0.05)
    X = np.ascontiguousarray(X, dtype=np.float32 if precision != 'fp64' else np.float64)
    g0 = np.random.default_rng(2).gamma(1.0, size=(T, S))
    g0 /= g0.sum(1, keepdims=True)
    batch = _capi.Batch(ctx, [T] * n, [S] * n, D, precision=precision, max_iters=iters)
    lib = ctx._lib
    try:
        run_ms, decode_ms, one_ms = [], [], []
        for r in range(runs + 1):
            for j in range(n):
                batch.set_recording(j, X, Phi, np.full(S, 1.0 / S), g0, 0.9, 0.3, 17.0)
            batch.run(iters, -1e300)
            ms = batch.last_run_ms()
            per = []
            for j in range(n):
                first, _second = batch.path(j)
                per.append(lib.vbx_viterbi_last_ms())
            if r:                                             # (the first round warms up)
                run_ms.append(ms[0] if isinstance(ms, tuple) else ms)
                decode_ms.append(sum(per))
                one_ms.append(float(np.median(per)))
        res = batch.result(0)
    finally:
        batch.close()
    # the referee on the host: the recursion in longdouble on what the device decoded (log-likelihoods of the last model)
    lls = np.log(np.maximum(res['gamma'], 1e-300))            # (any [T][S] array costs the referee the same)
    t0 = time.perf_counter()
    vr.structured(lls, 0.9, np.full(S, 1.0 / S))
    host_s = time.perf_counter() - t0
    one = float(np.median(one_ms))
    return dict(shape=shape['name'], recordings=n, T=T, S=S, precision=precision, iterations=iters,
                run_ms=[round(v, 3) for v in run_ms], decode_ms=[round(v, 3) for v in decode_ms],
                decode_ms_per_recording=round(one, 4), decode_over_run=round(float(np.median(decode_ms) / np.median(run_ms)), 4),
                cycles_per_frame=round(one * 1e-3 * clock_mhz * 1e6 / T, 1), clock_mhz=clock_mhz,
                referee_host_s=round(host_s, 3))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--iters', type=int, default=40, help='iterations of the run the decode follows (default: %(default)s)')
    p.add_argument('--precision', default='fp32', choices=['fp64', 'fp32', 'fp32-split'])
    p.add_argument('--clock-mhz', type=float, default=2400.0, help='shader clock the cycles per frame are counted at')
    p.add_argument('--shapes', type=int, nargs='*', default=None, help='indices into the three shapes (default: all)')
    p.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bench_viterbi.jsonl'))
    args = p.parse_args(argv)
    from vbx_amd import _capi
    ctx = _capi.default_context(0)
    for i in (args.shapes if args.shapes is not None else range(len(SHAPES))):
        rec = bench_shape(ctx, SHAPES[i], args.iters, args.precision, args.clock_mhz)
        rec['device'] = ctx.device_info()['name']
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, 'a') as fh:
            fh.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
