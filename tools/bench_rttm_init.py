#!/usr/bin/env python
"""One recording of a batch set from given speaker turns (``--init RTTM+VB``): ``Batch.set_recording_turns``,
where only the window edges and the turns go up and the responsibilities are built on the device, beside the route a caller
without it takes: the NumPy referee of tests/turn_init_ref.py builds ``qinit`` on the host and ``Batch.set_recording`` uploads
it with the recording's rows.

    python tools/bench_rttm_init.py --xvectors 10000 --turns 2000 --speakers 8 --runs 20

The recording: ``--xvectors`` windows of 1.44 s every 0.24 s over seeded rows of 128 dimensions, and ``--turns`` turns of
``--speakers`` speakers laid end to end over the same span with every second one running into the next.  Each route is timed
around whole calls that end in a synchronize (both setters do), after two warm-up calls, ``--runs`` times, the two routes in
turn; the line holds the medians and every time.  The host route is split into the referee and the upload.  The device route
builds rho from resident rows and the host route from uploaded rows -- what each caller actually has to do.  The largest
difference between the two sets of responsibilities is reported beside the times.  One JSON line; appended to ``--out``.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_turns(T, N, S, rng):
    """N turns over the span of T windows, sorted by (speaker, start): consecutive in time, speakers in rotation with a random
    skip, every second turn 0.3 s into the next."""
    a = np.arange(T, dtype=np.int64) * 240000
    b = a + 1440000
    edges = np.sort(rng.choice(np.arange(1, int(b[-1]) // 10000), size=N - 1, replace=False)) * 10000
    u = np.concatenate([[0], edges]).astype(np.int64)
    v = np.concatenate([edges, [int(b[-1])]]).astype(np.int64)
    v[1::2] += 300000
    spk = ((np.arange(N) + rng.integers(0, 2, size=N).cumsum()) % S).astype(np.int32)
    order = np.lexsort((u, spk))
    return a, b, u[order], v[order], spk[order]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--xvectors', type=int, default=10000)
    ap.add_argument('--turns', type=int, default=2000)
    ap.add_argument('--speakers', type=int, default=8)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--precision', default='fp64')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bench_rttm_init.jsonl'))
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import turn_init_ref as ref
    from vbx_amd import _capi
    T, N, S, D = a.xvectors, a.turns, a.speakers, 128
    rng = np.random.default_rng(24)
    seg_a, seg_b, u, v, spk = make_turns(T, N, S, rng)
    x = rng.standard_normal((T, D))
    eye, zero = np.eye(D), np.zeros(D)
    ctx = _capi.default_context(0)
    xv = _capi.XVectors(ctx, x, zero, eye, zero, zero, eye, D)
    fea = xv.get('fea', 0, T)
    Phi = rng.uniform(0.5, 3.0, D)
    hyper = dict(loopProb=0.9, Fa=0.3, Fb=17.0)
    batch = _capi.Batch(ctx, [T, T], [S, S], D, precision=a.precision, max_iters=1)
    times = {'turns': [], 'referee': [], 'upload': []}
    try:
        for run in range(a.runs + 2):
            t0 = time.perf_counter()
            batch.set_recording_turns(0, xv, 0, seg_a, seg_b, u, v, spk, 5.0, Phi, **hyper)
            t1 = time.perf_counter()
            q0 = ref.qinit(ref.weights(seg_a, seg_b, u, v, spk, S)[1], 5.0)
            t2 = time.perf_counter()
            batch.set_recording(1, fea, Phi, np.full(S, 1.0 / S), q0, **hyper)
            batch.sync_uploads()
            t3 = time.perf_counter()
            if run >= 2:
                times['turns'].append(t1 - t0)
                times['referee'].append(t2 - t1)
                times['upload'].append(t3 - t2)
        diff = float(np.abs(batch.result(0, want_model=False)['gamma'] - batch.result(1, want_model=False)['gamma']).max())
    finally:
        batch.close()
        xv.close()
    med = {k: statistics.median(t) for k, t in times.items()}
    line = {'metric': 'one recording of a batch set from speaker turns: Batch.set_recording_turns against the NumPy referee plus '
                      'Batch.set_recording', 'unit': 'ms',
            'config': {'xvectors': T, 'turns': N, 'speakers': S, 'dims': D, 'precision': a.precision, 'runs': a.runs,
                       'bytes_up_turns': int(16 * T + 20 * N), 'bytes_up_qinit': int(8 * T * S)},
            'value': 1e3 * med['turns'],
            'set_recording_turns_ms': 1e3 * med['turns'], 'referee_ms': 1e3 * med['referee'], 'set_recording_upload_ms': 1e3 * med['upload'],
            'host_route_ms': 1e3 * (med['referee'] + med['upload']),
            'all_ms': {k: [round(1e3 * t, 3) for t in ts] for k, ts in times.items()},
            'max_abs_q_difference': diff,
            'note': 'set_recording_turns builds rho from resident rows, set_recording from the T x 128 f64 rows it uploads with qinit'}
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fp:
            fp.write(text + '\n')


if __name__ == '__main__':
    main()
