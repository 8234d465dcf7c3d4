#!/usr/bin/env python
"""What scoring against reference labels costs: milliseconds per iteration (wall clock around the calls, host work included)
for (a) no labels, (b) labels scored on the device (vbx_batch_set_reference: one run, then the history and the Hungarian
assignment per iteration on the host), (c) the per-iteration host path of VBX_AMD_REF_SCORING=host (one run(1), one download
of the responsibilities and two DER() calls per iteration).  One JSON line per shape:

    one recording of T = 10 000, S = 30          fp64 and fp32
    the headline batch, 64 x (T = 10 000, S = 30) fp32-split
    the nine-point grid over T = 200 000, S = 50  fp32-split, (a) and (b) only: a sweep has no host path

    python tools/bench_ref.py [single] [batch] [sweep]      (default: all three)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ITERS = 20


def _inputs(n_rec, T, S, seed0=0):
    from vbx_amd.synth import make_recording
    out = []
    for b in range(n_rec):
        X, Phi, labels = make_recording(T, S, seed=seed0 + b, kappa=0.05, dtype=np.float32)
        g = np.random.default_rng(10_000 + seed0 + b).gamma(1.0, size=(T, S))
        out.append((X, Phi, g / g.sum(1, keepdims=True), labels))
    return out


def _fill(batch, inputs, S, labels, points=None):
    if points:                                               # a sweep: the other points share recording 0's x-vectors
        X, Phi, g, lab = inputs[0]
        for k, (fa, fb) in enumerate(points):
            if k:
                batch.set_recording_shared(k, 0, np.ones(S) / S, g, 0.9, fa, fb)
            else:
                batch.set_recording(0, X, Phi, np.ones(S) / S, g, 0.9, fa, fb)
    else:
        for b, (X, Phi, g, lab) in enumerate(inputs):
            batch.set_recording(b, X, Phi, np.ones(S) / S, g, 0.99, 0.3, 17.0)
    for b in range(batch.n):
        if labels:
            batch.set_reference(b, inputs[0 if points else b][3])


def measure(make, inputs, S, mode, points=None, reps=3):
    """best of `reps`: (wall ms per iteration, device ms per iteration of the run itself or None)"""
    from vbx_amd import _capi, DER, der_from_confusion
    best, dev = np.inf, None
    for rep in range(reps + 1):                              # (the first one warms up)
        batch = make()
        try:
            _fill(batch, inputs, S, labels=mode == 'device', points=points)
            batch.sync_uploads()
            t0 = time.perf_counter()
            if mode == 'host':
                batch.set_option(_capi.OPT_CHECK_EVERY, 1)
                for _ in range(ITERS):
                    batch.run(1, -np.inf)
                    for b, res in enumerate(batch.results(want_model=False)):
                        DER(res['gamma'], inputs[b][3])
                        DER(res['gamma'], inputs[b][3], xentropy=True)
            else:
                batch.run(ITERS, -np.inf)
                if mode == 'device':
                    for b in range(batch.n):
                        T = batch.T[b]
                        for c in batch.scores(b):
                            der_from_confusion(c, T)
                            der_from_confusion(c, T, xentropy=True)
            wall = 1e3 * (time.perf_counter() - t0) / ITERS
            if rep and wall < best:
                best = wall
                dev = None if mode == 'host' else batch.last_run_ms()[0] / ITERS
        finally:
            batch.close()
    return best, dev


def report(name, make, inputs, S, modes, points=None):
    out = {'shape': name, 'iterations': ITERS}
    for key, mode in (('a_no_labels', 'none'), ('b_device', 'device'), ('c_host', 'host')):
        if mode not in modes:
            continue
        wall, dev = measure(make, inputs, S, mode, points=points)
        out[key + '_ms_per_iteration'] = round(wall, 4)
        if dev is not None:
            out[key + '_device_ms_per_iteration'] = round(dev, 4)
    print(json.dumps(out), flush=True)


def main(which):
    from vbx_amd import _capi
    ctx = _capi.default_context(0)
    if 'single' in which:
        inputs = _inputs(1, 10000, 30)
        for precision in ('fp64', 'fp32'):
            report(f'1 x T=10000 S=30 {precision}', lambda: _capi.Batch(ctx, [10000], [30], 128, precision=precision, max_iters=ITERS),
                   inputs, 30, ('none', 'device', 'host'))
    if 'batch' in which:
        inputs = _inputs(64, 10000, 30)
        report('64 x T=10000 S=30 fp32-split', lambda: _capi.Batch(ctx, [10000] * 64, [30] * 64, 128, precision='fp32-split', max_iters=ITERS),
               inputs, 30, ('none', 'device', 'host'))
    if 'sweep' in which:
        from vbx_amd.batch import sweep_streams
        points = [(fa, fb) for fa in (0.2, 0.3, 0.4) for fb in (6.0, 17.0, 64.0)]
        inputs = _inputs(1, 200000, 50)
        report('9 points x T=200000 S=50 fp32-split',
               lambda: _capi.Batch(ctx, [200000] * 9, [50] * 9, 128, precision='fp32-split', max_iters=ITERS, streams=sweep_streams(9, 200000)),
               inputs, 50, ('none', 'device'), points=points)


if __name__ == '__main__':
    main(sys.argv[1:] or ['single', 'batch', 'sweep'])
