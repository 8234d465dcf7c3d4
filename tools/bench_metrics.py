#!/usr/bin/env python
"""Timing of the frame counts behind dscore's full table (vbx_amd/metrics.py, vbx_frame_score.hpp) on N synthetic
(reference, system) pairs shaped like the tuning loop's: the device route (all pairs in one vbx_frame_counts call) next to
the module's numpy route, and the dense referee of the tests on one pair.  Not the headline bench.

A pair is ``tools/bench_score.py``'s meeting-like recording: ``--speakers`` reference speakers taking ``--turns`` turns of
0.5 - 8 s over ``--seconds`` s, a fifth of them overlapping the previous one, and a system output that is the reference with
every boundary moved, 5 % of the turns relabelled and 5 % dropped.  Seeded.  Stages, host clock, median of ``--reps`` after
a warm-up (the device call ends in a stream synchronise):

  prepare      merge the turns, name the speakers (host, shared by both routes)
  device       pack + vbx_frame_counts: upload, the six kernels of phase 1, the class counts back, frame_acc, download
  numpy        the same cells in numpy, pair after pair
  columns      JER, B-cubed, GKT, entropies of every pair from the integers (host, shared)
  referee      tests/metrics_ref.py, one boolean row per frame, on the first pair alone

One JSON line, appended to ``--out`` (default profiles/bench_metrics.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, os.path.join(REPO, 'tools'))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--pairs', type=int, default=300)
    ap.add_argument('--speakers', type=int, default=4)
    ap.add_argument('--turns', type=int, default=2000)
    ap.add_argument('--seconds', type=float, default=7200.0)
    ap.add_argument('--step', type=float, default=0.010)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bench_metrics.jsonl'))
    opts = ap.parse_args()
    import metrics_ref
    from bench_score import median_ms, synthetic_pair
    from vbx_amd import _capi, metrics
    ctx = _capi.default_context(opts.device)                          # no device: an error, not a fall-back
    rng = np.random.default_rng(0)
    pairs = [synthetic_pair(rng, opts.speakers, opts.turns, opts.seconds) for _ in range(opts.pairs)]
    keep = {}

    def prepare():
        keep['preps'] = [metrics._Frames(ref, hyp) for ref, hyp in pairs]

    def device():
        keep['dev'] = metrics._device_counts(keep['preps'], opts.step, opts.device)

    def numpy_route():
        keep['host'] = [metrics._host_counts(p, opts.step) for p in keep['preps']]

    def columns():
        keep['columns'] = [(metrics._jer(r), metrics._clustering(r['cm'])) for r in keep['host']]

    def referee():
        keep['referee'] = metrics_ref.counts(*pairs[0], opts.step)

    prep_ms, prep_mm = median_ms(prepare, max(3, opts.reps // 2))
    dev_ms, dev_mm = median_ms(device, opts.reps)
    host_ms, host_mm = median_ms(numpy_route, max(3, opts.reps // 2))
    col_ms, col_mm = median_ms(columns, max(3, opts.reps // 2))
    ref_ms, ref_mm = median_ms(referee, 3)
    fell_back = sum(d is None for d in keep['dev'])
    for d, h in zip(keep['dev'], keep['host']):                       # integers: the routes agree exactly or the line is not written
        if d is not None:
            metrics_ref.assert_counts_equal(d, h, 'device against numpy')
    metrics_ref.assert_counts_equal(keep['host'][0], keep['referee'], 'numpy against the referee')
    preps = keep['preps']
    line = {'pairs': opts.pairs, 'speakers': opts.speakers, 'turns_per_pair': opts.turns, 'seconds': opts.seconds, 'step': opts.step,
            'merged_turns_total': int(sum(p.rb.size + p.sb.size for p in preps)),
            'frames_total': int(sum(int(h['cm'].sum()) for h in keep['host'])),
            'classes_per_pair_median': [float(np.median([h['cm'].shape[k] for h in keep['host']])) for k in (0, 1)],
            'pairs_over_the_class_cap': int(fell_back), 'device': ctx.device_info()['name'],
            'prepare_ms': prep_ms, 'prepare_min_max_ms': prep_mm, 'device_ms': dev_ms, 'device_min_max_ms': dev_mm, 'device_reps': opts.reps,
            'numpy_ms': host_ms, 'numpy_min_max_ms': host_mm, 'columns_ms': col_ms, 'columns_min_max_ms': col_mm,
            'referee_one_pair_ms': ref_ms, 'referee_one_pair_min_max_ms': ref_mm, 'counts_speedup': host_ms / dev_ms,
            'device_equals_numpy': True, 'numpy_equals_referee_on_pair_0': True}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, 'a') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
