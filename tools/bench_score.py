#!/usr/bin/env python
"""Timing of the RTTM scorer (vbx_amd/score.py, vbx_rttm_score.hpp) on N synthetic (reference, system) pairs: the device
path (all pairs in one vbx_rttm_score call) next to the numpy path, stage by stage.  Not the headline bench.

A pair is a meeting-like recording: ``--speakers`` reference speakers taking ``--turns`` turns of 0.5 - 8 s over
``--seconds`` s, a fifth of them started before the previous one ends (overlap), and a system output that is the reference
with every boundary moved by up to 0.3 s, 5 % of the turns relabelled and 5 % dropped; times with millisecond decimals.
Seeded.  Stages, host clock, median of ``--reps`` after a warm-up (the device call ends in a stream synchronise):

  prepare      merge the turns, build the cell edges (host, shared by both paths)
  device       pack + vbx_rttm_score: upload, rttm_cells, rttm_acc, rttm_fin, download
  numpy        the same sums in numpy, pair after pair
  mapping      linear_sum_assignment and the record of every pair (host, shared)

One JSON line, appended to ``--out`` (default profiles/bench_score.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def synthetic_pair(rng, n_spk, n_turns, seconds):
    starts = np.sort(rng.uniform(0, seconds, n_turns))
    ref = []
    for k, s in enumerate(starts):
        dur = rng.uniform(0.5, 8.0)
        if k and rng.random() < 0.2:
            s = max(0.0, ref[-1][1] - rng.uniform(0.1, 1.0))          # starts inside the previous turn
        ref.append((round(float(s), 3), round(float(s + dur), 3), int(rng.integers(n_spk))))
    hyp = []
    for b, e, spk in ref:
        if rng.random() < 0.05:
            continue
        b2, e2 = b + rng.uniform(-0.3, 0.3), e + rng.uniform(-0.3, 0.3)
        if rng.random() < 0.05:
            spk = int(rng.integers(n_spk))
        if e2 > b2:
            hyp.append((round(float(max(b2, 0.0)), 3), round(float(e2), 3), f's{spk}'))
    return ref, hyp


def median_ms(fn, reps):
    fn()                                                              # warm-up: code objects, allocator
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times)), [min(times), max(times)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--pairs', type=int, default=1000)
    ap.add_argument('--speakers', type=int, default=4)
    ap.add_argument('--turns', type=int, default=300)
    ap.add_argument('--seconds', type=float, default=1200.0)
    ap.add_argument('--collar', type=float, default=0.25)
    ap.add_argument('--ignore_overlaps', action='store_true')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bench_score.jsonl'))
    opts = ap.parse_args()
    from vbx_amd import _capi, score
    ctx = _capi.default_context(opts.device)                          # no device: an error, not a fall-back
    rng = np.random.default_rng(0)
    pairs = [synthetic_pair(rng, opts.speakers, opts.turns, opts.seconds) for _ in range(opts.pairs)]
    keep = {}

    def prepare():
        keep['preps'] = [score._Pair(ref, hyp, opts.collar) for ref, hyp in pairs]

    def device():
        keep['dev'] = _capi.rttm_score(ctx, *score._pack(keep['preps']), opts.collar, opts.ignore_overlaps)

    def numpy_path():
        keep['host'] = [score._host_totals(p, opts.collar, opts.ignore_overlaps) for p in keep['preps']]

    def mapping():
        keep['records'] = [score._record(p, *t) for p, t in zip(keep['preps'], keep['host'])]

    prep_ms, prep_mm = median_ms(prepare, max(3, opts.reps // 2))
    dev_ms, dev_mm = median_ms(device, opts.reps)
    host_ms, host_mm = median_ms(numpy_path, max(3, opts.reps // 2))
    map_ms, map_mm = median_ms(mapping, max(3, opts.reps // 2))
    # the two paths on the same cells: the largest difference of any total, relative to the pair's scored reference time
    off, worst = 0, 0.0
    for p, (tot, C) in zip(keep['preps'], keep['host']):
        n = 4 + p.n_ref * p.n_sys
        got = keep['dev'][off:off + n]
        worst = max(worst, float(np.abs(got - np.concatenate([tot, C.ravel()])).max() / max(tot[0], 1.0)))
        off += n
    preps = keep['preps']
    pooled = score._pool(keep['records'])
    line = {'pairs': opts.pairs, 'speakers': opts.speakers, 'turns_per_pair': opts.turns, 'seconds': opts.seconds, 'collar': opts.collar,
            'ignore_overlaps': opts.ignore_overlaps, 'cells_total': int(sum(max(p.edges.size - 1, 0) for p in preps)),
            'cells_per_pair_median': float(np.median([p.edges.size - 1 for p in preps])),
            'merged_turns_total': int(sum(p.rb.size + p.sb.size for p in preps)), 'device': ctx.device_info()['name'],
            'prepare_ms': prep_ms, 'prepare_min_max_ms': prep_mm, 'device_ms': dev_ms, 'device_min_max_ms': dev_mm, 'device_reps': opts.reps,
            'numpy_ms': host_ms, 'numpy_min_max_ms': host_mm, 'mapping_ms': map_ms, 'mapping_min_max_ms': map_mm,
            'sums_speedup': host_ms / dev_ms, 'end_to_end_speedup': (prep_ms + host_ms + map_ms) / (prep_ms + dev_ms + map_ms),
            'max_rel_diff_device_numpy': worst, 'overall_der': pooled['der']}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, 'a') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
