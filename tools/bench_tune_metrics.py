#!/usr/bin/env python
"""Seconds of scoring a grid search's label sequences with all eleven columns of dscore's table: ``metrics.score_labels(device)``
-- the reference's side prepared once per recording, the turns of every hypothesis built on the device -- against
``metrics.score_turns(device)`` on the turns of the same labels (built beforehand, not timed), the only route there was
before it: one host preparation per (reference, hypothesis) pair.  In this process, medians of ``--runs`` after ``--warmup``.
One JSON line, appended to ``--out`` (default profiles/bench_tune_metrics.jsonl).

    python tools/bench_tune_metrics.py [--recordings 64] [--xvectors 1000] [--runs 5] [--warmup 1] [--criterion jer]

Input: tests/tune_util.py -- generated recordings of ``--xvectors`` x-vectors with reference turns from the generator's
speakers; the label sequences are those of ``python -m vbx_amd.tune`` on the 3 x 3 x 3 grid of tools/bench_tune.py (1728
sequences at the defaults), collar 0.25, step 0.010.  The condition the line reports (``within_spread``): the median of
``score_labels`` is no more than the median of ``score_turns`` plus the spread (max - min) of its runs.  Both routes must give
the same integers for every pair (``same_integers``) and the same eleven figures (``same_columns``).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, os.path.join(REPO, 'tools'))

INTEGERS = ('ref_durs', 'sys_durs', 'inter', 'cm')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--recordings', type=int, default=64)
    ap.add_argument('--xvectors', type=int, default=1000)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--criterion', default='jer', help='the column the search of this run is judged by (its timing is reported)')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bench_tune_metrics.jsonl'))
    opts = ap.parse_args(argv)
    import tune_util
    from bench_tune import GRID, median_s
    from vbx_amd import _capi, metrics, score, tune
    from vbx_amd.kaldi_formats import read_xvector_timing_dict
    tmp = tempfile.mkdtemp(prefix='bench_tune_metrics_')
    p = tune_util.make_dev_set(tmp, opts.recordings, opts.xvectors)
    grid_argv = [a for k, vs in GRID.items() for a in ['--' + k] + [str(v) for v in vs]]
    points = tune.grid_points(**GRID)
    args = tune.build_parser().parse_args(tune_util.data_argv(p) + grid_argv + ['--criterion', opts.criterion])
    result = tune.tune(args, log=lambda *a: None)                    # (the process's first calls: start-up included)
    by_der = tune.best_point(result['pooled'], 'der')
    device = _capi.default_context().device
    segs = read_xvector_timing_dict(p['seg'])
    ref = tune.read_reference(p['ref'], result['names'])
    items = [(ref[n], *segs[n][1].T, [result['labels'][g][k] for g in range(len(points))]) for k, n in enumerate(result['names'])]
    pairs = [(it[0], score.labels_turns(it[1], it[2], lab)) for it in items for lab in it[3]]
    keep = {}
    new_s, new_runs = median_s(lambda: keep.update(new=metrics.score_labels(items, 0.25, False, 0.010, device)), opts.runs, opts.warmup)
    old_s, old_runs = median_s(lambda: keep.update(old=metrics.score_turns(pairs, 0.25, False, 0.010, device)), opts.runs, opts.warmup)
    flat = [r for per_item in keep['new'] for r in per_item]
    splits = []
    for _ in range(opts.runs):
        split = {}
        metrics.score_labels(items, 0.25, False, 0.010, device, timing=split)
        splits.append(split)
    counts_split = {}
    metrics.frame_counts_labels(items, 0.010, device, timing=counts_split)
    spread = max(old_runs) - min(old_runs)
    line = dict(tool='bench_tune_metrics', recordings=opts.recordings, xvectors_per_recording=opts.xvectors, grid=GRID, points=len(points),
                collar=0.25, step=0.010, runs=opts.runs, warmup=opts.warmup, pairs=len(pairs),
                system_turns=sum(len(hyp) for _, hyp in pairs), reference_turns=sum(len(score.merge_turns(it[0], touching=False)) for it in items),
                score_labels_s=new_s, score_labels_runs_s=[round(v, 4) for v in new_runs], score_turns_s=old_s,
                score_turns_runs_s=[round(v, 4) for v in old_runs], score_turns_spread_s=spread, factor_turns_over_labels=old_s / new_s,
                within_spread=new_s <= old_s + spread,
                score_labels_split_s={k: round(statistics.median(s[k] for s in splits), 4) for k in ('prepare', 'device', 'mapping', 'columns')},
                frame_counts_labels_split_s={k: round(v, 4) for k, v in counts_split.items()},
                same_integers=all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
                                  for a, b in zip(flat, keep['old']) for k in INTEGERS),
                same_columns=all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for a, b in zip(flat, keep['old']) for k in metrics.COLUMNS),
                criterion=opts.criterion, best=result['best'], best_by_der=by_der,
                pooled_best={k: round(result['pooled'][result['best']][k], 4) for k in metrics.COLUMNS},
                pooled_best_by_der={k: round(result['pooled'][by_der][k], 4) for k in metrics.COLUMNS},
                tune_stages_s={k: round(v, 4) for k, v in result['timing'].items() if isinstance(v, float)},
                device=_capi.default_context().device_info()['name'])
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, 'a') as f:
        f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
