#!/usr/bin/env python
"""Seconds of a grid search over Fa, Fb, loopP on a labelled development set: ``python -m vbx_amd.tune`` (one process: read,
project and AHC once, the VB-HMM per grid point, every label sequence scored in one device call) against what there was before
it, one ``python -m vbx_amd.vbhmm ... --ref-rttm-dir`` run per grid point.  Every run in fresh child processes, which is how
users run them; the two routes interleaved.  One JSON line, appended to ``--out`` (default profiles/bench_tune.jsonl).

    python tools/bench_tune.py [--recordings 64] [--xvectors 1000] [--runs 5] [--warmup 1] [--baseline-repo DIR]

Input: tests/tune_util.py -- generated recordings of ``--xvectors`` x-vectors (the golden archive resampled in blocks) with
reference turns from the generator's speakers.  Grid 3 x 3 x 3 round the recipe's values, collar 0.25.  ``--baseline-repo``: a
built checkout of the commit to compare with (the parent); its per-point route is the one timed as ``per_point``, and the line
carries its median and spread (max - min) -- the margin the median of ``tune`` is held against.  Without it the per-point route
runs from this tree.

Then, in this process, on the label sequences of the search: ``score.score_labels(device)`` against ``score.score_turns(device)``
on the turns of the same labels (built beforehand, not timed) -- the reference's side prepared once per recording and the turns
and edges made on the device, against one host preparation per (reference, hypothesis) pair.  Median of ``--runs`` after a
warm-up; held to the same condition.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

GRID = dict(Fa=[0.2, 0.3, 0.4], Fb=[11.0, 17.0, 23.0], loopP=[0.9, 0.95, 0.99])


def child(repo, module_argv, timeout):
    env = dict(os.environ, PYTHONPATH=repo)
    if repo != REPO:                                                  # the other checkout runs ITS library, as it was built
        env['VBX_AMD_LIB'] = os.path.join(repo, 'vbx_amd', 'csrc', 'libvbx_hip.so')
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, '-m'] + module_argv, env=env, cwd=repo, capture_output=True, text=True, timeout=timeout)
    if res.returncode != 0:
        raise SystemExit(f'{module_argv[0]} failed ({res.returncode}):\n{res.stderr[-3000:]}')
    return time.perf_counter() - t0, res.stdout


def median_s(fn, runs, warmup):
    times = []
    for n in range(warmup + runs):
        t0 = time.perf_counter()
        fn()
        if n >= warmup:
            times.append(time.perf_counter() - t0)
    return statistics.median(times), times


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--recordings', type=int, default=64)
    ap.add_argument('--xvectors', type=int, default=1000)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--baseline-repo', default=None, help='a built checkout of the commit to compare with (its per-point route)')
    ap.add_argument('--timeout', type=float, default=600.0, help='seconds a child process may take')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bench_tune.jsonl'))
    opts = ap.parse_args(argv)
    import tune_util
    from vbx_amd import score, tune
    tmp = tempfile.mkdtemp(prefix='bench_tune_')
    p = tune_util.make_dev_set(tmp, opts.recordings, opts.xvectors)
    data = tune_util.data_argv(p)
    grid_argv = [a for k, vs in GRID.items() for a in ['--' + k] + [str(v) for v in vs]]
    points = tune.grid_points(**GRID)
    base = os.path.abspath(opts.baseline_repo) if opts.baseline_repo else REPO

    def tune_route(n):
        s, out = child(REPO, ['vbx_amd.tune'] + data + grid_argv + ['--out-json', f'{tmp}/tune{n}.json'], opts.timeout)
        return s, dict(table=out, doc=json.load(open(f'{tmp}/tune{n}.json')))

    def per_point_route(n):
        total, ders = 0.0, []
        for g, (Fa, Fb, loopP) in enumerate(points):
            s, out = child(base, ['vbx_amd.vbhmm', '--init', 'AHC+VB', '--out-rttm-dir', f'{tmp}/pp{n}_{g}'] + data
                           + ['--Fa', str(Fa), '--Fb', str(Fb), '--loopP', str(loopP)], opts.timeout)
            total += s
            ders.append(out.strip().splitlines()[-1].split()[3])      # the *** OVERALL *** row: DER
        return total, dict(ders=ders)

    routes = {'tune': tune_route, 'per_point': per_point_route}
    times, last = {r: [] for r in routes}, {}
    for n in range(opts.warmup + opts.runs):                          # interleaved: drift of the machine hits both routes alike
        for r, fn in routes.items():
            s, last[r] = fn(n)
            print(f'run {n} {r}: {s:.3f} s', file=sys.stderr, flush=True)
            if n >= opts.warmup:
                times[r].append(s)
    doc = last['tune']['doc']
    tune_ders = [f"{pt['pooled']['der']:.2f}" for pt in doc['points']]
    line = dict(tool='bench_tune', recordings=opts.recordings, xvectors_per_recording=opts.xvectors, grid=GRID, points=len(points),
                collar=0.25, runs=opts.runs, warmup=opts.warmup, baseline_repo=bool(opts.baseline_repo),
                table_equal_to_two_decimals=tune_ders == last['per_point']['ders'], best=doc['best'])
    for r, t in times.items():
        line[f'{r}_s'] = statistics.median(t)
        line[f'{r}_runs_s'] = [round(v, 3) for v in t]
        line[f'{r}_spread_s'] = max(t) - min(t)
    line['ratio_per_point_over_tune'] = line['per_point_s'] / line['tune_s']
    line['within_baseline_spread'] = line['tune_s'] <= line['per_point_s'] + line['per_point_spread_s']
    line['tune_stages_s'] = {k: round(v, 4) for k, v in doc['timing'].items() if isinstance(v, float)}

    # ---- the scoring call alone, in this process: once per recording against once per pair --------------------------------
    from vbx_amd import _capi
    from vbx_amd.kaldi_formats import read_xvector_timing_dict
    args = tune.build_parser().parse_args(data + grid_argv)
    result = tune.tune(args, log=lambda *a: None)
    device = _capi.default_context().device
    segs = read_xvector_timing_dict(p['seg'])
    ref = tune.read_reference(p['ref'], result['names'])
    items = [(ref[n], *segs[n][1].T, [result['labels'][g][k] for g in range(len(points))]) for k, n in enumerate(result['names'])]
    pairs = [(it[0], score.labels_turns(it[1], it[2], lab)) for it in items for lab in it[3]]
    keep = {}
    new_s, new_runs = median_s(lambda: keep.update(new=score.score_labels(items, 0.25, False, device)), opts.runs, opts.warmup)
    old_s, old_runs = median_s(lambda: keep.update(old=score.score_turns(pairs, 0.25, False, device)), opts.runs, opts.warmup)
    flat = [r for per_item in keep['new'] for r in per_item]
    split = {}
    score.score_labels(items, 0.25, False, device, timing=split)
    line.update(score_pairs=len(pairs), score_labels_s=new_s, score_labels_runs_s=[round(v, 4) for v in new_runs],
                score_turns_s=old_s, score_turns_runs_s=[round(v, 4) for v in old_runs], score_turns_spread_s=max(old_runs) - min(old_runs),
                score_factor_turns_over_labels=old_s / new_s, score_within_spread=new_s <= old_s + (max(old_runs) - min(old_runs)),
                score_labels_split_s={k: round(v, 4) for k, v in split.items()},
                score_same_bytes=all(a[k] == b[k] for a, b in zip(flat, keep['old']) for k in ('miss', 'fa', 'confusion', 'ref_time')),
                device=_capi.default_context().device_info()['name'])
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, 'a') as f:
        f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
