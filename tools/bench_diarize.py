#!/usr/bin/env python
"""End-to-end seconds of wav files -> RTTM files: ``python -m vbx_amd.diarize`` (one process, x-vectors kept on the device)
against ``python -m vbx_amd.predict`` followed by ``python -m vbx_amd.vbhmm`` (two processes, an ark file between them),
every run in fresh child processes, which is how users run them.  Prints one JSON line.

    python tools/bench_diarize.py [--files 4] [--minutes 10] [--runs 5] [--warmup 1] [--baseline-repo DIR] [--gemm exact]

Input: generated audio (tests/diarize_util.py: two generated voices taking turns), --files recordings of --minutes at 16 kHz,
the models of tests/golden/driver_split3.npz and the synthetic network of the tests.  --baseline-repo: a built checkout of
another commit (the parent); its two-step route is timed in the same call, interleaved with the others, and the line
carries its median and spread (max - min) -- the margin the one-process median is held against.
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


def child(repo, module_argv, timeout):
    t0 = time.perf_counter()
    res = subprocess.run([sys.executable, '-m'] + module_argv, env=dict(os.environ, PYTHONPATH=repo), cwd=repo, capture_output=True,
                         text=True, timeout=timeout)
    if res.returncode != 0:
        raise SystemExit(f'{module_argv[0]} failed ({res.returncode}):\n{res.stderr[-3000:]}')
    return time.perf_counter() - t0, res.stdout


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--files', type=int, default=4)
    ap.add_argument('--minutes', type=float, default=10.0)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--gemm', default='exact', choices=['exact', 'split'])
    ap.add_argument('--baseline-repo', default=None, help='a built checkout of the commit to compare with (its two-step route)')
    ap.add_argument('--timeout', type=float, default=600.0, help='seconds a child process may take')
    args = ap.parse_args(argv)
    import diarize_util as du
    tmp = tempfile.mkdtemp(prefix='bench_diarize_')
    recs = {}
    for k in range(args.files):
        x, lab, _ = du.synth_recording(100 + k, 16000, 60.0 * args.minutes, 2)
        recs[f'file{k}'] = (x, 16000, lab)
    p = du.write_corpus(tmp, recs)
    p.update(du.write_models(tmp), ckpt=du.write_checkpoint(tmp))
    audio_s = sum(len(x) for x, _, _ in recs.values()) / 16000.0
    del recs
    front = ['--gpus', '0', '--checkpoint', p['ckpt'], '--gemm', args.gemm, '--in-file-list', p['list'], '--in-lab-dir', p['lab'],
             '--in-wav-dir', p['wav']]
    back = ['--init', 'AHC+VB', '--xvec-transform', p['transform'], '--plda-file', p['plda'], '--threshold', '0.0', '--lda-dim', '128',
            '--Fa', '4.0', '--Fb', '1.0', '--loopP', '0.99', '--timing']

    def one_process(n):
        s, out = child(REPO, ['vbx_amd.diarize'] + front + back + ['--out-rttm-dir', f'{tmp}/one{n}'], args.timeout)
        return s, json.loads(out.strip().splitlines()[-1])

    def two_step(repo, n):
        ark, seg = f'{tmp}/x{n}.ark', f'{tmp}/x{n}.seg'
        s1, _ = child(repo, ['vbx_amd.predict'] + front + ['--out-ark-fn', ark, '--out-seg-fn', seg], args.timeout)
        s2, out = child(repo, ['vbx_amd.vbhmm'] + back + ['--out-rttm-dir', f'{tmp}/two{n}', '--xvec-ark-file', ark, '--segments-file', seg],
                        args.timeout)
        os.remove(ark)
        return s1 + s2, dict(predict=s1, vbhmm=s2, vbhmm_stages=json.loads(out.strip().splitlines()[-1]))

    routes = {'one_process': one_process, 'two_step': lambda n: two_step(REPO, n)}
    if args.baseline_repo:
        base = os.path.abspath(args.baseline_repo)
        routes['two_step_baseline'] = lambda n: two_step(base, f'b{n}')
    times, last = {r: [] for r in routes}, {}
    for n in range(args.warmup + args.runs):                      # interleaved: drift of the machine hits every route alike
        for r, fn in routes.items():
            s, detail = fn(n)
            last[r] = detail
            print(f'run {n} {r}: {s:.3f} s', file=sys.stderr, flush=True)
            if n >= args.warmup:
                times[r].append(s)
    same = all(open(f'{tmp}/one0/{f}', 'rb').read() == open(f'{tmp}/two0/{f}', 'rb').read() for f in sorted(os.listdir(f'{tmp}/two0')))
    line = dict(tool='bench_diarize', files=args.files, audio_s=audio_s, gemm=args.gemm, runs=args.runs, warmup=args.warmup,
                xvectors=last['one_process'].get('xvectors'), rttm_identical=same)
    for r, t in times.items():
        line[f'{r}_s'] = statistics.median(t)
        line[f'{r}_runs_s'] = [round(v, 3) for v in t]
        line[f'{r}_spread_s'] = max(t) - min(t)
    line['one_process_stages_s'] = {k: round(v, 4) for k, v in last['one_process'].items() if isinstance(v, float)}
    line['two_step_split_s'] = dict(predict=round(last['two_step']['predict'], 3), vbhmm=round(last['two_step']['vbhmm'], 3),
                                    vbhmm_stages={k: round(v, 4) for k, v in last['two_step']['vbhmm_stages'].items() if isinstance(v, float)})
    if args.baseline_repo:
        line['within_baseline_spread'] = line['one_process_s'] <= line['two_step_baseline_s'] + line['two_step_baseline_spread_s']
    print(json.dumps(line))
    return 0


if __name__ == '__main__':
    sys.exit(main())
