#!/usr/bin/env python
"""``python -m vbx_amd.vbhmm``, files in -> RTTM files out, with ``--init random_N`` and with ``--init AHC+VB``: wall time of
fresh processes and the peak of the device memory in use.

    python tools/bench_random_init.py --recordings 4 --xvectors 10000 --init random_8 --random-restarts 5
    python tools/bench_random_init.py --recordings 1 --xvectors 100000 --init AHC+VB --runs 0 --peak-memory

The archive is the synthetic one of tools/bench_driver.py (the golden recording resampled in speaker turns).  Every run is a
child process of its own (interpreter start, library load and first launches included); one warm-up run, then ``--runs``
measured ones; the line holds their median, every wall time and the stage split the child reports with ``--timing``.
``--peak-memory`` adds one more child that runs the same driver call while a thread asks the runtime for the free device
memory every few milliseconds: the peak is the largest amount in use above what was in use before the call (a figure of the
whole device: other processes on it would show).  ``--tree DIR`` runs the driver of another checkout of this repository (built
there) on the same archive, e.g. the commit before a change.  One JSON line per call; no DER is computed: the archive has no
reference worth the name.
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

SAMPLER = r'''
import ctypes as C, json, sys, threading, time
sys.path.insert(0, sys.argv[1])
from vbx_amd import _capi, vbhmm
argv = json.loads(sys.argv[2])
ctx = _capi.default_context(0)
lib = ctx._lib
lib.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
def used():
    free, total = C.c_size_t(), C.c_size_t()
    assert lib.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value - free.value
before, peak, stop = used(), [0], threading.Event()
def watch():
    while not stop.is_set():
        peak[0] = max(peak[0], used())
        time.sleep(0.002)
th = threading.Thread(target=watch, daemon=True)
th.start()
error = None
try:
    vbhmm.diarize(vbhmm.build_parser().parse_args(argv), log=lambda *_: None)
except Exception as exc:                                      # (an allocation the device cannot make is a result, not a crash)
    error = f'{type(exc).__name__}: {exc}'[:400]
stop.set()
th.join()
print(json.dumps(dict(before_bytes=before, peak_bytes=max(peak[0], before), peak_above_before_bytes=max(peak[0] - before, 0), error=error)))
'''


def driver_argv(paths, out, a):
    argv = ['--init', a.init, '--out-rttm-dir', out, '--xvec-ark-file', paths['ark'], '--segments-file', paths['seg'],
            '--xvec-transform', paths['transform'], '--plda-file', paths['plda'], '--threshold', '-0.015', '--lda-dim', '128',
            '--Fa', '0.3', '--Fb', '17', '--loopP', '0.99', '--precision', a.precision]
    if a.init.startswith('random_'):
        argv += ['--random-restarts', str(a.random_restarts), '--seed', str(a.seed)]
    return argv


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--recordings', type=int, default=4)
    ap.add_argument('--xvectors', type=int, default=10000)
    ap.add_argument('--init', default='random_8')
    ap.add_argument('--random-restarts', type=int, default=1)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--precision', default='fp64')
    ap.add_argument('--runs', type=int, default=5, help='measured runs after the warm-up (0: no timing)')
    ap.add_argument('--peak-memory', action='store_true')
    ap.add_argument('--tree', default=REPO, help='checkout whose driver runs (default: this one)')
    ap.add_argument('--timeout', type=float, default=600.0, help='seconds a child may take')
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    env = dict(os.environ, PYTHONPATH=tree)
    sys.path.insert(0, REPO)
    from tools.bench_driver import make_archive
    line = {'metric': 'python -m vbx_amd.vbhmm, files in -> RTTM out, fresh process', 'unit': 's',
            'config': {'recordings': a.recordings, 'xvectors': a.xvectors, 'init': a.init, 'precision': a.precision,
                       'random_restarts': a.random_restarts if a.init.startswith('random_') else None, 'tree': os.path.relpath(tree, REPO),
                       'hyper': 'lda 128, Fa 0.3, Fb 17, loopP 0.99'},
            'der': None, 'note': 'no DER: the archive is synthetic and has no reference'}
    with tempfile.TemporaryDirectory() as tmp:
        paths = make_archive(tmp, a.recordings, a.xvectors)
        walls, stages = [], []
        for run in range(a.runs + 1 if a.runs > 0 else 0):
            argv = driver_argv(paths, os.path.join(tmp, f'out{run}'), a) + ['--timing']
            t0 = time.perf_counter()
            res = subprocess.run([sys.executable, '-m', 'vbx_amd.vbhmm'] + argv, env=env, cwd=tree, capture_output=True, text=True,
                                 timeout=a.timeout)
            wall = time.perf_counter() - t0
            if res.returncode != 0:
                line['error'] = res.stderr[-600:]
                break
            if run > 0:                                           # (run 0 warms the file cache and the code-object cache)
                walls.append(wall)
                stages.append(json.loads(res.stdout.strip().splitlines()[-1]))
            else:
                line['rttm_files'] = len(os.listdir(os.path.join(tmp, 'out0')))
        if walls:
            line.update(value=statistics.median(walls), seconds=[round(w, 4) for w in walls],
                        xvectors_per_s=a.recordings * a.xvectors / statistics.median(walls),
                        stages_s={k: round(statistics.median(s[k] for s in stages), 4) for k in ('read', 'project', 'ahc', 'vb', 'rttm', 'total')})
        if a.peak_memory:
            res = subprocess.run([sys.executable, '-c', SAMPLER, tree, json.dumps(driver_argv(paths, os.path.join(tmp, 'peak'), a))],
                                 env=env, cwd=tree, capture_output=True, text=True, timeout=a.timeout)
            if res.returncode == 0:
                line['device_memory'] = json.loads(res.stdout.strip().splitlines()[-1])
            else:
                line['device_memory'] = {'error': res.stderr[-600:]}
    print(json.dumps(line))


if __name__ == '__main__':
    main()
