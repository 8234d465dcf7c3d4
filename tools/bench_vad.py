#!/usr/bin/env python
"""Timing of the energy VAD (vbx_amd/vad.py, vbx_vad.hpp) on one recording of synthetic audio: the device path (one
vbx_vad_energy call) split into upload and kernels, next to the numpy path of vad.py on the same host.  Not the headline bench.

The recording is ``--seconds`` (default 3600: one hour) of 16 kHz int16 noise whose level switches between about 3000 and
about 10 every 0.3 - 6 s.  Seeded.  Medians of ``--reps`` after a warm-up:

  upload       device milliseconds (HIP events) of the copies in: the samples and the two small tables
  kernels      device milliseconds of the five kernels
  call         host clock round energy_vad(device=N): concatenation and tables, the call, the copies out (it ends in a
               stream synchronise)
  numpy        host clock round energy_vad(device=None)

One JSON line, appended to ``--out`` (default profiles/bench_vad.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def synthetic_recording(seconds, sr, seed=0):
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    level = np.empty(n, dtype=np.float32)
    pos, on = 0, False
    while pos < n:
        m = int(rng.uniform(0.3, 6.0) * sr)
        level[pos:pos + m] = 3000.0 if on else 10.0
        pos, on = pos + m, not on
    x = rng.standard_normal(n, dtype=np.float32) * level
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--seconds', type=float, default=3600.0)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bench_vad.jsonl'))
    opts = ap.parse_args()
    from vbx_amd import _capi, vad
    sr = 16000
    ctx = _capi.default_context(opts.device)                          # no device: an error, not a fall-back
    x = synthetic_recording(opts.seconds, sr)
    upload, kernels, call = [], [], []
    for rep in range(opts.reps + 1):                                  # (the first is the warm-up: code objects, allocator)
        times = {}
        t0 = time.perf_counter()
        dev = vad.energy_vad([x], sr, device=opts.device, times=times)[0]
        call.append(1e3 * (time.perf_counter() - t0))
        upload.append(times['upload'])
        kernels.append(times['kernels'])
    host = []
    for rep in range(max(3, opts.reps // 2)):
        t0 = time.perf_counter()
        ref = vad.energy_vad([x], sr)[0]
        host.append(1e3 * (time.perf_counter() - t0))
    upload, kernels, call = upload[1:], kernels[1:], call[1:]
    med = lambda v: float(np.median(v))                               # noqa: E731
    line = {'seconds': opts.seconds, 'sample_rate': sr, 'samples': int(x.size), 'upload_bytes': int(x.nbytes),
            'frames': vad.frame_count(x.size, sr), 'segments': int(len(dev)), 'same_segments_as_numpy': bool(np.array_equal(dev, ref)),
            'device': ctx.device_info()['name'], 'reps': opts.reps,
            'upload_ms': med(upload), 'upload_min_max_ms': [float(min(upload)), float(max(upload))],
            'upload_gb_per_s': x.nbytes / med(upload) / 1e6,
            'kernels_ms': med(kernels), 'kernels_min_max_ms': [float(min(kernels)), float(max(kernels))],
            'call_ms': med(call), 'call_min_max_ms': [float(min(call)), float(max(call))],
            'numpy_ms': med(host), 'numpy_min_max_ms': [float(min(host)), float(max(host))],
            'numpy_over_call': med(host) / med(call)}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, 'a') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
