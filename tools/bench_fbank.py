#!/usr/bin/env python
"""Device time of the filterbank front end (vbx_fbank.hpp) per hour of 16 kHz audio.

A seeded synthetic hour (85 % of it in VAD segments of 0.5 - 8 s) goes through FrontEnd.run once to warm up, then
--reps times; HIP events split each run into upload (signal + tables), frame kernel and CMN, and the gather of every full
window of the plan into [B, 64, 144].  The host dither of the same hour is timed too.  One JSON line on stdout.
usage: tools/bench_fbank.py [--hours 1] [--reps 5] [--device 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch                 # before libvbx_hip.so: one HIP runtime for both (vbx_amd.fbank.FrontEnd)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vbx_amd import fbank    # noqa: E402


def synthetic(hours, sr, seed=7):
    rng = np.random.default_rng(seed)
    n = int(hours * 3600 * sr)
    x = np.clip(np.round(rng.standard_normal(n) * 2000), -32768, 32767).astype(np.int64)
    labs, t = [], 0.0
    while t < n / sr:
        d = rng.uniform(0.5, 8.0)
        labs.append((t, min(t + d, n / sr)))
        t += d / 0.85                                   # 85 % speech
    return x, (np.array(labs) * sr).astype(int)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hours', type=float, default=1.0)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--device', type=int, default=0)
    a = ap.parse_args()
    sr = 16000
    x, labs = synthetic(a.hours, sr)
    dither_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        sig = fbank.dither(x)
        dither_s.append(time.perf_counter() - t0)
    dither_ms = float(np.median(dither_s)) * 1e3
    t0 = time.perf_counter()
    x16 = fbank.raw_samples(x)                      # (predict reads the WAV file as int16 and skips this)
    narrow_ms = (time.perf_counter() - t0) * 1e3
    segs = fbank.segments(labs, len(x), sr)
    fe = fbank.FrontEnd(sr, a.device)
    plan = fbank.window_plan('b', segs, sr)
    med = {}
    # the same input through both paths: the dithered f64 signal up (host), the int16 samples up and dithered there (device)
    for path, run in (('host', lambda: fe.run([(sig, segs)])), ('device', lambda: fe.run_raw([(x16, segs)]))):
        rows = run()[0]
        starts = [rows[w.seg] + w.start for w in plan if w.end - w.start == 144]
        fe.windows(starts, 144)
        out = torch.empty((len(starts), 64, 144), dtype=torch.float32, device=torch.device('cuda', a.device))
        torch.cuda.synchronize(a.device)
        recs = []
        for _ in range(a.reps):
            w0 = time.perf_counter()
            run()
            fe.dev.windows(np.array(starts, dtype=np.int64), 144, dst_ptr=out.data_ptr())
            wall = time.perf_counter() - w0
            recs.append(dict(fe.times(), dither=fe.dither_time(), wall=wall * 1e3))
        med[path] = {k: float(np.median([r[k] for r in recs])) for k in recs[0]}
        if path == 'device':
            n = min(len(x), 1 << 20)                              # the device signal has the host dither's bits
            same = bool(np.array_equal(fe.signal(0, n), sig[:n]) and np.array_equal(fe.signal(len(x) - n, n), sig[-n:]))
    scale = 1.0 / a.hours
    total = lambda m: m['upload'] + m['dither'] + m['frame'] + m['cmn'] + m['gather']   # noqa: E731
    row = lambda m, host_ms: dict(host_dither_ms=round(host_ms * scale, 1), upload_ms=round(m['upload'] * scale, 3),   # noqa: E731
                                  dither_kernel_ms=round(m['dither'] * scale, 3), device_total_ms=round(total(m) * scale, 3),
                                  host_plus_device_ms=round((host_ms + total(m)) * scale, 1))
    res = dict(tool='bench_fbank', hours=a.hours, frames=int(fe.rows), segments=len(segs), windows=len(starts),
               ms_per_hour={k: round(v * scale, 3) for k, v in med['host'].items() if k != 'dither'},
               device_ms_per_hour=round(total(med['host']) * scale, 3),
               host_dither_ms_per_hour=round(dither_ms * scale, 1),
               dither_host=row(med['host'], dither_ms), dither_device=row(med['device'], 0.0),
               device_path_ms_per_hour={k: round(v * scale, 3) for k, v in med['device'].items()},
               int16_check_ms_per_hour=round(narrow_ms * scale, 1), device_signal_equals_host=same,
               frame_gflops_f64=round(fe.rows * 2 * 2 * 272 * 400 / (med['host']['frame'] * 1e6), 1), reps=a.reps)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
