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
    t0 = time.perf_counter()
    sig = fbank.dither(x)
    dither_s = time.perf_counter() - t0
    segs = fbank.segments(labs, len(x), sr)
    fe = fbank.FrontEnd(sr, a.device)
    rows = fe.run([(sig, segs)])[0]
    plan = fbank.window_plan('b', segs, sr)
    starts = [rows[w.seg] + w.start for w in plan if w.end - w.start == 144]
    fe.windows(starts, 144)
    out = torch.empty((len(starts), 64, 144), dtype=torch.float32, device=torch.device('cuda', a.device))
    torch.cuda.synchronize(a.device)
    recs = []
    for _ in range(a.reps):
        w0 = time.perf_counter()
        fe.run([(sig, segs)])
        fe.dev.windows(np.array(starts, dtype=np.int64), 144, dst_ptr=out.data_ptr())
        wall = time.perf_counter() - w0
        recs.append(dict(fe.times(), wall=wall * 1e3))
    med = {k: float(np.median([r[k] for r in recs])) for k in recs[0]}
    scale = 1.0 / a.hours
    res = dict(tool='bench_fbank', hours=a.hours, frames=int(fe.rows), segments=len(segs), windows=len(starts),
               ms_per_hour={k: round(v * scale, 3) for k, v in med.items()},
               device_ms_per_hour=round((med['upload'] + med['frame'] + med['cmn'] + med['gather']) * scale, 3),
               host_dither_ms_per_hour=round(dither_s * 1e3 * scale, 1),
               frame_gflops_f64=round(fe.rows * 2 * 2 * 272 * 400 / (med['frame'] * 1e6), 1), reps=a.reps)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
