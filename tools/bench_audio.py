#!/usr/bin/env python
"""Timing of the conversion to mono int16 (vbx_amd/audio.py, vbx_resample.hpp) on generated audio: the device path (one
vbx_resample_pcm call) split into upload and kernel, next to the numpy path of audio.py and to scipy.signal.resample_poly on
the same host.  Not the headline bench.

Two inputs of ``--seconds`` (default 3600: one hour) of seeded noise: 48 kHz stereo s16 (691 MB an hour) and 44.1 kHz mono
s24 (476 MB an hour), both to 16 kHz.  Medians of ``--reps`` after a warm-up:

  upload       device milliseconds (HIP events) of the copies in: the file bytes and the three small tables
  kernels      device milliseconds of the one kernel
  call         host clock round to_mono16(device=N): the call and the copy out (it ends in a stream synchronise)

and, on the first ``--host-seconds`` (default 120) of the same input, once each:

  numpy        host clock round to_mono16(device=None)
  scipy        host clock round decode, downmix and resample_poly with the same filter in f64 (where scipy imports)

both also scaled to the whole input (``*_scaled_ms``: the slice's time times seconds / host-seconds; both are linear in the
length).  The device's samples are compared with numpy's on the slice, up to the filter's reach before the slice's end.
One JSON line per input, appended to ``--out`` (default profiles/bench_audio.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def generated(seconds, sr, fmt, channels, seed=0):
    """Raw interleaved frames (uint8) of Gaussian noise at about a tenth of full scale."""
    rng = np.random.default_rng(seed)
    n = int(seconds * sr) * channels
    if fmt == 's16':
        return (rng.standard_normal(n, dtype=np.float32) * 3000).astype('<i2').view(np.uint8)
    assert fmt == 's24'
    x = (rng.standard_normal(n, dtype=np.float32) * 800000).astype('<i4')
    return np.ascontiguousarray(x.view(np.uint8).reshape(n, 4)[:, :3]).reshape(-1)


def scipy_path(signal, audio, data, fmt, channels, f):
    X = audio.decode(data, fmt, channels).astype(np.float64) / (256 * channels)
    z = signal.resample_poly(X, f.L, f.M, window=f.hq.astype(np.float64) / audio.ONE / f.L, padtype='constant')
    return np.clip(np.floor(z + 0.5), -32768, 32767).astype(np.int16)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--seconds', type=float, default=3600.0)
    ap.add_argument('--host-seconds', type=float, default=120.0)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bench_audio.jsonl'))
    opts = ap.parse_args()
    from vbx_amd import _capi, audio
    try:
        from scipy import signal
    except ImportError:
        signal = None
    ctx = _capi.default_context(opts.device)                          # no device: an error, not a fall-back
    med = lambda v: float(np.median(v))                               # noqa: E731
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    for sr, fmt, channels in ((48000, 's16', 2), (44100, 's24', 1)):
        f = audio.resample_filter(sr, 16000)
        data = generated(opts.seconds, sr, fmt, channels)
        upload, kernels, call = [], [], []
        for rep in range(opts.reps + 1):                              # (the first is the warm-up: code objects, allocator)
            times = {}
            t0 = time.perf_counter()
            dev = audio.to_mono16([data], fmt, channels, sr, 16000, device=opts.device, times=times)[0]
            call.append(1e3 * (time.perf_counter() - t0))
            upload.append(times['upload'])
            kernels.append(times['kernels'])
        upload, kernels, call = upload[1:], kernels[1:], call[1:]
        host_seconds = min(opts.host_seconds, opts.seconds)
        part = data[:int(host_seconds * sr) * channels * audio.FORMATS[fmt][1]]
        t0 = time.perf_counter()
        ref = audio.to_mono16([part], fmt, channels, sr, 16000)[0]
        numpy_ms = 1e3 * (time.perf_counter() - t0)
        sure = len(ref) - (f.P // f.M + 2) if len(part) < len(data) else len(ref)      # (past it the slice's end is inside the window)
        scale = opts.seconds / host_seconds
        line = {'input': f'{sr} Hz, {channels} x {fmt}', 'sr_in': sr, 'sr_out': 16000, 'format': fmt, 'channels': channels, 'seconds': opts.seconds,
                'frames': int(data.size // (channels * audio.FORMATS[fmt][1])), 'upload_bytes': int(data.nbytes), 'samples_out': int(dev.size),
                'L': f.L, 'M': f.M, 'taps': f.taps, 'tile': _capi.RESAMPLE_TILE,
                'same_samples_as_numpy': bool(np.array_equal(dev[:sure], ref[:sure])), 'compared': int(sure),
                'device': ctx.device_info()['name'], 'reps': opts.reps,
                'upload_ms': med(upload), 'upload_min_max_ms': [float(min(upload)), float(max(upload))],
                'upload_gb_per_s': data.nbytes / med(upload) / 1e6,
                'kernels_ms': med(kernels), 'kernels_min_max_ms': [float(min(kernels)), float(max(kernels))],
                'call_ms': med(call), 'call_min_max_ms': [float(min(call)), float(max(call))],
                'host_seconds': host_seconds, 'numpy_ms': numpy_ms, 'numpy_scaled_ms': numpy_ms * scale}
        if signal is not None:
            t0 = time.perf_counter()
            z = scipy_path(signal, audio, part, fmt, channels, f)
            line['scipy_ms'] = 1e3 * (time.perf_counter() - t0)
            line['scipy_scaled_ms'] = line['scipy_ms'] * scale
            line['scipy_samples_that_differ'] = int(np.count_nonzero(z[:sure] != ref[:sure]))
        text = json.dumps(line)
        print(text, flush=True)
        with open(opts.out, 'a') as fh:
            fh.write(text + '\n')
        del data, dev


if __name__ == '__main__':
    main()
