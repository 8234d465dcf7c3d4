#!/usr/bin/env python
"""Device time of the x-vector network (vbx_resnet.hpp) on one batch of windows, per stage, against the same folded network
in f32 through PyTorch on the same GPU (F.conv2d: MIOpen).  Synthetic checkpoint (vbx_amd.xvector.synthetic_state_dict),
random N(0, 1) windows.

    python tools/bench_xvec.py [--batch 128] [--frames 144] [--reps 10] [--warmup 3] [--no-torch] [--gemm exact|split|both]

--gemm both measures the two modes of the network in one process on the same inputs and prints both tables.

    python tools/bench_xvec.py --tails 400 [--ways grouped|ragged|both] [--gemm ...] [--batch 128] [--frames 144]

times the windows of one synthetic file that are NOT full ones -- --tails windows, their lengths drawn uniformly from
10 .. frames - 1 -- both ways predict can run them: grouped by exact length, one run of the network per distinct length
(ResNet101.embed), and as ragged batches of at most batch x frames frames in all (ResNet101.embed_ragged).  Device time
is the sum of the runs' HIP-event times; wall time includes every run's launches and its synchronize.  --ways grouped
needs nothing but ResNet101.embed.

Prints a table and one JSON line.  FLOPs are counted from the architecture (xvector.flops, 2 per multiply-add); TF/s is
that count over the device time of the stage (once per multiply-add in the split mode too, not once per f16 matrix
instruction); the f32 matrix peak is 155 TF (MI355X_MICROARCH.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch                                     # first: libvbx_hip.so then binds to PyTorch's HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vbx_amd import xvector                      # noqa: E402

PEAK_TF = 155.0
HOUR_WINDOWS = 15000                             # one hour of speech at the 24-frame jump


def measure(net, xt, a, gemm):
    """One mode's table; -> (its result dict, the embeddings of the last run)."""
    B, T = a.batch, a.frames
    for _ in range(a.warmup):
        net.embed(xt)
    stages, wall = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        y = net.embed(xt)                                     # (ends in a device synchronize)
        wall.append(time.perf_counter() - t0)
        stages.append(net.times())
    assert net.gemm_in_effect() == gemm
    names = list(stages[0])
    med = {k: float(np.median([s[k] for s in stages])) for k in names}
    totals = [sum(s.values()) for s in stages]
    total = float(np.median(totals))
    fl = xvector.flops(T)
    fl['pool_embed'] = 2 * xvector.POOL_DIM * net.embed_dim
    print(f'ResNet101 ({gemm}), {B} windows of {T} frames, median of {a.reps} runs (device ms from HIP events)')
    print(f'{"stage":<12}{"ms":>10}{"GFLOP":>10}{"TF/s":>9}{"% peak":>9}')
    for k in names:
        g = fl[k] * B / 1e9
        tf = g / med[k] if med[k] > 0 else float('nan')
        print(f'{k:<12}{med[k]:>10.3f}{g:>10.1f}{tf:>9.1f}{100 * tf / PEAK_TF:>8.1f}%')
    gt = sum(fl.values()) * B / 1e9
    print(f'{"total":<12}{total:>10.3f}{gt:>10.1f}{gt / total:>9.1f}{100 * gt / total / PEAK_TF:>8.1f}%')
    print(f'total over the {a.reps} runs: min {min(totals):.3f}, max {max(totals):.3f} ms')
    print(f'host wall per batch (copy in, run, copy out): {1e3 * float(np.median(wall)):.3f} ms; '
          f'{HOUR_WINDOWS} windows (one hour): {total * HOUR_WINDOWS / B / 1e3:.3f} s of device time')
    return {'gemm': gemm, 'batch': B, 'frames': T, 'device_ms': total, 'device_ms_min': float(min(totals)),
            'device_ms_max': float(max(totals)), 'stages_ms': med, 'tflops': gt / total, 'gflop': gt,
            'hour_s': total * HOUR_WINDOWS / B / 1e3, 'wall_ms': 1e3 * float(np.median(wall))}, y


def measure_tails(net, a, gemm, dev):
    """The tails of one synthetic file both ways; -> its result dict."""
    rng = np.random.default_rng(a.seed)
    lengths = rng.integers(10, a.frames, a.tails)
    xs = [rng.standard_normal((64, int(T))).astype(np.float32) for T in lengths]
    ways, out = {}, {}
    if a.ways in ('grouped', 'both'):
        groups = {}
        for i, T in enumerate(lengths):
            groups.setdefault(int(T), []).append(i)
        batches = [(idx, torch.from_numpy(np.stack([xs[i] for i in idx])).to(dev)) for idx in groups.values()]
        ways['grouped'] = (batches, lambda xt: net.embed(xt))
    if a.ways in ('ragged', 'both'):
        batches, cur, frames = [], [], 0
        for i, T in enumerate(lengths):                       # (predict.ragged_batches)
            if cur and frames + T > a.batch * a.frames:
                batches.append(cur)
                cur, frames = [], 0
            cur.append(i)
            frames += int(T)
        batches.append(cur)
        batches = [(idx, (torch.from_numpy(np.concatenate([xs[i].reshape(-1) for i in idx])).to(dev), [int(lengths[i]) for i in idx]))
                   for idx in batches]
        ways['ragged'] = (batches, lambda xl: net.embed_ragged(*xl))
    res = {'gemm': gemm, 'tails': int(a.tails), 'frames_total': int(lengths.sum()), 'distinct_lengths': len(set(lengths.tolist())),
           'cap_frames': a.batch * a.frames}
    print(f'ResNet101 ({gemm}), {a.tails} tail windows of 10 .. {a.frames - 1} frames ({res["frames_total"]} frames, '
          f'{res["distinct_lengths"]} distinct lengths), median of {a.reps} runs after {a.warmup}')
    print(f'{"way":<10}{"runs":>6}{"device ms":>12}{"min":>10}{"max":>10}{"wall ms":>10}')
    for way, (batches, run) in ways.items():
        dev_ms, wall = [], []
        emb = np.empty((a.tails, net.embed_dim), dtype=np.float32)
        for rep_ in range(a.warmup + a.reps):
            t0, ms = time.perf_counter(), 0.0
            for idx, arg in batches:
                y = run(arg)
                ms += sum(net.times().values())
                if rep_ == 0:
                    emb[idx] = y.cpu().numpy()
            if rep_ >= a.warmup:
                dev_ms.append(ms)
                wall.append(1e3 * (time.perf_counter() - t0))
        assert net.gemm_in_effect() == gemm
        out[way] = emb
        res[way] = {'runs': len(batches), 'device_ms': float(np.median(dev_ms)), 'device_ms_min': float(min(dev_ms)),
                    'device_ms_max': float(max(dev_ms)), 'wall_ms': float(np.median(wall))}
        r = res[way]
        print(f'{way:<10}{r["runs"]:>6}{r["device_ms"]:>12.3f}{r["device_ms_min"]:>10.3f}{r["device_ms_max"]:>10.3f}{r["wall_ms"]:>10.3f}')
    if len(out) == 2:
        res['same_bits'] = bool(np.array_equal(out['grouped'].view(np.uint32), out['ragged'].view(np.uint32)))
        res['ragged_over_grouped_device'] = res['ragged']['device_ms'] / res['grouped']['device_ms']
        res['ragged_over_grouped_wall'] = res['ragged']['wall_ms'] / res['grouped']['wall_ms']
        print(f'ragged / grouped: device time {res["ragged_over_grouped_device"]:.3f}, wall time {res["ragged_over_grouped_wall"]:.3f}; '
              f'same bits: {res["same_bits"]}')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--frames', type=int, default=144)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--gemm', default='exact', choices=['exact', 'split', 'both'])
    ap.add_argument('--tails', type=int, default=0, help='time this many tail windows of one synthetic file instead')
    ap.add_argument('--ways', default='both', choices=['grouped', 'ragged', 'both'])
    a = ap.parse_args()
    B, T = a.batch, a.frames
    sd = xvector.synthetic_state_dict(a.seed)
    if a.tails > 0:
        results = []
        for gemm in ['exact', 'split'] if a.gemm == 'both' else [a.gemm]:
            net = xvector.ResNet101(sd, a.device, gemm=gemm)
            results.append(measure_tails(net, a, gemm, torch.device('cuda', a.device)))
            del net
        print(json.dumps({'tails_bench': results}))
        return
    x = np.random.default_rng(a.seed).standard_normal((B, 64, T)).astype(np.float32)
    dev = torch.device('cuda', a.device)
    xt = torch.from_numpy(x).to(dev)
    modes = ['exact', 'split'] if a.gemm == 'both' else [a.gemm]
    results, ys = [], []
    for gemm in modes:
        net = xvector.ResNet101(sd, a.device, gemm=gemm)
        r, y = measure(net, xt, a, gemm)
        results.append(r)
        ys.append(y)
        del net
    if len(results) == 2:
        ex, sp = results
        diff = float((ys[1] - ys[0]).abs().max() / ys[0].abs().max())
        print(f'split / exact device time {sp["device_ms"] / ex["device_ms"]:.3f} ({ex["device_ms"]:.3f} -> {sp["device_ms"]:.3f} ms; '
              f'the exact mode\'s own runs span {ex["device_ms_min"]:.3f} .. {ex["device_ms_max"]:.3f} ms); '
              f'max |split - exact| / max|e| = {diff:.2e}')
    result = dict(results[0])
    if len(results) == 2:
        result['split'] = results[1]
        result['max_rel_diff_split_vs_exact'] = diff
    y, total, gt, embed_dim = ys[0], results[0]['device_ms'], results[0]['gflop'], int(ys[0].shape[1])
    if not a.no_torch:
        tens = xvector.folded_tensors(xvector.fold(sd), embed_dim, device=dev, dtype=torch.float32)
        for _ in range(a.warmup):
            ref = xvector.run_folded(tens, xt)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        tms = []
        for _ in range(a.reps):
            ev[0].record()
            ref = xvector.run_folded(tens, xt)
            ev[1].record()
            torch.cuda.synchronize(dev)
            tms.append(ev[0].elapsed_time(ev[1]))
        tm = float(np.median(tms))
        diff = float((y - ref).abs().max() / ref.abs().max())
        print(f'PyTorch f32 (F.conv2d, same folded network): {tm:.3f} ms ({gt / tm:.1f} TF/s); '
              f'HIP ({modes[0]}) / PyTorch time {total / tm:.2f}; max |HIP - PyTorch| / max|e| = {diff:.2e}')
        result.update(torch_ms=tm, torch_tflops=gt / tm, max_rel_diff_vs_torch=diff)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
