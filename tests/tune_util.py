"""A generated development set for ``vbx_amd.tune``: x-vector archives with reference turns.  numpy only, deterministic.

Every recording is the driver's golden archive (tests/golden/driver_split3.npz: 1025 real x-vectors of three recordings)
resampled in blocks of 20 - 80 consecutive x-vectors with a little Gaussian noise, as tools/bench_driver.py does, on the
extractor's time grid (windows of 1.44 s every 0.24 s).  The generator's speaker of an x-vector is the speaker the golden
RTTM gives the source x-vector's window (at its middle; the nearest turn where none covers it); the reference turns are the
merged windows of one speaker, written with millisecond decimals.
"""
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden', 'driver_split3.npz')


def golden_speakers(g):
    """per golden x-vector: 'rec:label' of the golden RTTM turn at (or nearest to) the middle of its window"""
    turns = {}
    for rec in ('recA', 'recB', 'recC'):
        for line in g['rttm_' + rec].tobytes().decode().splitlines():
            f = line.split()
            turns.setdefault(rec, []).append((float(f[3]), float(f[3]) + float(f[4]), f[7]))
    out = []
    for rec, (s, e) in zip(g['recs'].tolist(), g['segments']):
        mid = 0.5 * (s + e)
        best = min(turns[rec], key=lambda t: 0.0 if t[0] <= mid <= t[1] else min(abs(t[0] - mid), abs(t[1] - mid)))
        out.append(f'{rec}:{best[2]}')
    return out


def make_dev_set(tmp, n_rec, n_xvec, seed=0):
    """-> dict(ark=, seg=, plda=, transform=, ref=<directory of reference RTTM files>, names=[...]) under tmp"""
    from vbx_amd import kaldi_formats as kf
    from vbx_amd.vbhmm import merge_adjacent_labels
    g = np.load(GOLD)
    rng = np.random.default_rng(seed)
    base, T0 = g['xvecs'], g['xvecs'].shape[0]
    spk = golden_speakers(g)
    ids = {s: i for i, s in enumerate(sorted(set(spk)))}
    spk = np.array([ids[s] for s in spk])
    tmp = str(tmp)
    paths = dict(ark=os.path.join(tmp, 'dev.ark'), seg=os.path.join(tmp, 'dev.seg'), plda=os.path.join(tmp, 'plda'),
                 transform=os.path.join(tmp, 'transform.npz'), ref=os.path.join(tmp, 'ref'), names=[f'dev{r:03d}' for r in range(n_rec)])
    os.makedirs(paths['ref'], exist_ok=True)
    items, segs = [], []
    for name in paths['names']:
        idx = []
        while len(idx) < n_xvec:
            lo = int(rng.integers(0, T0 - 80))
            idx.extend(range(lo, lo + int(rng.integers(20, 80))))
        idx = np.array(idx[:n_xvec])
        x = base[idx] + 0.02 * np.abs(base).mean() * rng.standard_normal((n_xvec, base.shape[1])).astype(np.float32)
        starts = np.round(0.24 * np.arange(n_xvec), 2)
        ends = np.round(starts + 1.44, 2)
        for k in range(n_xvec):
            key = f'{name}_{k:05d}'
            items.append((key, x[k]))
            segs.append((key, name, starts[k], ends[k]))
        b, e, s = merge_adjacent_labels(starts, ends, spk[idx])
        with open(os.path.join(paths['ref'], name + '.rttm'), 'w') as f:
            f.write(''.join(f'SPEAKER {name} 1 {bb:.3f} {ee - bb:.3f} <NA> <NA> spk{ss} <NA> <NA>\n' for bb, ee, ss in zip(b, e, s)))
    kf.write_vec_flt_ark(paths['ark'], items)
    kf.write_segments(paths['seg'], segs)
    kf.write_plda(paths['plda'], g['plda_mean'], g['plda_trans'], g['plda_psi'])
    np.savez(paths['transform'], mean1=g['mean1'], mean2=g['mean2'], lda=g['lda'])
    return paths


def data_argv(paths, threshold='-0.015'):
    """the arguments of vbx_amd.tune and vbx_amd.vbhmm that name the data and the AHC stage"""
    return ['--xvec-ark-file', paths['ark'], '--segments-file', paths['seg'], '--xvec-transform', paths['transform'], '--plda-file',
            paths['plda'], '--threshold', threshold, '--lda-dim', '128', '--ref-rttm-dir', paths['ref']]
