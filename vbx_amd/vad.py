"""Energy voice-activity detection: the ``<name>.lab`` files that ``python -m vbx_amd.predict`` and ``python -m
vbx_amd.diarize`` take through ``--in-lab-dir`` (lines ``start end sp`` in seconds), computed from the wav files alone.

The rule is the one of Kaldi's energy VAD (``compute-vad-energy``) on the 25 ms / 10 ms frames the front end cuts, followed
by a smoothing of the decisions.  For a recording of n int16 samples with L = winlen and H = shift of
``fbank.geometry(sr)``, T = (n - L) // H + 1 frames (0 if n < L), frame t the samples [t H, t H + L) as they are:

    N[t]   = L sum x^2 - (sum x)^2                      exact, int64: L times the energy of the frame without its mean
    e[t]   = log(max(N[t] / L, 1))                      f64 (digital silence gives 0)
    theta  = energy_threshold + mean_scale * sum(e) / T
    raw[t] = n_hot >= n_in * proportion                 n_in: the frames of [t - context, t + context] inside [0, T),
                                                        n_hot: those of them with e > theta
    close  every gap between two runs of raw that is shorter than min_silence frames
    drop   every run that is then shorter than min_speech frames
    pad    what is left by pad frames on both sides, clipped to [0, T); runs that touch or overlap become one

    energy_vad                 the frame runs [a, b) of every recording: in numpy (device=None) or by the kernels of
                               vbx_vad.hpp (device=N), which take a batch of recordings in one call
    segments_seconds, write_lab   a * H / sr, b * H / sr, printed as the reference's example/vad/*.lab are
    python -m vbx_amd.vad      wav files in, .lab files out

The defaults of the decision are believed to be those of the vad.conf of Kaldi's x-vector recipes (Kaldi's log energy is
taken on int16-scaled samples too, so its threshold carries over); those of the smoothing are this module's.  Nobody has
tuned either on a corpus.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import fbank

DEFAULTS = dict(energy_threshold=5.5, mean_scale=0.5, context=2, proportion=0.12, min_silence=30, min_speech=20, pad=0)
BATCH_SAMPLES = 1 << 28          # int16 samples per device call of the command line (0.5 GB: 4.7 hours at 16 kHz)


def _check(p: dict):
    for k in ('energy_threshold', 'mean_scale', 'proportion'):
        if not np.isfinite(p[k]):
            raise ValueError(f'{k}={p[k]} must be finite')
    for k in ('context', 'min_silence', 'min_speech', 'pad'):
        if int(p[k]) != p[k] or not 0 <= p[k] <= 2 ** 30:
            raise ValueError(f'{k}={p[k]} must be a number of frames in [0, 2^30]')


def frame_count(n: int, sr: int) -> int:
    g = fbank.geometry(sr)
    return (n - g['winlen']) // g['shift'] + 1 if n >= g['winlen'] else 0


# ---- the numpy path ---------------------------------------------------------------------------------------------------
def frame_energies(x, sr: int) -> np.ndarray:
    """N[t] of one recording as int64, from the sums over sub-blocks of gcd(L, H) samples (five a frame, two a shift)."""
    g = fbank.geometry(sr)
    L, H = g['winlen'], g['shift']
    G = int(np.gcd(L, H))
    T = frame_count(len(x), sr)
    if T == 0:
        return np.zeros(0, dtype=np.int64)
    nsub = (H // G) * (T - 1) + L // G
    b = np.asarray(x[:nsub * G], dtype=np.int64).reshape(nsub, G)
    cs = np.concatenate([[0], np.cumsum(b.sum(1))])
    cq = np.concatenate([[0], np.cumsum((b * b).sum(1))])
    lo = np.arange(T) * (H // G)
    S, Q = cs[lo + L // G] - cs[lo], cq[lo + L // G] - cq[lo]
    return L * Q - S * S


def runs_of(mask) -> np.ndarray:
    """The maximal runs [a, b) of a boolean sequence, int32 [k][2]."""
    d = np.diff(np.concatenate([[0], np.asarray(mask, dtype=np.int8), [0]]))
    return np.stack([np.flatnonzero(d == 1), np.flatnonzero(d == -1)], axis=1).astype(np.int32)


def _join(runs, gap: int) -> np.ndarray:
    """Neighbours whose gap is shorter than ``gap`` frames become one run."""
    if len(runs) == 0:
        return runs
    cut = runs[1:, 0] - runs[:-1, 1] >= gap
    return np.stack([runs[np.concatenate([[True], cut]), 0], runs[np.concatenate([cut, [True]]), 1]], axis=1)


def smooth(runs, T: int, min_silence: int, min_speech: int, pad: int) -> np.ndarray:
    runs = _join(np.asarray(runs, dtype=np.int32).reshape(-1, 2), min_silence)
    runs = runs[runs[:, 1] - runs[:, 0] >= min_speech]
    runs = np.stack([np.maximum(runs[:, 0] - pad, 0), np.minimum(runs[:, 1] + pad, T)], axis=1)
    return _join(runs, 1).astype(np.int32)


def _host(x, sr: int, p: dict):
    g = fbank.geometry(sr)
    N = frame_energies(x, sr)
    T = len(N)
    e = np.log(np.maximum(N / g['winlen'], 1.0))
    theta = p['energy_threshold'] + (p['mean_scale'] * e.sum() / T if T else 0.0)
    c = int(p['context'])
    hot = np.concatenate([[0], np.cumsum(e > theta)])
    t = np.arange(T)
    w0, w1 = np.maximum(t - c, 0), np.minimum(t + c, T - 1) + 1
    raw = (hot[w1] - hot[w0]).astype(np.float64) >= (w1 - w0).astype(np.float64) * p['proportion']
    runs = smooth(runs_of(raw), T, int(p['min_silence']), int(p['min_speech']), int(p['pad']))
    return runs, dict(N=N, e=e, theta=float(theta), raw=raw.astype(np.uint8))


# ---- the public call --------------------------------------------------------------------------------------------------
def energy_vad(recordings, sr: int, *, device=None, energy_threshold=5.5, mean_scale=0.5, context=2, proportion=0.12,
               min_silence=30, min_speech=20, pad=0, details=False, times=None):
    """The speech of every recording (a list of int16 sample arrays at ``sr``) as frame runs: per recording an int32
    [k][2] array of [a, b).  ``details``: (runs, details) with per recording a dict of N (int64), e (f64), theta and raw
    (uint8).  ``device=None`` computes in numpy, ``device=N`` on GPU N, all recordings in one call of vbx_vad_energy.
    ``times``: a dict that receives the device milliseconds ``upload`` and ``kernels`` of that call."""
    p = dict(energy_threshold=float(energy_threshold), mean_scale=float(mean_scale), context=context, proportion=float(proportion),
             min_silence=min_silence, min_speech=min_speech, pad=pad)
    _check(p)
    g = fbank.geometry(sr)
    raws = [fbank.raw_samples(x) for x in recordings]
    if not raws:
        return ([], []) if details else []
    if device is None:
        got = [_host(x, sr, p) for x in raws]
        runs, det = [r for r, _ in got], [d for _, d in got]
    else:
        from . import _capi
        if _capi._lib is None:
            try:                         # (PyTorch-ROCm's HIP runtime first, as fbank.FrontEnd explains)
                import torch  # noqa: F401
            except ImportError:
                pass
        lens = np.array([len(x) for x in raws], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)])
        rec = np.stack([offs[:-1], lens], axis=1)
        samples = raws[0] if len(raws) == 1 else np.concatenate(raws)        # (one recording goes up from where it lies)
        counts, segs, d, ms = _capi.vad_energy(_capi.default_context(int(device)), samples, rec, g['winlen'], g['shift'],
                                               p['energy_threshold'], p['mean_scale'], p['context'], p['proportion'],
                                               p['min_silence'], p['min_speech'], p['pad'], details=details, times=times is not None)
        ends = np.cumsum(counts)
        runs = [segs[b - c:b].copy() for b, c in zip(ends, counts)]
        if times is not None:
            times.update(upload=float(ms[0]), kernels=float(ms[1]))
        if details:
            fe = np.cumsum([frame_count(n, sr) for n in lens])
            det = [dict(N=d[0][b - t:b].copy(), e=d[1][b - t:b].copy(), theta=float(d[2][r]), raw=d[3][b - t:b].copy())
                   for r, (b, t) in enumerate(zip(fe, np.diff(np.concatenate([[0], fe]))))]
    return (runs, det) if details else runs


def segments_seconds(runs, sr: int) -> list:
    """[(start, end)] in seconds of frame runs [a, b): a H / sr and b H / sr."""
    H = fbank.geometry(sr)['shift']
    return [(int(a) * H / sr, int(b) * H / sr) for a, b in np.asarray(runs).reshape(-1, 2)]


def lab_text(runs, sr: int) -> str:
    return ''.join(f'{start:.3f} {end:.3f} sp\n' for start, end in segments_seconds(runs, sr))


def write_lab(path: str, runs, sr: int):
    """``start end sp`` per run, seconds with three decimals (the reference's example/vad/ES2005a.lab).  A file without a
    line cannot be read back by fbank.read_lab: an empty run list is refused."""
    if len(runs) == 0:
        raise ValueError(f'{path}: no segment to write')
    with open(path, 'w') as f:
        f.write(lab_text(runs, sr))


# ---- command line -----------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog='python -m vbx_amd.vad', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--in-file-list', required=True, type=str, help='input list of files')
    p.add_argument('--in-wav-dir', required=True, type=str, help='input directory with wavs')
    p.add_argument('--out-lab-dir', required=True, type=str, help='output directory for the VAD labels')
    p.add_argument('--out-file-list', type=str, default=None, help='write the names that got a .lab file (the --in-file-list of predict / diarize)')
    p.add_argument('--device', type=int, default=None, metavar='N', help='run on GPU N (default: in numpy on the host)')
    p.add_argument('--resample-to', type=int, default=None, choices=[8000, 16000], metavar='{8000,16000}',
                   help='take wavs of any PCM format, channel count and rate (vbx_amd.audio) and convert them to mono 16-bit at this '
                        'rate first, where the VAD runs (default: only mono 16-bit wavs at 8 or 16 kHz are taken)')
    p.add_argument('--energy-threshold', type=float, default=DEFAULTS['energy_threshold'], help='constant term of the threshold on the log energy')
    p.add_argument('--mean-scale', type=float, default=DEFAULTS['mean_scale'], help="factor of the recording's mean log energy in the threshold")
    p.add_argument('--context', type=int, default=DEFAULTS['context'], help='frames on either side that vote on a frame')
    p.add_argument('--proportion', type=float, default=DEFAULTS['proportion'], help='share of the votes that makes a frame speech')
    p.add_argument('--min-silence', type=int, default=DEFAULTS['min_silence'], help='frames: shorter gaps between speech are closed')
    p.add_argument('--min-speech', type=int, default=DEFAULTS['min_speech'], help='frames: shorter runs of speech are dropped')
    p.add_argument('--pad', type=int, default=DEFAULTS['pad'], help='frames added on both sides of every run of speech')
    return p


def batches(sizes, budget: int = BATCH_SAMPLES) -> list:
    """Consecutive groups of indices whose sizes add up to at most ``budget`` (a larger item is a group of its own)."""
    out, cur, tot = [], [], 0
    for i, n in enumerate(sizes):
        if cur and tot + n > budget:
            out.append(cur)
            cur, tot = [], 0
        cur.append(i)
        tot += n
    return out + ([cur] if cur else [])


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    params = {k: getattr(args, k) for k in DEFAULTS}
    try:
        _check(params)
        names = [str(f) for f in np.atleast_1d(np.loadtxt(args.in_file_list, dtype=object))]
        paths = [os.path.join(args.in_wav_dir, f'{fn}.wav') for fn in names]
        if args.resample_to is None:
            wavs = [fbank.read_wav(path, raw=True) for path in paths]
        else:                            # any PCM wav, converted where the VAD runs; from here on as if the converted file had been read
            from . import audio
            wavs = [(x, args.resample_to) for x in audio.convert_files(paths, args.resample_to, device=args.device)]
    except (ValueError, OSError) as exc:
        ap.error(str(exc))
    os.makedirs(args.out_lab_dir, exist_ok=True)
    runs = [None] * len(names)
    for sr in sorted({sr for _, sr in wavs}):                    # files of one rate run together
        idx = [i for i, (_, r) in enumerate(wavs) if r == sr]
        for group in batches([len(wavs[i][0]) for i in idx]):
            got = energy_vad([wavs[idx[j]][0] for j in group], sr, device=args.device, **params)
            for j, r in zip(group, got):
                runs[idx[j]] = r
    written = []
    for fn, (_, sr), r in zip(names, wavs, runs):
        if len(r) == 0:
            print(f'warning: {fn}: no speech found, no .lab file written', file=sys.stderr)
            continue
        write_lab(os.path.join(args.out_lab_dir, f'{fn}.lab'), r, sr)
        written.append(fn)
    if args.out_file_list:
        with open(args.out_file_list, 'w') as f:
            f.write(''.join(f'{fn}\n' for fn in written))
    return 0


if __name__ == '__main__':
    sys.exit(main())
