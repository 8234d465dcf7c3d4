"""Inputs for the tests of ``vbx_amd.diarize``: generated "recordings", the models of the driver's golden archive and a
synthetic x-vector network, all written as the files the command lines read.  numpy only, deterministic.

A recording is int16 audio in which two or three generated voices take turns every 1.5 - 4 s.  A voice is a stack of
harmonics of its own fundamental, weighted by its own formant bands, with a slow vibrato, a fade at either end of a turn
and a little noise; between turns lies a short near-silence.  The ``.lab`` text marks every turn as a VAD segment.
"""
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden', 'driver_split3.npz')
EMBED_DIM = 256
NET_SEED = 11

# (fundamental in Hz, formant bands as (centre, width) in Hz)
VOICES = [
    (105.0, [(650.0, 130.0), (1150.0, 160.0), (2500.0, 260.0)]),
    (215.0, [(330.0, 100.0), (2150.0, 220.0), (3000.0, 300.0)]),
    (155.0, [(850.0, 150.0), (1550.0, 200.0), (3400.0, 320.0)]),
]


def voice(v, n, sr, rng):
    """n samples (float64, peak about 6000) of voice v."""
    f0, formants = VOICES[v]
    t = np.arange(n) / sr
    phase = 2 * np.pi * f0 * t + 0.6 * np.sin(2 * np.pi * 5.0 * t + rng.uniform(0, 2 * np.pi))       # 5 Hz vibrato
    x = np.zeros(n)
    k = 1
    while k * f0 < 0.45 * sr:
        f = k * f0
        amp = 0.03 + sum(np.exp(-0.5 * ((f - c) / w) ** 2) for c, w in formants)
        x += amp * np.sin(k * phase + rng.uniform(0, 2 * np.pi))
        k += 1
    x *= 6000.0 / np.abs(x).max()
    fade = min(int(0.02 * sr), n // 2)
    ramp = np.linspace(0.0, 1.0, fade)
    x[:fade] *= ramp
    x[n - fade:] *= ramp[::-1]
    return x + 20.0 * rng.standard_normal(n)


def burst(n, sr, rng):
    """n samples of loud noise gated on and off six times a second: nothing like the voices."""
    t = np.arange(n) / sr
    return 20000.0 * rng.uniform(-1, 1, n) * (np.sin(2 * np.pi * 6.0 * t) > 0)


def synth_recording(seed, sr, seconds, n_voices=2, short_vad=False, tail_only=False, bursts=0.0):
    """-> (int16 samples, lab text, [(start s, end s, voice)]).  The turns fill about ``seconds``.
    short_vad: one extra VAD segment of 0.005 s (predict skips what is not longer than 0.01 s);
    tail_only: one extra turn of 0.8 s -- fewer frames than a window, so that it yields a tail window alone;
    bursts: so many seconds of ``burst`` marked as one VAD segment at the end (what ``write_checkpoint(overflow=True)``'s
    network answers with NaN embeddings)."""
    rng = np.random.default_rng(seed)
    pieces, turns, labs, pos, v = [], [], [], 0, int(rng.integers(n_voices))
    gap = lambda: int(rng.uniform(0.15, 0.4) * sr)

    def add_silence(n):
        nonlocal pos
        pieces.append(3.0 * rng.standard_normal(n))
        pos += n

    def add_turn(v, n):
        nonlocal pos
        pieces.append(voice(v, n, sr, rng))
        turns.append((pos / sr, (pos + n) / sr, v))
        labs.append((pos / sr, (pos + n) / sr))
        pos += n

    add_silence(gap())
    while pos < seconds * sr:
        add_turn(v, int(rng.uniform(1.5, 4.0) * sr))
        add_silence(gap())
        v = (v + 1 + int(rng.integers(n_voices - 1))) % n_voices           # always another voice
    if tail_only:
        add_turn(v, int(0.8 * sr))
        add_silence(gap())
    if short_vad:
        labs.append((pos / sr - 0.1, pos / sr - 0.095))
    if bursts:
        n = int(bursts * sr)
        pieces.append(burst(n, sr, rng))
        labs.append((pos / sr, (pos + n) / sr))
        pos += n
        add_silence(gap())
    x = np.clip(np.rint(np.concatenate(pieces)), -32768, 32767).astype(np.int16)
    lab = ''.join(f'{a:.6f} {b:.6f} sp\n' for a, b in labs)
    return x, lab, turns


def write_corpus(tmp, recordings):
    """recordings: {name: (samples, sr, lab text)} -> dict(wav=, lab=, list=) of paths under tmp."""
    from vbx_amd import fbank
    tmp = str(tmp)
    wav, lab = os.path.join(tmp, 'wav'), os.path.join(tmp, 'lab')
    os.makedirs(wav, exist_ok=True)
    os.makedirs(lab, exist_ok=True)
    for name, (x, sr, text) in recordings.items():
        fbank.write_wav(os.path.join(wav, name + '.wav'), x, sr)
        with open(os.path.join(lab, name + '.lab'), 'w') as f:
            f.write(text)
    lst = os.path.join(tmp, 'list.txt')
    with open(lst, 'w') as f:
        f.write(''.join(name + '\n' for name in recordings))
    return dict(wav=wav, lab=lab, list=lst)


def write_models(tmp):
    """The transform and the PLDA of the driver's golden archive, as tests/test_driver.py writes them."""
    from vbx_amd import kaldi_formats as kf
    g = np.load(GOLD)
    paths = dict(plda=os.path.join(str(tmp), 'plda'), transform=os.path.join(str(tmp), 'transform.npz'))
    kf.write_plda(paths['plda'], g['plda_mean'], g['plda_trans'], g['plda_psi'])
    np.savez(paths['transform'], mean1=g['mean1'], mean2=g['mean2'], lda=g['lda'])
    return paths


# One output channel of the network's last convolution, and the factor on its BatchNorm weight: with it the channel's
# largest value is G (z - beta), z - beta being what the folded convolution gives before the shortcut is added.  For the
# windows of the generated voices z - beta stays below 8.7 (the network in f32 on the CPU, every window of the recordings of
# the NaN test, tails included), for the windows of a ``burst`` segment it reaches at least 188: G = 3.4e36 leaves the former
# below 3e37 and takes the latter past the largest float32 (3.4e38) to +inf.  An infinite activation makes the pooled
# standard deviation inf - inf = NaN, and with it the whole embedding: the case predict.py:185 skips.  (The front end floors
# the Mel energies at 1, so digital silence gives zeros, not the non-finite features a bare logarithm would.)
OVERFLOW_CHANNEL, OVERFLOW_GAIN = 724, 3.4e36


def write_checkpoint(tmp, seed=NET_SEED, overflow=False):
    import torch
    from vbx_amd import xvector
    path = os.path.join(str(tmp), 'ckpt.pth')
    sd = xvector.synthetic_state_dict(seed, EMBED_DIM)
    if overflow:
        sd['layer4.2.bn3.weight'][OVERFLOW_CHANNEL] *= np.float32(OVERFLOW_GAIN)
    torch.save({'state_dict': {k: torch.from_numpy(v) for k, v in sd.items()}}, path)
    return path


def standard_corpus():
    """The three recordings of the whole-route tests: 16 kHz of about 20 s (with a VAD segment shorter than 0.01 s) and 35 s
    (three voices), 8 kHz of about 15 s (with a turn that yields only a tail window)."""
    a = synth_recording(1, 16000, 20, 2, short_vad=True)
    b = synth_recording(2, 16000, 35, 3)
    c = synth_recording(3, 8000, 15, 2, tail_only=True)
    return {'recA': (a[0], 16000, a[1]), 'recB': (b[0], 16000, b[1]), 'recC': (c[0], 8000, c[1])}


def rttm_dir(path):
    """{file name: bytes} of a directory of RTTM files ({} where it does not exist)."""
    if not os.path.isdir(path):
        return {}
    return {f: open(os.path.join(path, f), 'rb').read() for f in sorted(os.listdir(path))}


def rttm_speakers_and_lines(data: bytes):
    lines = [l.split() for l in data.decode().splitlines() if l.strip()]
    return len({l[7] for l in lines}), len(lines)
