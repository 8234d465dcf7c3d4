"""Reference, inputs and comparison functions for the filterbank front end's kernels (vbx_fbank.hpp)  --  test helper, not
a test.  tests/test_fbank_ref_host.py checks it on the CPU (against the fixture of the unmodified predict.py, and with
deliberately wrong models of the kernels); tests/test_gpu_fbank_kernels.py runs the device on the very same cases through
the very same comparison functions.

    ref_logmel   features.fbank_htk of one mirror-padded segment (predict.py:173-175), step by step in float64: no folded
                 operator, np.fft.rfft for the transform.  Its pieces (pad, cut, frames_to_logmel) are separate so that
                 a wrong model can replace one of them.
    ref_cmn      features.cmvn_floating_kaldi(x, lc, rc, norm_vars=False) as its definition reads: one mean per frame.
    signal       one seeded speech-like recording per rate; every case is a slice of it.
    cases        named (first sample, samples) slices: the mirror edges, every frame count around the 16-frame wave run,
                 the 64-frame workgroup and the 300-frame default window, each at its smallest and largest sample count,
                 a loud tone and digital silence.

Only the definitions test_fbank_host.py pins to the reference at 1e-15 are taken from the package (geometry, mel_matrix,
povey_window, n_frames); nothing here touches the device library.
"""
import functools

import numpy as np

from vbx_amd import fbank

RATES = (16000, 8000)
PREEMPH = 0.97
SIGNAL_SECONDS = 9.5
FRAME_COUNTS = (2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 299, 300, 301, 364, 470)
# (lc, rc): the default; a window of one frame; windows that slide inside a 16-frame wave run and across the 64-frame
# workgroup boundary of segments of 15 .. 129 frames; a window longer than every segment
CMN_SETTINGS = ((150, 149), (0, 0), (0, 5), (5, 0), (5, 3), (20, 43), (1000, 1000))
SHORT_WINDOWS = tuple(s for s in CMN_SETTINGS if s[0] + s[1] + 1 < 64)
GATHER_LENGTHS = (1, 2, 63, 64, 127, 128, 129, 144, 255, 256, 257, 300)

# log-Mel rows: the project's own bound is 1e-6 (the power spectrum is kept in f32, 2^-24 relative on each term of a Mel
# sum of positive terms, so about 6e-8 on its log).  Measured on an MI355X over every case (test_gpu_fbank_kernels.py):
# 5.805e-8 at 16 kHz, 5.907e-8 at 8 kHz; the tolerance is four times the larger one
LOGMEL_MEASURED = 5.907e-8
LOGMEL_TOL = min(1e-6, 4 * LOGMEL_MEASURED)
FEA_TOL = 4e-6          # the project's end-to-end bound on the float32 features
CMN_SHARE = 0.01        # share of CMN outputs that may be a float32 neighbour of the reference's instead of equal to it


def dims(sr):
    """(pre, shift, winlen, nfft) of a rate: 120 / 160 / 400 / 512 at 16 kHz, half of each at 8 kHz."""
    g = fbank.geometry(sr)
    return g['noverlap'] // 2, g['shift'], g['winlen'], g['nfft']


def smallest(sr):
    """Samples of the smallest segment that holds a frame, pre + 2 n >= winlen: 140 at 16 kHz (pre + 20), 70 at 8 kHz."""
    pre, _, winlen, _ = dims(sr)
    return (winlen - pre + 1) // 2


# ---- reference -----------------------------------------------------------------------------------------------------
def pad(seg, sr):
    """predict.py:173-174: the first `pre` samples mirrored in front, at most winlen // 2 trailing ones behind."""
    pre, _, winlen, _ = dims(sr)
    seg = np.asarray(seg, dtype=np.float64)
    return np.concatenate([seg[:pre][::-1], seg, seg[::-1][:min(winlen // 2, len(seg))]])


def cut(padded, sr):
    """Frames of winlen samples every shift, [frames][winlen]; what is left behind the last full frame is dropped."""
    _, shift, winlen, _ = dims(sr)
    nf = (len(padded) - winlen) // shift + 1
    return np.stack([padded[f * shift:f * shift + winlen] for f in range(nf)])


def frames_to_logmel(frames, sr):
    """features.fbank_htk on cut frames -> (log-Mel rows, the Mel sums before the floor and the log)."""
    _, _, winlen, nfft = dims(sr)
    z = frames - frames.mean(axis=1, keepdims=True)
    y = np.empty_like(z)
    y[:, 0] = z[:, 0] * (1.0 - PREEMPH)
    y[:, 1:] = z[:, 1:] - PREEMPH * z[:, :-1]
    spec = np.fft.rfft(y * fbank.povey_window(winlen), nfft, axis=1)
    acc = (spec.real ** 2 + spec.imag ** 2) @ fbank.mel_matrix(sr)
    return np.log(np.maximum(1.0, acc)), acc


def ref_logmel(seg, sr):
    """(logmel [frames][64], acc [frames][64]) of one segment, float64."""
    return frames_to_logmel(cut(pad(seg, sr), sr), sr)


def ref_cmn(x, lc, rc):
    """Floating-window mean normalisation, the definition itself (features.py:207-216): float64 in, float64 out."""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    win = min(N, lc + rc + 1)
    out = np.empty_like(x)
    for t in range(N):
        ws = max(min(t - lc, N - win), 0)
        out[t] = x[t] - x[ws:ws + win].mean(0)
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------
def samples(n, sr, seed):
    """Seeded speech-like int16 samples: harmonics of a wandering pitch under a syllable envelope (amplitude about 3000),
    white noise, and a low rumble that keeps the lowest Mel channels (below the pitch) well above the floor."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f0 = 120 + 40 * np.sin(2 * np.pi * 0.3 * t) + 10 * rng.standard_normal(n).cumsum() / np.sqrt(n)
    ph = 2 * np.pi * np.cumsum(f0) / sr
    voiced = sum(np.sin(k * ph) / k for k in range(1, 30) if k * f0.max() < sr / 2)
    env = 0.5 + 0.5 * np.sin(2 * np.pi * 3.7 * t + rng.uniform(0, 6)) ** 2
    rumble = np.convolve(rng.standard_normal(n + 255), np.hanning(256), mode='valid')
    x = 1700 * env * voiced + 300 * rng.standard_normal(n) + 60 * rumble
    return np.clip(np.round(x), -32768, 32767).astype(np.int16), rng


def signal(n, sr, seed):
    """The float64 signal the front end is given: samples() plus a +-8 dither from the same generator."""
    x, rng = samples(n, sr, seed)
    return x + 8.0 * (2.0 * rng.random(n) - 1.0)


def n_signal(sr):
    return int(SIGNAL_SECONDS * sr)


@functools.lru_cache(maxsize=None)
def recording(sr):
    """The one signal of a rate every case is cut from (float64, read-only): the tone is written into the samples before
    the dither is added, the silence after it (digital silence: the signal itself is zero)."""
    n = n_signal(sr)
    x, rng = samples(n, sr, seed=2026 + sr)
    x = x.astype(np.float64)
    (_, a0, n0), (_, a1, n1) = _special(sr)
    x[a1:a1 + n1] = np.round(30000 * np.sin(2 * np.pi * 200 * np.arange(n1) / sr))
    x += 8.0 * (2.0 * rng.random(n) - 1.0)
    x[a0:a0 + n0] = 0.0
    x.setflags(write=False)
    return x


def _special(sr):
    """(name, first sample, samples): digital silence (40 frames) and the loud tone (65 frames), next to each other near
    the middle of the signal; no other case overlaps them (cases() places the others around them)."""
    _, shift, _, _ = dims(sr)
    a = n_signal(sr) // 2
    return [('silence', a, 40 * shift), ('tone', a + 40 * shift, 65 * shift)]


@functools.lru_cache(maxsize=None)
def cases(sr):
    """[(name, first sample, samples)], a fixed order.  Mirror edges and frame counts are placed by a seeded draw inside
    the part of the signal before or behind the special cases, so they overlap each other freely; 'N470max' starts at
    sample 0 and 'N364max' ends at the last sample."""
    pre, shift, winlen, _ = dims(sr)
    out = [('mirror-smallest', smallest(sr)), ('mirror-pre+20', pre + 20), ('mirror-shift+1', shift + 1),
           ('mirror-half-1', winlen // 2 - 1), ('mirror-half', winlen // 2), ('mirror-half+1', winlen // 2 + 1)]
    for N in FRAME_COUNTS:
        lo = shift * N - shift // 2
        out += [(f'N{N}min', lo), (f'N{N}max', lo + shift - 1)]
    total = n_signal(sr)
    sp = _special(sr)
    hole0, hole1 = sp[0][1], sp[-1][1] + sp[-1][2]
    rng = np.random.default_rng(77 + sr)
    placed = []
    for name, n in out:
        if name == 'N470max':
            a = 0
        elif name == 'N364max':
            a = total - n
        else:
            before = rng.integers(0, 2) == 0
            if n > hole0:
                before = False
            if n > total - hole1:
                before = True
            a = int(rng.integers(0, hole0 - n + 1)) if before else int(rng.integers(hole1, total - n + 1))
        assert 0 <= a and a + n <= total and (a + n <= hole0 or a >= hole1), (name, a, n)
        placed.append((name, a, n))
    return tuple(placed + sp)


def case_ids(sr):
    return [c[0] for c in cases(sr)]


def segment(sr, name):
    a, n = {c[0]: c[1:] for c in cases(sr)}[name]
    return recording(sr)[a:a + n]


@functools.lru_cache(maxsize=None)
def reference(sr):
    """{case: (logmel, acc)} of every case, computed once and read-only."""
    out = {}
    for name, a, n in cases(sr):
        lm, acc = ref_logmel(recording(sr)[a:a + n], sr)
        lm.setflags(write=False)
        acc.setflags(write=False)
        out[name] = (lm, acc)
    return out


# ---- comparison ----------------------------------------------------------------------------------------------------
# Each returns how far `got` is from the reference in units of the check's tolerance: <= 1 passes.  A wrong shape (a
# frame too few or too many) is infinitely far.
def logmel_excess(got, ref, tol=None):
    if got.shape != ref.shape:
        return np.inf
    return float(np.abs(got - ref).max()) / (LOGMEL_TOL if tol is None else tol)


def fea_excess(got, ref64):
    """float32 features against float32(ref64), in units of FEA_TOL."""
    if got.shape != ref64.shape:
        return np.inf
    return float(np.abs(got.astype(np.float64) - ref64.astype(np.float32).astype(np.float64)).max()) / FEA_TOL


def cmn_slack(x, lc, rc, terms=None):
    """What float64 rounding may put between two evaluations of x[t] - mean(window), absolutely: u = 2^-53 per operation
    on values of at most X = max |x|.  A window sum of `win` terms that is then slid up to 15 times (the kernel) or summed
    pairwise (ref_cmn) carries at most (win + 2 * 15) u win X, so its mean (win + 30) u X; the division, the subtraction
    and the reference's own mean stay within another 18 u X.  `terms` replaces win + 48 for another formulation (host_cmn's
    differences of cumulative sums: 2 N^2).  At most 1e-12 for every case here, 1e-5 of a float32 step at 1."""
    win = min(len(x), lc + rc + 1)
    return (win + 48 if terms is None else terms) * 2.0 ** -53 * float(np.abs(x).max())


def cmn_steps(got, ref64, slack=0.0):
    """(largest distance from float32(ref64) in float32 steps at that value, elements that differ from it, elements that
    differ from it by more than `slack`, elements).
    The check: at most one step (the value itself or one of its two float32 neighbours), and at most CMN_SHARE differ.
    For the distance, an element within `slack` (cmn_slack) of ref64 counts as equal: where x[t] and the mean cancel, a
    float32 step is as small as the result, and two float64 evaluations of the same window are then many such steps
    apart (at a window of one frame the reference is exactly 0 and a slid sum now and then gives 1e-15).  Every element
    of ordinary size is judged by its float32 neighbours alone: slack is 1e-5 of its step."""
    if got.shape != ref64.shape:
        return np.inf, got.size, got.size, got.size
    assert got.dtype == np.float32
    r = ref64.astype(np.float32)
    up, down = np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))
    g, r64 = got.astype(np.float64), r.astype(np.float64)
    steps = np.where(g >= r64, (g - r64) / (up.astype(np.float64) - r64), (r64 - g) / (r64 - down.astype(np.float64)))
    judged = np.abs(g - ref64) > slack
    steps = np.where(judged, steps, 0.0)
    ok = (got == r) | (got == up) | (got == down) | ~judged
    worst = float(steps.max()) if steps.size else 0.0
    if not ok.all():
        worst = max(worst, 2.0)                                   # (never reports a pass for an element outside the three)
    return worst, int((got != r).sum()), int(((got != r) & judged).sum()), got.size


def gather_ref(fea, start, length):
    """The window the gather kernels write for rows start .. start + length: [64][length]."""
    return np.ascontiguousarray(fea[start:start + length].T)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
