"""The x-vector extractor's front end on the GPU: what predict.py does between the WAV file and the embedding network.

    read_wav / read_lab        predict.py:149-151 (16-bit PCM through the standard library; soundfile is not needed)
    dither                     predict.py:169-170, numpy's legacy generator on the host (bit-exact)
    mt19937_seed_state,        the same dither drawn on the device (FrontEnd.run_raw, dither_on='device'): the state
    raw_samples                np.random.seed leaves, and the int16 samples that go up instead of the f64 signal
    povey_window, mel_matrix   features.py:povey_window / mel_fbank_mx(htk_bug=False) for the two supported rates
    segments, window_plan      predict.py:171-204: which VAD segments are processed, the 144-frame windows every 24
                               frames, their ark keys and segments-file lines
    FrontEnd                   the device path (libvbx_hip.so, vbx_fbank.hpp): log-Mel filterbank with the folded f64
                               frame operator, floating-window CMN, windows in the model's [B, 64, T] layout
    features, windows          one-call conveniences over FrontEnd

The network after it is vbx_amd.xvector (ResNet101 from a checkpoint, on the same device stream).
"""
from __future__ import annotations

import wave
from dataclasses import dataclass

import numpy as np

from . import _capi

N_MEL, LOFREQ, PREEMPH, DITHER_LEVEL, DITHER_SEED = 64, 20.0, 0.97, 8, 3
CMN_LC, CMN_RC = 150, 149
# predict.py:152-163
RATES = {16000: dict(winlen=400, noverlap=240, nfft=512, hifreq=7600.0),
         8000: dict(winlen=200, noverlap=120, nfft=256, hifreq=3700.0)}


def geometry(sr: int) -> dict:
    if sr not in RATES:
        raise ValueError(f'Only 8kHz and 16kHz are supported. Got {sr} instead.')
    g = dict(RATES[sr])
    g['shift'] = g['winlen'] - g['noverlap']
    return g


# ---- input ---------------------------------------------------------------------------------------------------------
def read_wav(path: str, raw: bool = False):
    """(samples as int64, sample rate) of a mono 16-bit PCM WAV at 8 or 16 kHz: (sf.read(path)[0] * 2**15).astype(int) of
    predict.py:149,170 is exactly the int16 sample values for such a file.  Anything else is refused.  raw: the samples
    stay int16, as the device dither takes them."""
    with wave.open(path, 'rb') as w:
        ch, width, sr, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        if ch != 1 or width != 2:
            raise ValueError(f'{path}: {ch} channel(s) of {8 * width}-bit samples; only mono 16-bit PCM is supported')
        geometry(sr)
        data = w.readframes(n)
    return np.frombuffer(data, dtype='<i2').astype(np.int16 if raw else np.int64), sr


def write_wav(path: str, samples, sr: int):
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sr))
        w.writeframes(np.asarray(samples, dtype='<i2').tobytes())


def read_lab(path: str, sr: int) -> np.ndarray:
    """VAD labels in samples, [n][2] int64: predict.py:150-151 (times * sr truncated; a one-line file gives one row)."""
    return np.atleast_2d((np.loadtxt(path, usecols=(0, 1)) * sr).astype(int))


def dither(x, seed: int = DITHER_SEED, level: int = DITHER_LEVEL) -> np.ndarray:
    """features.add_dither after np.random.seed(seed) (predict.py:169-170), without touching the global generator."""
    return x + level * (np.random.RandomState(seed).rand(*np.shape(x)) * 2 - 1)


def mt19937_seed_state(seed: int) -> np.ndarray:
    """The 624 words np.random.RandomState(seed) starts from (init_genrand of an int seed): mt[0] = seed,
    mt[i] = 1812433253 (mt[i - 1] ^ (mt[i - 1] >> 30)) + i mod 2^32.  The device does the same for run_raw."""
    seed = int(seed)
    if not 0 <= seed < 2 ** 32:
        raise ValueError(f'Seed must be between 0 and 2**32 - 1, got {seed}')
    mt = np.empty(624, dtype=np.uint32)
    w = seed
    mt[0] = w
    for i in range(1, 624):
        w = (1812433253 * (w ^ (w >> 30)) + i) & 0xffffffff
        mt[i] = w
    return mt


def raw_samples(x) -> np.ndarray:
    """The samples of a recording as int16, the type the device dithers: an integer array (what read_wav returns) whose
    values fit; anything else is refused, never wrapped."""
    x = np.asarray(x)
    if x.dtype.kind not in 'iu':
        raise ValueError(f'raw samples must be integers, got dtype {x.dtype}')
    x = x.reshape(-1)
    if x.dtype == np.int16 or x.size == 0:
        return x.astype(np.int16, copy=False)
    if x.min() < -32768 or x.max() > 32767:
        bad = int(np.flatnonzero((x < -32768) | (x > 32767))[0])
        raise ValueError(f'sample {bad} is {int(x[bad])}: outside int16 [-32768, 32767]')
    return x.astype(np.int16)


# ---- filterbank definition -----------------------------------------------------------------------------------------
def povey_window(L: int) -> np.ndarray:
    """(1/2 - 1/2 cos(2 pi l / (L - 1)))^0.85, l = 0 .. L - 1 (both ends included: a linspace, not a periodic window)."""
    return (0.5 - 0.5 * np.cos(np.linspace(0.0, 2.0 * np.pi, L))) ** 0.85


def mel_matrix(sr: int) -> np.ndarray:
    """[nfft/2 + 1][64] triangular filters on the HTK Mel scale 1127 ln(1 + f / 700) between 20 Hz and HIFREQ, with
    edges at bin floor(f nfft / sr) + 1 (features.mel_fbank_mx(winlen, sr, 64, 20, HIFREQ, htk_bug=False))."""
    g = geometry(sr)
    nfft = g['nfft']
    to_mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)          # noqa: E731
    from_mel = lambda m: (np.exp(m / 1127.0) - 1.0) * 700.0      # noqa: E731
    bins = to_mel(np.arange(nfft // 2 + 1, dtype=float) * sr / nfft)
    edges = np.linspace(to_mel(LOFREQ), to_mel(g['hifreq']), N_MEL + 2)
    first = np.floor(from_mel(edges) / sr * nfft).astype(int) + 1
    out = np.zeros((nfft // 2 + 1, N_MEL))
    for m in range(N_MEL):
        lo, mid, hi = first[m], first[m + 1], first[m + 2]
        out[lo:mid, m] = (edges[m] - bins[lo:mid]) / (edges[m] - edges[m + 1])
        out[mid:hi, m] = (edges[m + 2] - bins[mid:hi]) / (edges[m + 2] - edges[m + 1])
    return out


def frame_operator(sr: int) -> np.ndarray:
    """The four linear steps of a frame as one f64 operator [2K][L] (K = nfft/2 + 1): rows 0 .. K-1 the real part of the
    rfft, K .. 2K-1 the imaginary part, of window * preemphasis(frame - mean(frame)).  The device builds the same product
    (vbx_host_fbank.hpp); here it serves the host checks."""
    g = geometry(sr)
    L, nfft = g['winlen'], g['nfft']
    K = nfft // 2 + 1
    Z = np.eye(L) - 1.0 / L
    P = np.eye(L) - PREEMPH * np.eye(L, k=-1)
    P[0, 0] -= PREEMPH
    q = (np.arange(K)[:, None] * np.arange(L)[None, :]) % nfft
    ang = 2.0 * np.pi * q / nfft
    WPZ = (povey_window(L)[:, None] * P) @ Z
    return np.vstack([np.cos(ang) @ WPZ, -np.sin(ang) @ WPZ])


def host_logmel(seg, sr: int) -> np.ndarray:
    """log-Mel rows of one mirror-padded segment through frame_operator (f64, host): the device's arithmetic, unfused."""
    g = geometry(sr)
    L, shift = g['winlen'], g['shift']
    nf = (len(seg) - L) // shift + 1
    frames = np.lib.stride_tricks.sliding_window_view(seg, L)[::shift][:nf]
    y = frames @ frame_operator(sr).T
    K = y.shape[1] // 2
    return np.log(np.maximum(1.0, (y[:, :K] ** 2 + y[:, K:] ** 2) @ mel_matrix(sr)))


def host_cmn(x, lc: int = CMN_LC, rc: int = CMN_RC) -> np.ndarray:
    """Floating-window mean normalisation (features.cmvn_floating_kaldi, norm_vars=False) written as window sums."""
    N = len(x)
    win = min(N, lc + rc + 1)
    ws = np.clip(np.arange(N) - lc, 0, N - win)
    c = np.vstack([np.zeros((1, x.shape[1])), np.cumsum(x, 0)])
    return x - (c[ws + win] - c[ws]) / win


def mirror_pad(seg, sr: int) -> np.ndarray:
    """predict.py:173-174: noverlap // 2 leading samples mirrored, then at most winlen // 2 trailing ones."""
    g = geometry(sr)
    pre, post = g['noverlap'] // 2, min(g['winlen'] // 2, len(seg))
    return np.concatenate([seg[:pre][::-1], seg, seg[::-1][:post]])


# ---- segments and windows ------------------------------------------------------------------------------------------
@dataclass
class Segment:
    segnum: int          # row of the .lab file
    start: int           # first sample
    n: int               # samples after clipping to the signal
    nframes: int
    lab: tuple           # the (start, end) label in samples as read


def n_frames(n: int, sr: int) -> int:
    g = geometry(sr)
    return (g['noverlap'] // 2 + n + min(g['winlen'] // 2, n) - g['winlen']) // g['shift'] + 1


def segments(labs, n_signal: int, sr: int) -> list:
    """The segments predict.py:171-172 processes: longer than 0.01 s after slicing the signal."""
    out = []
    for segnum, (a, b) in enumerate(np.asarray(labs)):
        lo, hi = min(max(int(a), 0), n_signal), min(int(b), n_signal)
        n = max(hi - lo, 0)
        if n > 0.01 * sr:
            out.append(Segment(segnum, lo, n, n_frames(n, sr), (a, b)))
    return out


@dataclass
class Window:
    key: str
    seg: int             # index into the segment list
    start: int           # first frame within the segment
    end: int             # one past the last frame
    line: str            # the segments-file line (without the line end)


def window_plan(fn: str, segs, sr: int, seg_len: int = 144, seg_jump: int = 24) -> list:
    """Every window predict.py:181-204 embeds, in the order it writes them: full windows at range(0, slen - seg_len,
    seg_jump), then the tail fea[start + seg_jump:] if it holds at least 10 frames.  Times are printed as the reference
    prints them: round(numpy float64, 3) through str()."""
    out = []
    for si, s in enumerate(segs):
        slen, lab0, lab1 = s.nframes, s.lab[0], s.lab[1]
        start = -seg_jump
        for start in range(0, slen - seg_len, seg_jump):
            key = f'{fn}_{s.segnum:04}-{start:08}-{(start + seg_len):08}'
            t0 = round(lab0 / float(sr) + start / 100.0, 3)
            t1 = round(lab0 / float(sr) + start / 100.0 + seg_len / 100.0, 3)
            out.append(Window(key, si, start, start + seg_len, f'{key} {fn} {t0} {t1}'))
        if slen - start - seg_jump >= 10:
            key = f'{fn}_{s.segnum:04}-{(start + seg_jump):08}-{slen:08}'
            t0 = round(lab0 / float(sr) + (start + seg_jump) / 100.0, 3)
            t1 = round(lab1 / float(sr), 3)
            out.append(Window(key, si, start + seg_jump, slen, f'{key} {fn} {t0} {t1}'))
    return out


# ---- device path ---------------------------------------------------------------------------------------------------
class FrontEnd:
    """Filterbank + CMN of one sample rate on one device.  run() takes one or more recordings (dithered f64 signals with
    their segment lists), lays them end to end and computes all their features in one launch sequence; the features
    stay on the device until get() / windows() copy them out.  run_raw() takes the undithered integer samples instead
    and draws the dither on the device, to the same bits."""

    def __init__(self, sr: int, device: int = 0):
        g = geometry(sr)
        self.sr, self.device, self.g = sr, int(device), g
        if _capi._lib is None:
            # PyTorch-ROCm carries its own HIP runtime under the same soname: loaded first, it is the one libvbx_hip.so
            # binds to, so that device pointers of torch tensors are valid here (two runtimes in one process do not
            # share the device)
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        self.ctx = _capi.default_context(self.device)
        self.dev = _capi.FbankDevice(self.ctx, g['winlen'], g['shift'], g['nfft'], povey_window(g['winlen']),
                                     mel_matrix(sr), PREEMPH)
        self.seg_rows = []                       # per recording of the last run: [row0 of every segment]
        self.rows = 0

    def run(self, recordings) -> list:
        """recordings: [(signal f64, [Segment])].  Returns per recording the first feature row of each segment."""
        sigs, table, rows, off, seg_rows = [], [], 0, 0, []
        for sig, segs in recordings:
            r = []
            for s in segs:
                table.append((off + s.start, s.n))
                r.append(rows)
                rows += s.nframes
            seg_rows.append(r)
            sigs.append(np.asarray(sig, dtype=np.float64))
            off += len(sig)
        if not table:
            self.seg_rows, self.rows = seg_rows, 0
            return seg_rows
        got = self.dev.run(np.concatenate(sigs), np.array(table, dtype=np.int64).reshape(-1, 2), CMN_LC, CMN_RC)
        assert got == rows, (got, rows)
        self.seg_rows, self.rows = seg_rows, rows
        return seg_rows

    def run_raw(self, recordings, seed: int = DITHER_SEED, level=DITHER_LEVEL) -> list:
        """recordings: [(int samples, [Segment])].  run() on dither(samples, seed, level) of every recording, with the
        dither drawn on the device (one workgroup per recording follows numpy's MT19937 stream from the seed) and the
        int16 samples uploaded instead of the f64 signal.  Returns what run() returns."""
        mt19937_seed_state(seed)                 # (refuses what numpy refuses)
        raws, recs, table, rows, off, seg_rows = [], [], [], 0, 0, []
        for x, segs in recordings:
            r = []
            for s in segs:
                table.append((off + s.start, s.n))
                r.append(rows)
                rows += s.nframes
            seg_rows.append(r)
            raws.append(raw_samples(x))
            recs.append((off, len(raws[-1])))
            off += len(raws[-1])
        if not table:
            self.seg_rows, self.rows = seg_rows, 0
            return seg_rows
        got = self.dev.run_raw(np.concatenate(raws), np.array(recs, dtype=np.int64).reshape(-1, 2),
                               np.full(len(recs), int(seed), dtype=np.uint32), np.full(len(recs), float(level)),
                               np.array(table, dtype=np.int64).reshape(-1, 2), CMN_LC, CMN_RC)
        assert got == rows, (got, rows)
        self.seg_rows, self.rows = seg_rows, rows
        return seg_rows

    def signal(self, first: int, n: int) -> np.ndarray:
        """Samples [first, first + n) of the f64 signal of the last run, recordings end to end: what run() was given, or
        what run_raw() dithered."""
        return self.dev.signal(first, n)

    def _torch_empty(self, shape, dtype):
        import torch
        if not torch.cuda.is_available():
            raise _capi.VbxError('PyTorch sees no GPU in this process: import torch before libvbx_hip.so is loaded '
                                 '(the first vbx_amd call on the device), so that both use one HIP runtime')
        dev = torch.device('cuda', self.device)
        t = torch.empty(shape, dtype=dtype, device=dev)
        torch.cuda.current_stream(dev).synchronize()   # the block may still be in use by work queued before it was freed
        return t

    def get(self, row0: int, nrows: int, which: str = 'fea', out: str = 'numpy'):
        """Feature rows ('fea': CMN, f32; 'logmel': before CMN, f64) as a numpy array or a torch tensor on the device."""
        if out == 'numpy':
            return self.dev.get(which, row0, nrows)
        import torch
        t = self._torch_empty((nrows, N_MEL), torch.float32 if which == 'fea' else torch.float64)
        if nrows:
            self.dev.get(which, row0, nrows, dst_ptr=t.data_ptr())
        return t

    def windows(self, starts, length: int, out: str = 'numpy'):
        """[n][64][length] f32 windows starting at feature rows `starts` (numpy, or a torch tensor on the device)."""
        starts = np.asarray(starts, dtype=np.int64)
        if out == 'numpy':
            return self.dev.windows(starts, length)
        import torch
        t = self._torch_empty((len(starts), N_MEL, int(length)), torch.float32)
        if len(starts):
            self.dev.windows(starts, length, dst_ptr=t.data_ptr())
        return t

    def times(self) -> dict:
        return self.dev.times()

    def dither_time(self) -> float:
        """Device ms of the dither kernel of the last run_raw."""
        return self.dev.dither_time()


_front_ends = {}


def front_end(sr: int, device: int = 0) -> FrontEnd:
    key = (sr, int(device))
    if key not in _front_ends:
        _front_ends[key] = FrontEnd(sr, device)
    return _front_ends[key]


def prepare(samples, labs, sr: int, dither_signal: bool = True):
    """(f64 signal, processed segments) of one recording: predict.py:169-172."""
    x = dither(samples) if dither_signal else np.asarray(samples, dtype=np.float64)
    return x, segments(labs, len(samples), sr)


def _run(fe, recordings, sr: int, dither_signal: bool, dither_on: str):
    """One FrontEnd run over [(int samples, labels in samples)]: (first rows per recording, segments per recording)."""
    if dither_on not in ('host', 'device'):
        raise ValueError(f"dither_on must be 'host' or 'device', got {dither_on!r}")
    if dither_on == 'device':
        if not dither_signal:
            raise ValueError("dither_on='device' draws the dither: it cannot go with dither_signal=False")
        prep = [(x, segments(labs, len(x), sr)) for x, labs in recordings]
        return fe.run_raw(prep), [segs for _, segs in prep]
    prep = [prepare(x, labs, sr, dither_signal) for x, labs in recordings]
    return fe.run(prep), [segs for _, segs in prep]


def features(recordings, sr: int, device: int = 0, dither_signal: bool = True, out: str = 'numpy',
             dither_on: str = 'host') -> list:
    """recordings: [(int samples, labels in samples)] of one sample rate.  Per recording, the list of its processed
    segments' CMN features ([nframes][64] f32) as predict.py:175-177 computes them.  dither_on: 'host' draws the dither with
    numpy and uploads the f64 signal, 'device' uploads the int16 samples and draws it there; the features are the same."""
    fe = front_end(sr, device)
    seg_rows, seg_lists = _run(fe, recordings, sr, dither_signal, dither_on)
    return [[fe.get(r0, s.nframes, out=out) for r0, s in zip(rows, segs)] for rows, segs in zip(seg_rows, seg_lists)]


def windows(samples, labs, sr: int, fn: str, device: int = 0, seg_len: int = 144, seg_jump: int = 24,
            dither_signal: bool = True, out: str = 'numpy', dither_on: str = 'host'):
    """The windows of one recording: (plan, full windows [B][64][seg_len], {length: (plan indices, [n][64][length])}
    for the tails), in the order of window_plan().  dither_on as for features()."""
    fe = front_end(sr, device)
    seg_rows, seg_lists = _run(fe, [(samples, labs)], sr, dither_signal, dither_on)
    rows, segs = seg_rows[0], seg_lists[0]
    plan = window_plan(fn, segs, sr, seg_len, seg_jump)
    full = [i for i, w in enumerate(plan) if w.end - w.start == seg_len]
    full_t = fe.windows([rows[plan[i].seg] + plan[i].start for i in full], seg_len, out=out)
    tails = {}
    for i, w in enumerate(plan):
        if w.end - w.start != seg_len:
            tails.setdefault(w.end - w.start, []).append(i)
    tail_t = {n: (idx, fe.windows([rows[plan[i].seg] + plan[i].start for i in idx], n, out=out)) for n, idx in tails.items()}
    return plan, full, full_t, tail_t
