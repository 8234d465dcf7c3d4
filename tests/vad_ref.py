"""Referee of the energy VAD, written from the definition and independently of vbx_amd/vad.py: plain
loops over frames and runs, Python integers for N, no cumulative sums.  It also reports how far the nearest frame energy
lies from the threshold, the margin inside which a decision could legitimately flip with rounding."""
import math

import numpy as np

GEOMETRY = {16000: (400, 160), 8000: (200, 80)}          # sample rate -> (L, H)
DEFAULTS = dict(energy_threshold=5.5, mean_scale=0.5, context=2, proportion=0.12, min_silence=30, min_speech=20, pad=0)


def frame_energies(x, sr):
    L, H = GEOMETRY[sr]
    n = len(x)
    T = (n - L) // H + 1 if n >= L else 0
    N = []
    for t in range(T):
        fr = np.asarray(x[t * H:t * H + L]).astype(np.int64)
        s, q = int(fr.sum()), int((fr * fr).sum())          # (400 squares of 2^30 at most: no int64 overflow)
        N.append(L * q - s * s)
    return N


def raw_decisions(e, theta, context, proportion):
    T = len(e)
    raw = []
    for t in range(T):
        n_in = n_hot = 0
        for t2 in range(t - context, t + context + 1):
            if 0 <= t2 < T:
                n_in += 1
                n_hot += 1 if e[t2] > theta else 0
        raw.append(1 if float(n_hot) >= float(n_in) * proportion else 0)
    return raw


def maximal_runs(seq, value):
    out, t = [], 0
    while t < len(seq):
        if seq[t] == value:
            a = t
            while t < len(seq) and seq[t] == value:
                t += 1
            out.append((a, t))
        else:
            t += 1
    return out


def smooth(raw, min_silence, min_speech, pad):
    T = len(raw)
    s = list(raw)
    for a, b in maximal_runs(s, 0):                          # close
        if a > 0 and b < T and b - a < min_silence:
            s[a:b] = [1] * (b - a)
    for a, b in maximal_runs(list(s), 1):                    # drop
        if b - a < min_speech:
            s[a:b] = [0] * (b - a)
    padded = [0] * T                                         # pad
    for a, b in maximal_runs(s, 1):
        for t in range(max(a - pad, 0), min(b + pad, T)):
            padded[t] = 1
    return maximal_runs(padded, 1)


def energy_vad(x, sr, **kw):
    """One recording -> dict(N: Python ints, e, theta, raw, runs [(a, b)], margin = min_t |e[t] - theta| (inf if T = 0))."""
    p = dict(DEFAULTS, **kw)
    L, _ = GEOMETRY[sr]
    N = frame_energies(x, sr)
    T = len(N)
    e = [math.log(max(v / L, 1.0)) for v in N]
    theta = p['energy_threshold'] + (p['mean_scale'] * math.fsum(e) / T if T else 0.0)
    raw = raw_decisions(e, theta, p['context'], p['proportion'])
    runs = smooth(raw, p['min_silence'], p['min_speech'], p['pad'])
    margin = min((abs(v - theta) for v in e), default=math.inf)
    return dict(N=N, e=np.array(e, dtype=np.float64), theta=theta, raw=np.array(raw, dtype=np.uint8),
                runs=np.array(runs, dtype=np.int32).reshape(-1, 2), margin=margin)


def lab_text(runs, sr):
    _, H = GEOMETRY[sr]
    return ''.join('%.3f %.3f sp\n' % (a * H / sr, b * H / sr) for a, b in runs)


def ulps(a, b):
    """Largest distance in units of the last place between two arrays of non-negative doubles."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and (a >= 0).all() and (b >= 0).all()
    return int(np.abs(a.view(np.int64) - b.view(np.int64)).max()) if a.size else 0


# ---- synthetic audio ---------------------------------------------------------------------------------------------------
def bursts(seed, sr, pattern, loud=3000.0, quiet=10.0):
    """Gaussian noise, int16: ``pattern`` is [(frames, is_loud)], each stretch frames * H samples; L - H more samples of the
    last level close the last frame."""
    L, H = GEOMETRY[sr]
    rng = np.random.default_rng(seed)
    parts = [rng.normal(0.0, loud if on else quiet, size=f * H) for f, on in pattern]
    if parts:
        parts.append(rng.normal(0.0, loud if pattern[-1][1] else quiet, size=L - H))
    x = np.concatenate(parts) if parts else np.zeros(0)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def uniform(seed, n):
    """Full-scale int16 noise: the largest sums a frame can hold, short of a constant -32768."""
    return np.random.default_rng(seed).integers(-32768, 32768, size=n).astype(np.int16)


# ---- the cases both test files run: name -> (sample rate, samples, parameters, the runs expected by hand or None) ----
PLAIN = dict(context=0, proportion=0.5)                      # raw[t] = e[t] > theta
BARE = dict(min_silence=0, min_speech=0)
_CASES = {}


def cases():
    """With ``context 0`` a loud stretch of f frames from frame s makes the frames [s - 2, s + f) hot: frame s - 2 still holds
    half a shift of its samples.  The hand-written expectations below follow from that."""
    if _CASES:
        return _CASES
    q, l = (lambda n: (n, False)), (lambda n: (n, True))     # noqa: E741
    for sr in (16000, 8000):
        L, H = GEOMETRY[sr]
        k = sr // 1000

        def add(name, x, params=None, expect=None):
            _CASES[f'{name}-{k}k'] = (sr, x, dict(params or {}), expect)

        # N: the first frames, the tile edges, the largest sums
        for n in (0, L - 1, L, L + H - 1, L + H):
            add(f'n{n}', uniform(n, n))
        for T in (255, 256, 257, 512):
            add(f'T{T}', uniform(T, (T - 1) * H + L))
        add('floor', np.full(299 * H + L + 7, -32768, dtype=np.int16), expect=[])
        add('zero', np.zeros(199 * H + L, dtype=np.int16), expect=[])
        add('below', bursts(11, sr, [l(300)], loud=5.0), expect=[])             # e = log(L 25) < 11: below 5.5 + e / 2
        add('above', bursts(12, sr, [l(300)]), expect=[(0, 300)])                  # e = log(L 9e6) > 11: above it
        # the smoothing, on raw decisions that are the hot frames themselves
        add('gap29', bursts(21, sr, [q(10), l(40), q(31), l(40), q(10)]), PLAIN, [(8, 121)])
        add('gap30', bursts(22, sr, [q(10), l(40), q(32), l(40), q(10)]), PLAIN, [(8, 50), (80, 122)])
        add('speech19', bursts(23, sr, [q(10), l(17), q(50)]), PLAIN, [])
        add('speech20', bursts(24, sr, [q(10), l(18), q(50)]), PLAIN, [(8, 28)])
        add('rescued', bursts(25, sr, [q(10), l(5), q(12), l(40), q(60), l(5), q(40)]), PLAIN, [(8, 67)])
        add('pad_merge', bursts(26, sr, [q(30), l(30), q(42), l(30), q(30)]), dict(PLAIN, pad=20), [(8, 152)])
        add('pad_apart', bursts(26, sr, [q(30), l(30), q(42), l(30), q(30)]), dict(PLAIN, pad=19), [(9, 79), (81, 151)])
        add('pad_clip', bursts(27, sr, [q(5), l(30), q(60), l(30), q(1)]), dict(PLAIN, pad=10), [(0, 45), (83, 126)])
        add('bare', bursts(28, sr, [q(7), l(3), q(4), l(1), q(9), l(2), q(3)]), dict(PLAIN, **BARE), [(5, 10), (12, 15), (22, 26)])
        # the context window: across the tile edges 256 and 512, clipped at both ends of the recording, n_in * proportion hit
        add('tile_edge', bursts(29, sr, [q(252), l(5), q(97), l(160), q(2)]), BARE, [(248, 259), (350, 516)])
        add('starts_hot', bursts(30, sr, [l(4), q(30), l(3)]), BARE, [(0, 6), (30, 37)])
        add('prop_exact', bursts(31, sr, [q(20), l(10), q(20), l(6)]), dict(BARE, context=2, proportion=0.6), [(18, 30), (48, 56)])
        add('wide_context', bursts(32, sr, [q(20), l(10), q(20)]), dict(BARE, context=300, proportion=0.2), [(0, 50)])
        # more runs than one pass of the run-list stages takes, more frames than one pass of the boundary compaction
        add('many_runs', bursts(33, sr, [q(6), l(4)] * 330), dict(PLAIN, **BARE))
        add('many_merges', bursts(34, sr, [q(6), l(4), q(12), l(4)] * 200), dict(PLAIN, min_silence=5, min_speech=16, pad=4))
        add('one_merge', bursts(34, sr, [q(6), l(4), q(12), l(4)] * 200), dict(PLAIN, min_silence=11, min_speech=0, pad=0), [(4, 5200)])
        # seeded bursts of random lengths, the defaults
        for seed in (41, 42, 43):
            rng = np.random.default_rng(seed)
            pattern = [(int(rng.integers(5, 120)), bool(i & 1)) for i in range(60)]
            add(f'bursts{seed}', bursts(seed, sr, pattern))
        add('long', bursts(44, sr, [q(300), l(700)] * 4 + [q(40), l(100), q(200)]))          # a run across frame 4096
    return _CASES


_REFERENCE = {}


def reference(name):
    """The referee's result for a case, computed once and shared (treat it as read-only)."""
    if name not in _REFERENCE:
        sr, x, params, _ = cases()[name]
        _REFERENCE[name] = energy_vad(x, sr, **params)
    return _REFERENCE[name]
