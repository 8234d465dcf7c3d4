"""The referee of ``--init RTTM`` / ``--init RTTM+VB``, written from its definition and from nothing else:
numpy and Python integers.  No import from vbx_amd.

    tick(x) = int(round(x * 1e6))                         integer microseconds; nothing below sees a float time
    turn    = [u, v) = [tick(start), tick(start) + tick(duration)) of speaker s; window i = [a_i, b_i) = ticks of the segments file
    speakers are numbered by first appearance; turns with v <= u are dropped; turns of one speaker that overlap or touch are merged
    d[i][s] = sum over the turns j of s of max(0, min(b_i, v_j) - max(a_i, u_j))          D_i = sum_s d[i][s]
    D_i > 0:   w[i][s] = d[i][s] / D_i,  label[i] = argmax_s d[i][s], the lowest among equals
    D_i == 0:  the turn with the smallest gap max(u_j - b_i, a_i - v_j) names the speaker, the lowest index among equal gaps;
               w[i] is its one-hot row and label[i] that speaker
    qinit[i] = softmax(init_smoothing * w[i])
"""
import os

import numpy as np


def tick(seconds):
    return int(round(seconds * 1e6))


def read_speaker_lines(path, recording):
    """[(start, duration, speaker name)] of the SPEAKER lines of ``path`` whose file field is ``recording``, in file order."""
    out = []
    with open(path) as fp:
        for line in fp:
            f = line.split()
            if f and f[0] == 'SPEAKER' and f[1] == recording:
                out.append((float(f[3]), float(f[4]), f[7]))
    return out


def prepare(lines):
    """``lines`` = [(start, duration, speaker name)] -> (u, v, spk, S): int64 ticks and speaker indices of the turns that are
    left, sorted by (speaker, start); S counts every speaker that appears.  ValueError when no turn is left."""
    order = []
    for _start, _dur, name in lines:
        if name not in order:
            order.append(name)
    turns = []
    for s, name in enumerate(order):
        mine = sorted((tick(start), tick(start) + tick(dur)) for start, dur, n in lines if n == name)
        mine = [(u, v) for u, v in mine if v > u]
        merged = []
        for u, v in mine:
            if merged and u <= merged[-1][1]:
                merged[-1] = (merged[-1][0], max(merged[-1][1], v))
            else:
                merged.append((u, v))
        turns += [(u, v, s) for u, v in merged]
    if not turns:
        raise ValueError('no turn left')
    u, v, spk = (np.array(c, dtype=np.int64) for c in zip(*turns))
    return u, v, spk, len(order)


def read(rttm_dir, recording):
    return prepare(read_speaker_lines(os.path.join(rttm_dir, f'{recording}.rttm'), recording))


def windows(times):
    """(a, b): the [T][2] start / end seconds of the segments file in ticks."""
    times = np.asarray(times, dtype=float).reshape(-1, 2)
    return (np.array([tick(float(t)) for t in times[:, 0]], dtype=np.int64),
            np.array([tick(float(t)) for t in times[:, 1]], dtype=np.int64))


def overlaps(a, b, u, v, spk, S):
    """d int64 [T][S]."""
    a, b, u, v = (np.asarray(x, dtype=np.int64) for x in (a, b, u, v))
    over = np.maximum(0, np.minimum(b[:, None], v[None, :]) - np.maximum(a[:, None], u[None, :]))      # [T][N]
    d = np.zeros((len(a), S), dtype=np.int64)
    for j, s in enumerate(np.asarray(spk)):
        d[:, s] += over[:, j]
    return d


def nearest(a, b, u, v, spk):
    """int [T]: the speaker of the turn with the smallest gap, the lowest speaker among equal gaps."""
    a, b, u, v, spk = (np.asarray(x, dtype=np.int64) for x in (a, b, u, v, spk))
    gap = np.maximum(u[None, :] - b[:, None], a[:, None] - v[None, :])                                  # [T][N]
    out = np.empty(len(a), dtype=np.int64)
    for i in range(len(a)):
        out[i] = spk[gap[i] == gap[i].min()].min()
    return out


def weights(a, b, u, v, spk, S):
    """-> (labels int64 [T], w float64 [T][S], d int64 [T][S])"""
    d = overlaps(a, b, u, v, spk, S)
    D = d.sum(axis=1)
    near = nearest(a, b, u, v, spk)
    w = np.zeros(d.shape)
    labels = np.empty(len(D), dtype=np.int64)
    for i in range(len(D)):
        if D[i] > 0:
            w[i] = d[i].astype(np.float64) / np.float64(D[i])
            labels[i] = int(np.argmax(d[i]))                       # (argmax: the first of the largest)
        else:
            w[i, near[i]] = 1.0
            labels[i] = near[i]
    return labels, w, d


def qinit(w, init_smoothing):
    x = init_smoothing * np.asarray(w, dtype=np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def rename_by_first_appearance(names):
    """{name: index} in order of first appearance."""
    out = {}
    for n in names:
        out.setdefault(n, len(out))
    return out
