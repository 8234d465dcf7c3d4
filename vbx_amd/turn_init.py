"""The host side of ``--init RTTM`` / ``--init RTTM+VB``: a diarization that exists, read from
``<dir>/<recording>.rttm``, as the integer arrays ``vbx_turn_weights`` and ``vbx_batch_set_recording_turns`` take.

All times become integer microseconds here and nowhere else: ``tick(x) = int(round(x * 1e6))``; a turn is
``[tick(start), tick(start) + tick(duration))``, a window ``[tick(seg_start), tick(seg_end))``.  Everything after that -- the
merging below and the overlaps on the device -- is integer arithmetic, so a tie is a tie on the host and on the device alike.
"""
from __future__ import annotations

import os

import numpy as np

__all__ = ['INITS', 'tick', 'window_ticks', 'turn_ticks', 'read_init_turns', 'check_init_rttm_dir']

INITS = ('RTTM', 'RTTM+VB')       # the --init values that start from given turns


def tick(seconds):
    """Seconds to integer microseconds, rounded to the nearest (Python's round: halves to even)."""
    return int(round(float(seconds) * 1e6))


def window_ticks(times):
    """(a, b) int64 [T]: the x-vector windows ``times`` [T][2] = (start, end) seconds of the segments file in ticks."""
    times = np.asarray(times, dtype=float).reshape(-1, 2)
    a = np.array([tick(t) for t in times[:, 0]], dtype=np.int64)
    b = np.array([tick(t) for t in times[:, 1]], dtype=np.int64)
    return a, b


def turn_ticks(turns, recording='?'):
    """``turns`` = [(start, duration, speaker name)] in file order -> ``(u, v, spk, names)``: int64 [N] ticks, int32 [N] speaker
    indices and the speakers' names by index.  Speakers are numbered by first appearance (before anything is dropped), turns
    with ``v <= u`` are dropped, turns of one speaker that overlap or touch are merged, and what is left is sorted by
    (speaker, start).  ValueError that names the recording when no turn is left."""
    names, by_spk = [], {}
    for start, dur, name in turns:
        if name not in by_spk:
            by_spk[name] = []
            names.append(name)
        u = tick(start)
        v = u + tick(dur)
        if v > u:
            by_spk[name].append((u, v))
    merged = []                                                   # [u, v, speaker], by (speaker, start)
    for s, name in enumerate(names):
        first = len(merged)
        for u, v in sorted(by_spk[name]):
            if len(merged) > first and u <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], v)
            else:
                merged.append([u, v, s])
    if not merged:
        raise ValueError(f'{recording}: no speaker turn of positive duration to start from')
    u, v, spk = zip(*merged)
    return np.array(u, dtype=np.int64), np.array(v, dtype=np.int64), np.array(spk, dtype=np.int32), names


def check_init_rttm_dir(rttm_dir):
    """ValueError unless ``rttm_dir`` names a directory (found before the run, not after it)."""
    if rttm_dir is None:
        raise ValueError('--init RTTM and RTTM+VB need --init-rttm-dir (init_rttm_dir): the diarization to start from')
    if not os.path.isdir(rttm_dir):
        raise ValueError(f'--init-rttm-dir {rttm_dir}: no such directory')


def read_init_turns(rttm_dir, recording):
    """``turn_ticks`` of the SPEAKER lines of ``<rttm_dir>/<recording>.rttm`` whose file field is ``recording`` (read by
    ``score.read_turns``).  ValueError that names what is missing: the directory, the file, or the recording in it."""
    from .score import read_turns
    check_init_rttm_dir(rttm_dir)
    path = os.path.join(rttm_dir, f'{recording}.rttm')
    if not os.path.isfile(path):
        raise ValueError(f'--init-rttm-dir {rttm_dir}: no {recording}.rttm')
    turns = read_turns(path, durations=True).get(recording)
    if not turns:
        raise ValueError(f'{path}: no SPEAKER line for recording {recording}')
    return turn_ticks([(start, dur, spk) for start, _end, spk, dur in turns], recording)
