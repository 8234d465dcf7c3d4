#!/usr/bin/env python
"""python -m vbx_amd.metrics: dscore's full table for system RTTM files against reference RTTM files.

    python -m vbx_amd.metrics -r ref.rttm -s sys.rttm --collar 0.25 [--ignore_overlaps] [--step 0.010] [--device 0]

The last step of the reference's recipes (``dscore/score.py -r ... -s ... --collar 0.25 [--ignore_overlaps]``) with the
program name swapped, all eleven columns of it:

    File  DER  JER  B3-Precision  B3-Recall  B3-F1  GKT(ref, sys)  GKT(sys, ref)  H(ref|sys)  H(sys|ref)  MI  NMI

DER is ``vbx_amd.score``'s (md-eval's, time-weighted; ``--collar`` and ``--ignore_overlaps`` act on this column only).  The
other ten are frame metrics, fixed by the row the reference's README publishes for ES2005a:

Frames.  The frame step is 0.010 s (``--step``).  Per recording, ``lo`` is the smallest turn start and ``hi`` the largest turn
end, reference and system together (turns without duration dropped; there is no UEM file, ``-u`` is refused).  Frame ``i``
exists for ``0 <= i < int(hi / step)``, its time is the float64 product ``step * i`` (not ``i / 100``: ``0.01 * 57`` is
0.5700000000000001, above the literal 0.57, and the rule sees it), a turn ``[b, e)`` holds the frames with ``b <= step * i <
e``, and only the frames with ``lo <= step * i < hi`` are counted.

JER.  ``ref_durs[r]``, ``sys_durs[s]``: frames per speaker; ``inter[r][s]``: frames that hold both; speakers without a frame
are dropped.  ``J[r][s] = 1 - inter / (ref_durs[r] + sys_durs[s] - inter)``, ``scipy.optimize.linear_sum_assignment`` on J
(on the host, as the DER mapping), an unmapped reference speaker scores 1, and the recording's JER is 100 times the mean
over its reference speakers.  Without a reference speaker it is 100 if the system has a speech frame, else 0.

Clustering columns.  A frame's class on a side is the set of speakers active in it -- the empty set (non-speech) and every
distinct overlap combination are classes like any other.  ``cm[a][b]`` counts frames by (reference class, system class),
``N = sum cm``, ``p = cm / N``.  B3 precision is ``sum(cm^2 / column sums) / N``, B3 recall the same with the row sums, F1
their harmonic mean.  ``GKT(ref, sys) = (V(sys) - V(sys|ref)) / V(sys)`` with ``V(Y) = 1 - sum_y p_y^2`` and ``V(Y|X) = 1 -
sum_x sum_y p_xy^2 / p_x``; ``GKT(sys, ref)`` with the sides swapped.  Entropies in bits, ``MI = H(ref) - H(ref|sys)``,
``NMI = MI / sqrt(H(ref) H(sys))``.  This project's choice where the published row says nothing: a GKT whose ``V(Y)`` is 0
is 1; NMI is 1 when both entropies are 0 and 0 when exactly one is; a recording without a counted frame scores B3 1 / 1 / 1,
GKT 1, entropies and MI 0, NMI 1.

``*** OVERALL ***``: DER pooled as in ``vbx_amd.score``; JER the mean over the reference speakers of all files, each weighing
the same; the clustering columns from the block-diagonal sum of the files' ``cm`` (classes of different files are
distinct).  With one published file these three rules could not be checked against dscore.

The integers (``ref_durs``, ``sys_durs``, ``inter``, the classes and ``cm``) come from the cells between the sorted distinct
frame indices of the turn boundaries -- never from one row per frame -- on the device for any number of pairs in one launch
sequence (``device=N``; vbx_frame_score.hpp) or in numpy (``device=None``).  The floating-point columns are always computed
here, in float64, from those integers: both routes give the same records bit for bit.

As a library: ``frame_counts``, ``score_turns``, ``score_rttm``, ``format_table``; for label sequences -- many hypotheses per
recording, the turns built on the device, as ``python -m vbx_amd.tune --criterion`` needs them -- ``frame_counts_labels`` and
``score_labels`` (vbx_labels_frame.hpp).
"""
from __future__ import annotations

import argparse
import math
import sys

import numpy as np

from . import score as _score
from .score import merge_turns

__all__ = ['frame_counts', 'frame_counts_labels', 'score_turns', 'score_labels', 'score_rttm', 'format_table', 'build_parser', 'main']

MAX_DEVICE_SPEAKERS = 64      # speakers per side the device route takes (vbx_frame_score.hpp: kFrmMaxSpk)
MAX_DEVICE_CLASSES = 256      # classes per side it returns (kFrmMaxCls)
MAX_DEVICE_FRAMES = 2 ** 40   # frames of a recording it indexes
HEADER = ['File', 'DER', 'JER', 'B3-Precision', 'B3-Recall', 'B3-F1', 'GKT(ref, sys)', 'GKT(sys, ref)', 'H(ref|sys)', 'H(sys|ref)',
          'MI', 'NMI']
COLUMNS = ['der', 'jer', 'b3_precision', 'b3_recall', 'b3_f1', 'gkt_ref_sys', 'gkt_sys_ref', 'h_ref_sys', 'h_sys_ref', 'mi', 'nmi']


# ---- the integers ---------------------------------------------------------------------------------------------------------
def _frame_index(x, step, n):
    """min(n, the first i >= 0 with step * i >= x) for every x: the number of frames below x.  The candidate floor(x / step)
    is corrected by comparing the float64 product with x (vbx_frame_score.hpp: frm_index)."""
    x = np.asarray(x, dtype=np.float64)
    c = np.where(x > 0, np.minimum(np.floor(x / step), float(n)), 0.0).astype(np.int64)
    while True:
        m = (c > 0) & (step * (c - 1).astype(np.float64) >= x)
        if not m.any():
            break
        c[m] -= 1
    while True:
        m = (c < n) & (step * c.astype(np.float64) < x)
        if not m.any():
            break
        c[m] += 1
    return c


class _Frames:
    """One recording ready for either route: merged turns as arrays, speaker names, extent."""

    def __init__(self, ref_turns, sys_turns):
        ref, hyp = merge_turns(ref_turns, touching=False), merge_turns(sys_turns, touching=False)
        self.ref_names = sorted({t[2] for t in ref}, key=str)
        self.sys_names = sorted({t[2] for t in hyp}, key=str)
        ri = {s: i for i, s in enumerate(self.ref_names)}
        si = {s: i for i, s in enumerate(self.sys_names)}
        self.rb = np.array([t[0] for t in ref], dtype=np.float64)
        self.re = np.array([t[1] for t in ref], dtype=np.float64)
        self.rs = np.array([ri[t[2]] for t in ref], dtype=np.int32)
        self.sb = np.array([t[0] for t in hyp], dtype=np.float64)
        self.se = np.array([t[1] for t in hyp], dtype=np.float64)
        self.ss = np.array([si[t[2]] for t in hyp], dtype=np.int32)
        times = np.concatenate([self.rb, self.re, self.sb, self.se])
        if not np.isfinite(times).all():
            raise ValueError('a turn has a time that is not finite')
        self.lo = float(min(a.min() for a in (self.rb, self.sb) if a.size)) if times.size else 0.0
        self.hi = float(max(a.max() for a in (self.re, self.se) if a.size)) if times.size else 0.0

    @property
    def n_ref(self):
        return len(self.ref_names)

    @property
    def n_sys(self):
        return len(self.sys_names)

    def n_frames(self, step):
        return int(self.hi / step) if self.hi > 0 else 0


def _active(fb, fe, spk, n_spk, u):
    """bool [cells][n_spk]: the speakers whose turns [fb, fe) hold the cells between the sorted distinct indices u"""
    delta = np.zeros((u.size, n_spk), dtype=np.int64)
    np.add.at(delta, (np.searchsorted(u, fb), spk), 1)
    np.add.at(delta, (np.searchsorted(u, fe), spk), -1)
    return np.cumsum(delta, axis=0)[:-1] > 0


def _classes(active, names):
    """(class of every cell, the classes as tuples of names) with the classes in order of first appearance"""
    if active.shape[0] == 0:
        return np.zeros(0, dtype=np.int64), []
    rows = np.packbits(np.concatenate([active, np.zeros((active.shape[0], 1), dtype=bool)], axis=1), axis=1)
    _, first, inverse = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.arange(order.size)
    return rank[inverse.reshape(-1)], [tuple(names[i] for i in np.flatnonzero(active[c])) for c in first[order]]


def _record(p, ref_durs, sys_durs, inter, ref_classes, sys_classes, cm):
    return dict(ref_speakers=list(p.ref_names), sys_speakers=list(p.sys_names), ref_durs=ref_durs, sys_durs=sys_durs, inter=inter,
                ref_classes=ref_classes, sys_classes=sys_classes, cm=cm)


def _host_counts(p, step):
    """The integer record of one pair in numpy: the cells of the device route."""
    n = p.n_frames(step)
    rb, re, sb, se = (_frame_index(a, step, n) for a in (p.rb, p.re, p.sb, p.se))
    u = np.unique(np.concatenate([rb, re, sb, se, _frame_index([p.lo, p.hi], step, n)]))
    cnt = np.diff(u)
    R, S = _active(rb, re, p.rs, p.n_ref, u), _active(sb, se, p.ss, p.n_sys, u)
    Rw = R.astype(np.int64) * cnt[:, None]
    rc, ref_classes = _classes(R, p.ref_names)
    sc, sys_classes = _classes(S, p.sys_names)
    cm = np.zeros((len(ref_classes), len(sys_classes)), dtype=np.int64)
    np.add.at(cm, (rc, sc), cnt)
    return _record(p, Rw.sum(axis=0), (S.astype(np.int64) * cnt[:, None]).sum(axis=0), Rw.T @ S.astype(np.int64), ref_classes,
                   sys_classes, cm)


def _pack(preps):
    """the arrays of vbx_frame_counts for prepared pairs: counts [n][4], extent [n][2], turns [.][2], speaker indices"""
    counts = np.array([[p.rb.size, p.sb.size, p.n_ref, p.n_sys] for p in preps], dtype=np.int32)
    extent = np.array([[p.lo, p.hi] for p in preps], dtype=np.float64)
    begins = np.concatenate([a for p in preps for a in (p.rb, p.sb)])
    ends = np.concatenate([a for p in preps for a in (p.re, p.se)])
    spk = np.concatenate([a for p in preps for a in (p.rs, p.ss)])
    return counts, extent, np.stack([begins, ends], axis=1), spk


def _device_counts(preps, step, device):
    """the integer records of the pairs the device takes; None for a pair with more classes than it returns"""
    from . import _capi
    info, classes, flat = _capi.frame_counts(_capi.default_context(device), *_pack(preps), step)
    out, off = [], 0
    for p, (_, ncr, ncs, _), masks in zip(preps, info.tolist(), classes):
        nr, ns = p.n_ref, p.n_sys
        ref_durs, sys_durs = flat[off:off + nr].copy(), flat[off + nr:off + nr + ns].copy()
        inter = flat[off + nr + ns:off + nr + ns + nr * ns].reshape(nr, ns).copy()
        off += nr + ns + nr * ns
        if ncr > MAX_DEVICE_CLASSES or ncs > MAX_DEVICE_CLASSES:
            out.append(None)
            continue
        cm = flat[off:off + ncr * ncs].reshape(ncr, ncs).copy()
        off += ncr * ncs
        names = [[tuple(n for i, n in enumerate(side) if int(m) >> i & 1) for m in masks[k, :count]]
                 for k, (side, count) in enumerate(((p.ref_names, ncr), (p.sys_names, ncs)))]
        out.append(_record(p, ref_durs, sys_durs, inter, names[0], names[1], cm))
    return out


def _check_step(step):
    step = float(step)
    if not step > 0.0 or step == float('inf'):
        raise ValueError(f'step must be a length > 0, not {step!r}')
    return step


def _frame_counts(preps, step, device):
    records = [None] * len(preps)
    if device is not None:
        on_dev = [k for k, p in enumerate(preps) if p.n_ref <= MAX_DEVICE_SPEAKERS and p.n_sys <= MAX_DEVICE_SPEAKERS
                  and p.hi / step < MAX_DEVICE_FRAMES]
        if on_dev:
            for k, rec in zip(on_dev, _device_counts([preps[k] for k in on_dev], step, int(device))):
                records[k] = rec
    for k, p in enumerate(preps):
        if records[k] is None:
            records[k] = _host_counts(p, step)
    return records


def frame_counts(pairs, step=0.010, device=None):
    """The integers behind the frame metrics of ``pairs`` = ``[(reference turns, system turns)]``, each side ``[(start, end,
    speaker)]`` of one recording.  -> per pair a dict: ``ref_speakers`` / ``sys_speakers`` (sorted names), ``ref_durs`` /
    ``sys_durs`` (frames per speaker, int64), ``inter`` (int64 [reference speakers][system speakers]: frames that hold both),
    ``ref_classes`` / ``sys_classes`` (tuples of speaker names, ``()`` is non-speech, in order of first appearance) and ``cm``
    (int64 [reference classes][system classes]).

    ``device=None``: in numpy.  ``device=N``: all pairs in one launch sequence on GPU N, a pair's numbers independent of the
    batch it is in.  A pair with more than 64 speakers or more than 256 classes on either side runs on the numpy route in
    either case.  Both routes count the same cells in integers: the records are equal bit for bit."""
    step = _check_step(step)
    return _frame_counts([_Frames(ref, hyp) for ref, hyp in pairs], step, device)


# ---- label sequences: many hypotheses per recording ---------------------------------------------------
class _LabelsFrames:
    """The reference's side of one recording for ``vbx_labels_frame_counts``, prepared once for all its label sequences:
    merged turns and speaker names.  ``ok``: the device takes the recording -- at most 64 reference speakers, segments of
    positive finite duration whose starts and ends both never decrease, fewer than 2^40 frames.  Then the turns of ANY label
    sequence form a chain and ``lo`` / ``hi`` of ``_Frames`` do not depend on the labels (``score._LabelsRef``)."""

    def __init__(self, ref_turns, starts, ends, step):
        ref = merge_turns(ref_turns, touching=False)
        self.ref_names = sorted({t[2] for t in ref}, key=str)
        ri = {s: i for i, s in enumerate(self.ref_names)}
        self.turns = np.array([t[:2] for t in ref], dtype=np.float64).reshape(-1, 2)
        self.rs = np.array([ri[t[2]] for t in ref], dtype=np.int32)
        s = self.starts = np.asarray(starts, dtype=np.float64).reshape(-1)
        e = self.ends = np.asarray(ends, dtype=np.float64).reshape(-1)
        self.ok = bool(s.size > 0 and s.size == e.size and len(self.ref_names) <= MAX_DEVICE_SPEAKERS and np.isfinite(s).all()
                       and np.isfinite(e).all() and np.isfinite(self.turns).all() and (s < e).all() and (s[1:] >= s[:-1]).all()
                       and (e[1:] >= e[:-1]).all())
        if self.ok:
            self.ok = max([e[-1]] + self.turns[:, 1].tolist()) / step < MAX_DEVICE_FRAMES


def _labels_host_counts(item, labels, step):
    return _host_counts(_Frames(item[0], _score.labels_turns(item[1], item[2], labels)), step)


def frame_counts_labels(items, step=0.010, device=None, timing=None):
    """The integers of ``frame_counts`` for label sequences: ``items`` = ``[(reference turns, starts, ends, [labels, ...])]``,
    the items of ``score.score_labels``.  -> per item a list with, per label sequence, the record ``frame_counts([(reference
    turns, score.labels_turns(starts, ends, labels))])`` gives; the system speakers are the integer labels that have a turn
    of positive duration.

    ``device=None``: that call, in numpy.  ``device=N``: ONE ``vbx_labels_frame_counts`` call for everything the device takes --
    the turns of every hypothesis are built on GPU N, the reference's side goes up and is cut into frames once per recording
    (vbx_labels_frame.hpp).  These run in numpy, item by item: more than 64 reference speakers or distinct labels, more than
    256 classes on a side, segment times that decrease, a segment without duration.  Both routes count the same cells in
    integers: the records are equal bit for bit.  ``timing``: a dict that receives the seconds of the host preparation, the
    device call and the mapping of what came back."""
    import time
    t0 = t1 = t2 = time.perf_counter()
    step = _check_step(step)
    out = [[None] * len(item[3]) for item in items]
    host = []                                                         # (item, hypothesis) for the numpy route
    if device is None:
        host = [(k, j) for k, item in enumerate(items) for j in range(len(item[3]))]
    else:
        from . import _capi
        refs, where, hyp, labs, names = [], [], [], [], []
        for k, (ref_turns, starts, ends, hyps) in enumerate(items):
            ref = _LabelsFrames(ref_turns, starts, ends, step) if len(hyps) else None
            taken = False
            for j, labels in enumerate(hyps):
                labels = np.asarray(labels).reshape(-1)
                uniq, inv = np.unique(labels, return_inverse=True)
                if not ref.ok or labels.size != ref.starts.size or uniq.size > MAX_DEVICE_SPEAKERS:
                    host.append((k, j))
                    continue
                order = sorted(range(uniq.size), key=lambda c: str(int(uniq[c])))      # the order of _Frames: by name as text
                rank = np.empty(uniq.size, dtype=np.int32)
                rank[order] = np.arange(uniq.size, dtype=np.int32)
                taken = True
                where.append((k, j))
                hyp.append((len(refs), uniq.size))
                labs.append(rank[inv.reshape(-1)])
                names.append([int(uniq[c]) for c in order])
            if taken:
                refs.append(ref)
        t1 = t2 = time.perf_counter()
        if where:
            info, classes, flat, masks = _capi.labels_frame_counts(
                _capi.default_context(int(device)), [(r.starts.size, r.rs.size, len(r.ref_names)) for r in refs],
                np.concatenate([a for r in refs for a in (r.starts, r.ends)]), np.concatenate([r.turns for r in refs]),
                np.concatenate([r.rs for r in refs]), hyp, np.concatenate(labs), step)
            t2 = time.perf_counter()
            off = 0
            for (k, j), (r, ns), lab_names, (_, ncr, ncs, _), cls, mask in zip(where, hyp, names, info.tolist(), classes, masks.tolist()):
                ref_names = refs[r].ref_names
                nr = len(ref_names)
                ref_durs, sys_durs = flat[off:off + nr].copy(), flat[off + nr:off + nr + ns]
                inter = flat[off + nr + ns:off + nr + ns + nr * ns].reshape(nr, ns)
                off += nr + ns + nr * ns
                if ncr > MAX_DEVICE_CLASSES or ncs > MAX_DEVICE_CLASSES:
                    host.append((k, j))                               # (the device returned no cm)
                    continue
                cm = flat[off:off + ncr * ncs].reshape(ncr, ncs).copy()
                off += ncr * ncs
                cols = [c for c in range(ns) if mask >> c & 1]        # a label whose only turns have no duration is no speaker
                out[k][j] = dict(ref_speakers=list(ref_names), sys_speakers=[lab_names[c] for c in cols], ref_durs=ref_durs,
                                 sys_durs=sys_durs[cols], inter=np.ascontiguousarray(inter[:, cols]),
                                 ref_classes=[tuple(n for i, n in enumerate(ref_names) if int(m) >> i & 1) for m in cls[0, :ncr]],
                                 sys_classes=[tuple(lab_names[c] for c in cols if int(m) >> c & 1) for m in cls[1, :ncs]], cm=cm)
    for k, j in host:
        out[k][j] = _labels_host_counts(items[k], items[k][3][j], step)
    if timing is not None:
        timing.update(prepare=t1 - t0, device=t2 - t1, mapping=time.perf_counter() - t2)
    return out


# ---- the floating-point columns, always here, from the integers -----------------------------------------------------------
def _jer(rec):
    """per reference speaker with a frame: its Jaccard error in [0, 1], as {name: error}"""
    from scipy.optimize import linear_sum_assignment
    rk, sk = np.flatnonzero(rec['ref_durs'] > 0), np.flatnonzero(rec['sys_durs'] > 0)
    per = np.ones(rk.size)
    if rk.size and sk.size:
        inter = rec['inter'][np.ix_(rk, sk)].astype(np.float64)
        union = rec['ref_durs'][rk].astype(np.float64)[:, None] + rec['sys_durs'][sk].astype(np.float64)[None, :] - inter
        J = 1.0 - inter / union
        rows, cols = linear_sum_assignment(J)
        per[rows] = J[rows, cols]
    return {rec['ref_speakers'][r]: float(v) for r, v in zip(rk, per)}, bool(sk.size)


def _jer_percent(errors, sys_speech):
    if not errors:
        return 100.0 if sys_speech else 0.0
    return 100.0 * float(np.mean(np.array(errors, dtype=np.float64)))


def _entropy(p):
    p = p[p > 0]
    return float(-np.sum(p * np.log2(p)))


def _clustering(cm):
    """the nine clustering columns of a contingency matrix (int64 [reference classes][system classes])"""
    N = int(cm.sum())
    if N == 0:
        return dict(b3_precision=1.0, b3_recall=1.0, b3_f1=1.0, gkt_ref_sys=1.0, gkt_sys_ref=1.0, h_ref_sys=0.0, h_sys_ref=0.0,
                    mi=0.0, nmi=1.0)
    keep_r, keep_c = cm.sum(axis=1) > 0, cm.sum(axis=0) > 0            # (a class has a frame; a block-diagonal sum too)
    cmf = cm[np.ix_(keep_r, keep_c)].astype(np.float64)
    row, col = cmf.sum(axis=1), cmf.sum(axis=0)
    precision = float(np.sum(cmf * cmf / col[None, :]) / N)
    recall = float(np.sum(cmf * cmf / row[:, None]) / N)
    p, pr, pc = cmf / N, row / N, col / N

    def gkt(py, p_given):                                             # (V(Y) - V(Y|X)) / V(Y)
        v = 1.0 - float(np.sum(py * py))
        return 1.0 if v == 0.0 else (v - (1.0 - float(np.sum(p_given)))) / v

    h_ref, h_sys = _entropy(pr), _entropy(pc)
    nz = p > 0
    h_ref_sys = float(-np.sum(p[nz] * np.log2((p / pc[None, :])[nz])))
    h_sys_ref = float(-np.sum(p[nz] * np.log2((p / pr[:, None])[nz])))
    mi = h_ref - h_ref_sys
    if h_ref == 0.0 or h_sys == 0.0:
        nmi = 1.0 if h_ref == 0.0 and h_sys == 0.0 else 0.0
    else:
        nmi = mi / math.sqrt(h_ref * h_sys)
    return dict(b3_precision=precision, b3_recall=recall, b3_f1=2.0 * precision * recall / (precision + recall),
                gkt_ref_sys=gkt(pc, p * p / pr[:, None]), gkt_sys_ref=gkt(pr, p * p / pc[None, :]), h_ref_sys=h_ref_sys,
                h_sys_ref=h_sys_ref, mi=mi, nmi=nmi)


def _extend(der_record, rec):
    errors, sys_speech = _jer(rec)
    out = dict(der_record)
    out.update(jer=_jer_percent(list(errors.values()), sys_speech), jer_speakers={k: 100.0 * v for k, v in errors.items()},
               sys_speech=sys_speech, **_clustering(rec['cm']))
    out.update((k, rec[k]) for k in ('ref_durs', 'sys_durs', 'inter', 'ref_classes', 'sys_classes', 'cm'))
    return out


def score_turns(pairs, collar=0.0, ignore_overlaps=False, step=0.010, device=None):
    """Score ``pairs`` = ``[(reference turns, system turns)]``.  -> per pair the record of ``vbx_amd.score.score_turns``
    (``der``, ``miss``, ``fa``, ``confusion``, ``ref_time``, ``C``, ``ref_speakers``, ``sys_speakers``, ``mapping``; ``collar``
    and ``ignore_overlaps`` act on these only) extended with ``jer`` (percent), ``jer_speakers`` {reference speaker with a
    frame: its Jaccard error in percent}, ``b3_precision``, ``b3_recall``, ``b3_f1``, ``gkt_ref_sys``, ``gkt_sys_ref``,
    ``h_ref_sys``, ``h_sys_ref``, ``mi``, ``nmi`` and the integers of ``frame_counts``: ``ref_durs``, ``sys_durs``, ``inter``,
    ``ref_classes``, ``sys_classes``, ``cm``."""
    step = _check_step(step)
    pairs = list(pairs)
    der = _score.score_turns(pairs, collar, ignore_overlaps, device)
    counts = _frame_counts([_Frames(ref, hyp) for ref, hyp in pairs], step, device)
    return [_extend(d, c) for d, c in zip(der, counts)]


def score_labels(items, collar=0.0, ignore_overlaps=False, step=0.010, device=None, timing=None):
    """Score label sequences: ``items`` = ``[(reference turns, starts, ends, [labels, ...])]``, the items of
    ``score.score_labels``.  -> per item a list with, per label sequence, exactly the record ``score_turns([(reference turns,
    score.labels_turns(starts, ends, labels))], collar, ignore_overlaps, step, device)`` returns.  The DER part is
    ``score.score_labels``, the integers are ``frame_counts_labels``: with ``device=N`` two device calls for all sequences of
    all recordings, the reference's side prepared once per recording in both.  The floating-point columns are computed here
    from the integers, as in ``score_turns``.  ``timing``: a dict that receives the seconds of the host preparation, the
    device calls and the mapping (``linear_sum_assignment``, the records, the columns; ``columns`` names the columns' share)."""
    import time
    step = _check_step(step)
    items = list(items)
    t_der, t_cnt = {}, {}
    der = _score.score_labels(items, collar, ignore_overlaps, device, timing=t_der)
    counts = frame_counts_labels(items, step, device, timing=t_cnt)
    t0 = time.perf_counter()
    out = [[_extend(d, c) for d, c in zip(ds, cs)] for ds, cs in zip(der, counts)]
    if timing is not None:
        columns = time.perf_counter() - t0
        timing.update(prepare=t_der['prepare'] + t_cnt['prepare'], device=t_der['device'] + t_cnt['device'],
                      mapping=t_der['mapping'] + t_cnt['mapping'] + columns, columns=columns)
    return out


def _overall(records):
    """OVERALL: DER pooled; JER over the reference speakers of all files; clustering columns of the block-diagonal cm"""
    out = _score._pool(records)
    errors = [v / 100.0 for r in records for v in r['jer_speakers'].values()]
    out['jer'] = _jer_percent(errors, any(r['sys_speech'] for r in records))
    cm = np.zeros((sum(r['cm'].shape[0] for r in records), sum(r['cm'].shape[1] for r in records)), dtype=np.int64)
    a = b = 0
    for r in records:
        cm[a:a + r['cm'].shape[0], b:b + r['cm'].shape[1]] = r['cm']
        a, b = a + r['cm'].shape[0], b + r['cm'].shape[1]
    out.update(cm=cm, **_clustering(cm))
    return out


def score_rttm(ref_paths, sys_paths, collar=0.0, ignore_overlaps=False, step=0.010, device=None):
    """Score the system RTTM files against the reference RTTM files (a path or a list of paths each; a file may hold
    several recordings).  -> ``({recording: record of score_turns}, overall)`` in the order of the sorted recording names.
    A recording of the reference without system turns is scored against nothing; a recording only the system has raises
    ``ValueError`` naming it."""
    ref, hyp = _score._read_all(ref_paths), _score._read_all(sys_paths)
    unknown = sorted(set(hyp) - set(ref))
    if unknown:
        raise ValueError('the system output holds recordings the reference does not: ' + ', '.join(unknown))
    names = sorted(ref)
    records = score_turns([(ref[n], hyp.get(n, [])) for n in names], collar, ignore_overlaps, step, device)
    return dict(zip(names, records)), _overall(records)


def format_table(records, overall):
    """dscore's table: the header, a dashed rule, one row per recording and ``*** OVERALL ***``; two decimals, numbers
    right-aligned, names left-aligned, two spaces between columns.  A column is as wide as its widest entry, a header
    counting two more than its length (the table package dscore prints with pads its headers so)."""
    def row(name, r):
        return [name] + ['nan' if math.isnan(r[k]) else f'{r[k]:.2f}' for k in COLUMNS]
    rows = [row(n, r) for n, r in records.items()] + [row('*** OVERALL ***', overall)]
    width = [max([len(h) + 2] + [len(r[c]) for r in rows]) for c, h in enumerate(HEADER)]
    lines = ['  '.join([r[0].ljust(width[0])] + [r[c].rjust(width[c]) for c in range(1, len(HEADER))]) for r in [HEADER] + rows]
    lines.insert(1, '  '.join('-' * w for w in width))
    return '\n'.join(lines)


def build_parser():
    p = argparse.ArgumentParser(prog='python -m vbx_amd.metrics', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('-r', dest='ref_rttm_fns', nargs='+', required=True, metavar='REF', help='reference RTTM files')
    p.add_argument('-s', dest='sys_rttm_fns', nargs='+', required=True, metavar='SYS', help='system RTTM files')
    p.add_argument('-u', '--uem', dest='uemf', default=None, metavar='UEM', help='not supported: the scored extent is the extent of the turns')
    p.add_argument('--collar', type=float, default=0.0, metavar='DUR',
                   help='DER column: no-score zone of +-DUR seconds round every reference turn boundary (default: %(default)s)')
    p.add_argument('--ignore_overlaps', action='store_true', help='DER column: do not score where two or more reference speakers speak')
    p.add_argument('--step', type=float, default=0.010, metavar='DUR', help='frame step of the other columns in seconds (default: %(default)s)')
    p.add_argument('--device', type=int, default=None, metavar='N', help='count on GPU N (default: in numpy on the host)')
    return p


def main(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if args.uemf is not None:
        p.error('-u/--uem is not supported: the scored extent of a recording runs from its first turn start to its last '
                'turn end (reference and system)')
    if not args.collar >= 0.0:
        p.error('--collar must be >= 0')
    if not args.step > 0.0:
        p.error('--step must be > 0')
    try:
        records, overall = score_rttm(args.ref_rttm_fns, args.sys_rttm_fns, args.collar, args.ignore_overlaps, args.step, args.device)
    except (ValueError, OSError) as exc:
        p.error(str(exc))
    print(format_table(records, overall))
    return 0


if __name__ == '__main__':
    sys.exit(main())
