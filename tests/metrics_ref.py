"""Dense referee of ``vbx_amd.metrics``, written apart from it: one boolean row per frame.

The formulation that reproduced the row the reference's README publishes for ES2005a: the frame times are
``step * np.arange(n)`` with ``n = int(hi / step)``, a turn ``[b, e)`` sets the rows ``searchsorted(times, b) ...
searchsorted(times, e)`` of its speaker's column, the rows with ``lo <= time < hi`` are kept, and the classes are
``np.unique`` of the rows.  Nothing here knows of cells, masks or frame indices corrected by a product.

Rows below ``int(lo / step) - 2`` are never built: their times lie below ``lo``, no turn starts there and none is kept, so
leaving them out changes no count (and a recording that starts at 1e5 s stays small).
"""
import math

import numpy as np


def _side(turns, names, times):
    rows = np.zeros((times.size, len(names)), dtype=bool)
    col = {s: i for i, s in enumerate(names)}
    for b, e, s in turns:
        rows[np.searchsorted(times, b, side='left'):np.searchsorted(times, e, side='left'), col[s]] = True
    return rows


def _classes(rows, names):
    if rows.shape[0] == 0:
        return np.zeros(0, dtype=np.int64), []
    packed = np.packbits(np.concatenate([rows, np.zeros((rows.shape[0], 1), dtype=bool)], axis=1), axis=1)
    _, first, inverse = np.unique(packed, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    by_appearance = sorted(range(first.size), key=lambda k: first[k])
    number = {k: a for a, k in enumerate(by_appearance)}
    cls = np.array([number[k] for k in range(first.size)], dtype=np.int64)[inverse]
    return cls, [tuple(names[i] for i in range(len(names)) if rows[first[k], i]) for k in by_appearance]


def counts(ref, hyp, step=0.010):
    """the integer record of one pair: the keys of ``metrics.frame_counts``"""
    ref = [(float(b), float(e), s) for b, e, s in ref if e > b]
    hyp = [(float(b), float(e), s) for b, e, s in hyp if e > b]
    ref_names, sys_names = sorted({t[2] for t in ref}, key=str), sorted({t[2] for t in hyp}, key=str)
    if ref or hyp:
        lo, hi = min(t[0] for t in ref + hyp), max(t[1] for t in ref + hyp)
        n = int(hi / step) if hi > 0 else 0
        times = step * np.arange(max(0, int(lo / step) - 2) if lo > 0 else 0, n)
        keep = (times >= lo) & (times < hi)
    else:
        times, keep = np.zeros(0), np.zeros(0, dtype=bool)
    R, S = _side(ref, ref_names, times)[keep], _side(hyp, sys_names, times)[keep]
    rc, ref_classes = _classes(R, ref_names)
    sc, sys_classes = _classes(S, sys_names)
    cm = np.zeros((len(ref_classes), len(sys_classes)), dtype=np.int64)
    np.add.at(cm, (rc, sc), 1)                                        # one frame at a time
    return dict(ref_speakers=ref_names, sys_speakers=sys_names, ref_durs=R.sum(axis=0).astype(np.int64),
                sys_durs=S.sum(axis=0).astype(np.int64), inter=R.T.astype(np.int64) @ S.astype(np.int64), ref_classes=ref_classes,
                sys_classes=sys_classes, cm=cm)


def assert_counts_equal(got, want, what=''):
    for k in ('ref_speakers', 'sys_speakers', 'ref_classes', 'sys_classes'):
        assert list(got[k]) == list(want[k]), (what, k, got[k], want[k])
    for k in ('ref_durs', 'sys_durs', 'inter', 'cm'):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b), (what, k, a, b)


def columns(rec):
    """the ten frame columns from the integers of ``counts``, in plain loops over Python floats"""
    from scipy.optimize import linear_sum_assignment
    rd = [int(v) for v in rec['ref_durs'] if v > 0]
    sd = [int(v) for v in rec['sys_durs'] if v > 0]
    inter = [[int(rec['inter'][r, s]) for s in range(len(rec['sys_durs'])) if rec['sys_durs'][s] > 0]
             for r in range(len(rec['ref_durs'])) if rec['ref_durs'][r] > 0]
    if not rd:
        jer = 100.0 if sd else 0.0
    else:
        per = [1.0] * len(rd)
        if sd:
            J = np.array([[1.0 - inter[r][s] / (rd[r] + sd[s] - inter[r][s]) for s in range(len(sd))] for r in range(len(rd))])
            for r, s in zip(*linear_sum_assignment(J)):
                per[r] = float(J[r, s])
        jer = 100.0 * sum(per) / len(per)
    cm = [[int(v) for v in row] for row in rec['cm'].tolist()]
    N = sum(sum(row) for row in cm)
    if N == 0:
        return dict(jer=jer, b3_precision=1.0, b3_recall=1.0, b3_f1=1.0, gkt_ref_sys=1.0, gkt_sys_ref=1.0, h_ref_sys=0.0,
                    h_sys_ref=0.0, mi=0.0, nmi=1.0)
    rows, cols = [sum(row) for row in cm], [sum(row[b] for row in cm) for b in range(len(cm[0]))]
    cells = [(a, b, cm[a][b]) for a in range(len(rows)) for b in range(len(cols)) if cm[a][b] > 0]
    precision = sum(v * v / cols[b] for a, b, v in cells) / N
    recall = sum(v * v / rows[a] for a, b, v in cells) / N
    v_ref, v_sys = 1.0 - sum((x / N) ** 2 for x in rows), 1.0 - sum((x / N) ** 2 for x in cols)
    v_sys_ref = 1.0 - sum((v / N) ** 2 / (rows[a] / N) for a, b, v in cells)
    v_ref_sys = 1.0 - sum((v / N) ** 2 / (cols[b] / N) for a, b, v in cells)
    h_ref = -sum(x / N * math.log2(x / N) for x in rows if x > 0)
    h_sys = -sum(x / N * math.log2(x / N) for x in cols if x > 0)
    h_ref_sys = -sum(v / N * math.log2((v / N) / (cols[b] / N)) for a, b, v in cells)
    h_sys_ref = -sum(v / N * math.log2((v / N) / (rows[a] / N)) for a, b, v in cells)
    mi = h_ref - h_ref_sys
    if h_ref == 0.0 or h_sys == 0.0:
        nmi = 1.0 if h_ref == 0.0 and h_sys == 0.0 else 0.0
    else:
        nmi = mi / math.sqrt(h_ref * h_sys)
    return dict(jer=jer, b3_precision=precision, b3_recall=recall, b3_f1=2.0 * precision * recall / (precision + recall),
                gkt_ref_sys=1.0 if v_sys == 0.0 else (v_sys - v_sys_ref) / v_sys,
                gkt_sys_ref=1.0 if v_ref == 0.0 else (v_ref - v_ref_sys) / v_ref, h_ref_sys=h_ref_sys, h_sys_ref=h_sys_ref, mi=mi,
                nmi=nmi)
