"""An exact referee for ``vbx_amd.score``: md-eval's DER of one recording in rational arithmetic.

Times are ``fractions.Fraction`` of what the caller passes -- the decimal text of an RTTM file, or a float's exact binary
value -- so no sum here rounds.  (All of a recording's times are brought to their common denominator first; the sums then run
on Python integers, which is the same exact arithmetic, only quicker.)  Shares no code with ``vbx_amd/score.py`` and works
differently: the active speakers of a cell come from a bisection of every speaker's own sorted turns, the collar test from the
nearest reference boundary, where the product compares every cell with every turn.

Semantics (dscore / md-eval): turns of no duration dropped; turns of one speaker that overlap merged
(turns that only touch keep their boundary, and its collar); extent = [smallest start, largest end] over both sides; not
scored: within ``collar`` (strictly) of a reference turn start or end, and, with ``ignore_overlaps``, where two or more
reference speakers speak; cells between consecutive distinct boundaries, decided at their midpoints.
"""
import bisect
import itertools
import math
from fractions import Fraction


def read_rttm_exact(path):
    """{recording: [(start, end, speaker)]} with Fraction times from the decimal text: end = start + duration, exactly."""
    out = {}
    for line in open(path):
        f = line.split()
        if f and f[0] == 'SPEAKER':
            start, dur = Fraction(f[3]), Fraction(f[4])
            out.setdefault(f[1], []).append((start, start + dur, f[7]))
    return out


def _merged(turns):
    """{speaker: [(begin, end)]} sorted, strictly overlapping turns of a speaker merged."""
    by = {}
    for b, e, s in turns:
        b, e = Fraction(b), Fraction(e)
        if e > b:
            by.setdefault(s, []).append((b, e))
    for s, ts in by.items():
        ts.sort()
        keep = [list(ts[0])]
        for b, e in ts[1:]:
            if b < keep[-1][1]:
                keep[-1][1] = max(keep[-1][1], e)
            else:
                keep.append([b, e])
        by[s] = [tuple(t) for t in keep]
    return by


def _best_mapping(C, nr, ns):
    """max over one-to-one mappings of sum C[r][s], exactly (C: integers)."""
    if min(nr, ns) == 0:
        return 0
    if nr <= 5 and ns <= 5:                                   # every mapping
        small, big, get = (nr, ns, lambda a, b: C[a][b]) if nr <= ns else (ns, nr, lambda a, b: C[b][a])
        return max(sum(get(a, b) for a, b in zip(range(small), perm)) for perm in itertools.permutations(range(big), small))
    import numpy as np
    from scipy.optimize import linear_sum_assignment
    assert max(max(row) for row in C) < 2 ** 52                # exact as float64: the optimum found is an exact optimum
    rows, cols = linear_sum_assignment(np.array(C, dtype=np.float64), maximize=True)
    return sum(C[r][s] for r, s in zip(rows, cols))


def score_exact(ref_turns, sys_turns, collar=0, ignore_overlaps=False):
    """-> dict of Fractions: ref_time, miss, fa, both, confusion, C {(ref speaker, sys speaker): seconds}, scored (the scored
    length, sum of w), der (percent, None where ref_time is 0), and n_cells."""
    collar = Fraction(collar)
    ref, hyp = _merged(ref_turns), _merged(sys_turns)
    all_turns = [t for side in (ref, hyp) for ts in side.values() for t in ts]
    zero = dict(ref_time=Fraction(0), miss=Fraction(0), fa=Fraction(0), both=Fraction(0), confusion=Fraction(0), C={},
                scored=Fraction(0), der=None, n_cells=0)
    if not all_turns:
        return zero
    den = 1
    for v in [collar] + [x for t in all_turns for x in t]:
        den = den * v.denominator // math.gcd(den, v.denominator)
    unit = 2 * den                                             # midpoints are integers in units of 1 / unit
    I = lambda v: int(v * unit)
    k = I(collar)
    lo, hi = min(I(t[0]) for t in all_turns), max(I(t[1]) for t in all_turns)
    ref_i = {s: ([I(b) for b, _ in ts], [I(e) for _, e in ts]) for s, ts in ref.items()}
    hyp_i = {s: ([I(b) for b, _ in ts], [I(e) for _, e in ts]) for s, ts in hyp.items()}
    ref_bounds = sorted({x for bs, es in ref_i.values() for x in bs + es})
    points = {lo, hi} | {I(x) for t in all_turns for x in t}
    if k > 0:
        points |= {min(max(b + d, lo), hi) for b in ref_bounds for d in (-k, k)}
    edges = sorted(points)
    rn, sn = sorted(ref_i, key=str), sorted(hyp_i, key=str)
    C = [[0] * len(sn) for _ in rn]
    ref_time = miss = fa = both = scored = 0
    for a, b in zip(edges, edges[1:]):
        m2 = a + b                                             # twice the midpoint: compare with twice the bounds
        R = [i for i, s in enumerate(rn) if _active(ref_i[s], m2)]
        S = [j for j, s in enumerate(sn) if _active(hyp_i[s], m2)]
        noscore = False
        if k > 0:
            j = bisect.bisect_left(ref_bounds, (m2 + 1) // 2)
            for q in (j - 1, j):
                if 0 <= q < len(ref_bounds) and abs(m2 - 2 * ref_bounds[q]) < 2 * k:
                    noscore = True
        if ignore_overlaps and len(R) >= 2:
            noscore = True
        if noscore:
            continue
        w = b - a
        scored += w
        ref_time += w * len(R)
        miss += w * max(len(R) - len(S), 0)
        fa += w * max(len(S) - len(R), 0)
        both += w * min(len(R), len(S))
        for i in R:
            for j in S:
                C[i][j] += w
    F = lambda v: Fraction(v, unit)
    confusion = both - _best_mapping(C, len(rn), len(sn))
    return dict(ref_time=F(ref_time), miss=F(miss), fa=F(fa), both=F(both), confusion=F(confusion), scored=F(scored),
                C={(r, s): F(C[i][j]) for i, r in enumerate(rn) for j, s in enumerate(sn)},
                der=Fraction(100 * (miss + fa + confusion), ref_time) if ref_time else None, n_cells=len(edges) - 1)


def _active(turns, m2):
    """is the point m2 / 2 strictly inside one of the sorted turns (begins, ends)?"""
    begins, ends = turns
    i = bisect.bisect_left(begins, (m2 + 1) // 2) - 1          # the last turn with 2 begin < m2
    return i >= 0 and 2 * begins[i] < m2 < 2 * ends[i]
