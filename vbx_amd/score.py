#!/usr/bin/env python
"""python -m vbx_amd.score: diarization error rate of system RTTM files against reference RTTM files.

    python -m vbx_amd.score -r ref.rttm -s sys.rttm --collar 0.25 [--ignore_overlaps] [--device 0]

The last step of the reference's recipes (run_example.sh:40: ``dscore/score.py -r ... -s ... --collar 0.25
[--ignore_overlaps]``) with the program name swapped: the flags are dscore's, the DER is md-eval's -- time-weighted, with
no-score collars round every reference turn boundary, an optional exclusion of overlapped reference speech and overlapping
reference speakers counted once each.  DER ONLY: the table has the columns File, DER, Miss, FA, Conf (percent of the scored
reference speaker time) and an ``*** OVERALL ***`` row that pools the times of all files; dscore's JER, B-cubed and
information-theoretic columns are not computed, and there is no UEM file: the scored extent of a recording runs from its
first turn start to its last turn end, reference and system together (``-u`` is refused).

Per recording: turns of one speaker that overlap are merged, turns without duration dropped.  Turns of one speaker that only
touch keep their common boundary and with it its collar, as in dscore (which merges with intervaltree's strict overlap
test): the published DER 7.06 of the reference's example (ES2005a, README) is reproduced only so.  The sorted distinct
turn boundaries, collar zone ends ``b -+ collar`` and extent ends cut the extent into cells; in a cell the active reference
speakers R, the active system speakers S and the no-score flag are constant (decided at the midpoint, strict comparisons),
its weight w is its length, or 0 where it is not scored.  Then

    C[r][s] = sum w [r in R][s in S]     ref_time = sum w |R|        both = sum w min(|R|, |S|)
    miss = sum w max(|R| - |S|, 0)       fa = sum w max(|S| - |R|, 0)
    confusion = both - (C summed over the best one-to-one speaker mapping)      DER = 100 (miss + fa + confusion) / ref_time

The sums run on the device for any number of (recording, hypothesis) pairs in one launch (``device=N``; vbx_rttm_score.hpp)
or in numpy (``device=None``); the mapping is ``scipy.optimize.linear_sum_assignment`` on the host either way.

As a library: ``read_turns``, ``merge_turns``, ``score_turns``, ``score_rttm``, ``format_table``.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

__all__ = ['read_turns', 'merge_turns', 'score_turns', 'score_labels', 'labels_turns', 'score_rttm', 'score_written', 'format_table', 'build_parser', 'main']

MAX_DEVICE_SPEAKERS = 64      # speakers per side the device path takes (vbx_rttm_score.hpp: kRttmMaxSpk)


def read_turns(path, durations=False):
    """``{recording: [(start, end, speaker)]}`` of the SPEAKER lines of an RTTM file, in file order; ``end`` is
    ``start + duration`` in float64.  Other line types and blank lines are skipped.  ``durations``: the entries are
    ``(start, end, speaker, duration)``, the duration as the file gives it."""
    out = {}
    with open(path) as fp:
        for n, line in enumerate(fp, 1):
            f = line.split()
            if not f or f[0] != 'SPEAKER':
                continue
            if len(f) < 8:
                raise ValueError(f'{path}:{n}: a SPEAKER line has at least 8 fields')
            start, dur = float(f[3]), float(f[4])
            out.setdefault(f[1], []).append((start, start + dur, f[7], dur) if durations else (start, start + dur, f[7]))
    return out


def merge_turns(turns, touching=True):
    """The turns ``[(start, end, speaker)]`` with those of no or negative duration dropped and those of one speaker that
    overlap or touch merged; sorted by (start, speaker).  ``touching=False`` merges only turns that share more than an
    instant: what the scorer does, because dscore does (see ``score_turns``)."""
    by_spk = {}
    for start, end, spk in turns:
        if end > start:
            by_spk.setdefault(spk, []).append((float(start), float(end)))
    out = []
    for spk, ts in by_spk.items():
        ts.sort()
        cur_b, cur_e = ts[0]
        for b, e in ts[1:]:
            if b < cur_e or (touching and b == cur_e):
                cur_e = max(cur_e, e)
            else:
                out.append((cur_b, cur_e, spk))
                cur_b, cur_e = b, e
        out.append((cur_b, cur_e, spk))
    out.sort(key=lambda t: (t[0], str(t[2])))
    return out


class _Pair:
    """One recording ready for either path: merged turns as arrays, speaker names, cell edges."""

    def __init__(self, ref_turns, sys_turns, collar):
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
        vals = [self.rb, self.re, self.sb, self.se]
        if vals[0].size + vals[2].size == 0:
            self.edges = np.zeros(0)
            return
        if collar > 0:
            vals += [self.rb - collar, self.rb + collar, self.re - collar, self.re + collar]
        lo = min(a.min() for a in (self.rb, self.sb) if a.size)
        hi = max(a.max() for a in (self.re, self.se) if a.size)
        self.edges = np.unique(np.clip(np.concatenate(vals), lo, hi))          # (lo and hi are among the values)

    @property
    def n_ref(self):
        return len(self.ref_names)

    @property
    def n_sys(self):
        return len(self.sys_names)


def _host_totals(p, collar, ignore_overlaps, block=4096):
    """(ref_time, miss, fa, both), C [n_ref][n_sys] of one pair in numpy: the cells of the device path."""
    tot = np.zeros(4)
    C = np.zeros((p.n_ref, p.n_sys))
    ref_hot = np.eye(max(p.n_ref, 1))[:, :p.n_ref][p.rs] if p.rs.size else np.zeros((0, p.n_ref))
    sys_hot = np.eye(max(p.n_sys, 1))[:, :p.n_sys][p.ss] if p.ss.size else np.zeros((0, p.n_sys))
    for c0 in range(0, max(p.edges.size - 1, 0), block):
        a, b = p.edges[c0:c0 + block + 1][:-1], p.edges[c0:c0 + block + 1][1:]
        mid = (0.5 * (a + b))[:, None]
        R = ((p.rb < mid) & (mid < p.re)).astype(np.float64) @ ref_hot > 0
        S = ((p.sb < mid) & (mid < p.se)).astype(np.float64) @ sys_hot > 0
        noscore = np.zeros(a.size, dtype=bool)
        if collar > 0:
            noscore |= (((p.rb - collar < mid) & (mid < p.rb + collar)) | ((p.re - collar < mid) & (mid < p.re + collar))).any(1)
        nr, ns = R.sum(1), S.sum(1)
        if ignore_overlaps:
            noscore |= nr >= 2
        w = np.where(noscore, 0.0, b - a)
        tot += [np.sum(w * nr), np.sum(w * np.maximum(nr - ns, 0)), np.sum(w * np.maximum(ns - nr, 0)), np.sum(w * np.minimum(nr, ns))]
        C += (R * w[:, None]).T @ S.astype(np.float64)
    return tot, C


def _pack(pairs):
    """the arrays of vbx_rttm_score for prepared pairs: counts [n][5], edges, turns [.][2], speaker indices"""
    counts = np.array([[p.edges.size, p.rb.size, p.sb.size, p.n_ref, p.n_sys] for p in pairs], dtype=np.int32)
    edges = np.concatenate([p.edges for p in pairs])
    begins = np.concatenate([a for p in pairs for a in (p.rb, p.sb)])
    ends = np.concatenate([a for p in pairs for a in (p.re, p.se)])
    spk = np.concatenate([a for p in pairs for a in (p.rs, p.ss)])
    return counts, edges, np.stack([begins, ends], axis=1), spk


def _device_totals(pairs, collar, ignore_overlaps, device):
    from . import _capi
    flat = _capi.rttm_score(_capi.default_context(device), *_pack(pairs), collar, ignore_overlaps)
    out, off = [], 0
    for p in pairs:
        n = p.n_ref * p.n_sys
        out.append((flat[off:off + 4].copy(), flat[off + 4:off + 4 + n].reshape(p.n_ref, p.n_sys).copy()))
        off += 4 + n
    return out


def _record(p, tot, C):
    from scipy.optimize import linear_sum_assignment
    ref_time, miss, fa, both = (float(v) for v in tot)
    mapping, mapped = {}, 0.0
    if C.size:
        rows, cols = linear_sum_assignment(C, maximize=True)
        for r, s in zip(rows, cols):
            if C[r, s] > 0:
                mapping[p.ref_names[r]] = p.sys_names[s]
                mapped += float(C[r, s])
    confusion = both - mapped
    der = 100.0 * (miss + fa + confusion) / ref_time if ref_time > 0 else float('nan')
    return dict(der=der, miss=miss, fa=fa, confusion=confusion, ref_time=ref_time, C=C, ref_speakers=list(p.ref_names),
                sys_speakers=list(p.sys_names), mapping=mapping)


def score_turns(pairs, collar=0.0, ignore_overlaps=False, device=None):
    """Score ``pairs`` = ``[(reference turns, system turns)]``, each side ``[(start, end, speaker)]`` of one recording.

    -> per pair a dict: ``der`` (percent; nan where no reference speech is scored), ``miss``, ``fa``, ``confusion``,
    ``ref_time`` (seconds), ``C`` (the confusion matrix, seconds, [reference speakers][system speakers]) with
    ``ref_speakers`` / ``sys_speakers`` (its row and column names, sorted) and ``mapping`` {reference speaker: system
    speaker} (pairs that share no scored time are unmapped).

    ``device=None``: the sums run in numpy.  ``device=N``: all pairs in one launch on GPU N, a pair's numbers independent of
    the batch it is in.  A pair with more than 64 speakers on either side runs on the numpy path in either case (the device
    masks are 64 bits wide).  Both paths cut the same cells; they add them in different orders.

    Turns are merged by ``merge_turns(., touching=False)``: two turns of one speaker that merely touch are one stretch of
    speech for every sum, but their common boundary keeps its collar (dscore's behaviour, see the module text)."""
    collar = float(collar)
    if not collar >= 0.0 or collar == float('inf'):
        raise ValueError(f'collar must be a length >= 0, not {collar!r}')
    preps = [_Pair(ref, hyp, collar) for ref, hyp in pairs]
    totals = [None] * len(preps)
    if device is not None:
        on_dev = [k for k, p in enumerate(preps) if p.n_ref <= MAX_DEVICE_SPEAKERS and p.n_sys <= MAX_DEVICE_SPEAKERS]
        if on_dev:
            for k, t in zip(on_dev, _device_totals([preps[k] for k in on_dev], collar, ignore_overlaps, int(device))):
                totals[k] = t
    for k, p in enumerate(preps):
        if totals[k] is None:
            totals[k] = _host_totals(p, collar, ignore_overlaps)
    return [_record(p, *t) for p, t in zip(preps, totals)]


def labels_turns(starts, ends, labels):
    """The system turns ``[(start, end, label)]`` of one label per segment: ``vbhmm.merge_adjacent_labels``, what the RTTM
    writer is given (labels as Python ints)."""
    from .vbhmm import merge_adjacent_labels
    if len(labels) == 0:
        return []
    s, e, l = merge_adjacent_labels(np.asarray(starts, dtype=np.float64), np.asarray(ends, dtype=np.float64), np.asarray(labels))
    return [(float(a), float(b), int(c)) for a, b, c in zip(s, e, l)]


class _LabelsRef:
    """The reference's side of one recording for ``vbx_labels_score``, prepared once for all its label sequences: merged
    turns, speaker names, and its part of the cell edges.  ``ok``: the device takes the recording -- at most 64 reference
    speakers, segments of positive finite duration whose starts and ends both never decrease.  Then the turns of ANY label
    sequence form a chain, their extent is [starts[0], ends[-1]], and ``lo`` / ``hi`` of ``_Pair`` do not depend on the labels."""

    def __init__(self, ref_turns, starts, ends, collar):
        ref = merge_turns(ref_turns, touching=False)
        self.ref_names = sorted({t[2] for t in ref}, key=str)
        ri = {s: i for i, s in enumerate(self.ref_names)}
        self.rb = np.array([t[0] for t in ref], dtype=np.float64)
        self.re = np.array([t[1] for t in ref], dtype=np.float64)
        self.rs = np.array([ri[t[2]] for t in ref], dtype=np.int32)
        self.starts, self.ends = np.asarray(starts, dtype=np.float64).reshape(-1), np.asarray(ends, dtype=np.float64).reshape(-1)
        s, e = self.starts, self.ends
        self.ok = bool(s.size > 0 and s.size == e.size and len(self.ref_names) <= MAX_DEVICE_SPEAKERS and np.isfinite(s).all()
                       and np.isfinite(e).all() and (s < e).all() and (s[1:] >= s[:-1]).all() and (e[1:] >= e[:-1]).all())
        if not self.ok:
            return
        lo, hi = min([s[0]] + self.rb[:1].tolist()), max([e[-1], self.re.max()] if self.re.size else [e[-1]])    # (rb is sorted)
        vals = [self.rb, self.re, np.array([lo, hi])]
        if collar > 0:
            vals += [self.rb - collar, self.rb + collar, self.re - collar, self.re + collar]
        self.edges = np.unique(np.clip(np.concatenate(vals), lo, hi))


class _Names:
    def __init__(self, ref_names, sys_names):
        self.ref_names, self.sys_names = ref_names, sys_names


def score_labels(items, collar=0.0, ignore_overlaps=False, device=None, timing=None):
    """Score label sequences: ``items`` = ``[(reference turns, starts, ends, [labels, ...])]``, one entry per recording with the
    times of its segments and any number of hypotheses, each one integer label per segment.  -> per item a list with one
    record of ``score_turns`` per label sequence; the system speakers are the integer labels that have a turn.

    ``device=None`` is ``score_turns([(reference turns, labels_turns(starts, ends, labels))], ..., device=None)``.
    ``device=N``: the turns (``vbhmm.merge_adjacent_labels``) and the cell edges of every hypothesis are built on GPU N and the
    reference's side is prepared once per recording (vbx_labels_score.hpp); the numbers are those of
    ``score_turns(..., device=N)`` on the same turns.  What the device does not take runs on the numpy route: a recording with
    more than 64 reference speakers or with segment times that decrease or have no duration, a hypothesis with more than 64
    different labels.  ``timing``: a dict that receives the seconds of the host preparation, the device call and the mapping."""
    import time
    t0 = t1 = t2 = time.perf_counter()
    collar = float(collar)
    if not collar >= 0.0 or collar == float('inf'):
        raise ValueError(f'collar must be a length >= 0, not {collar!r}')
    out = [[None] * len(item[3]) for item in items]
    host = []                                                         # (item, hypothesis) for the numpy route
    if device is None:
        host = [(k, j) for k, item in enumerate(items) for j in range(len(item[3]))]
    else:
        from . import _capi
        refs, where, hyp, labs, names = [], [], [], [], []
        for k, (ref_turns, starts, ends, hyps) in enumerate(items):
            ref = _LabelsRef(ref_turns, starts, ends, collar) if len(hyps) else None
            taken = False
            for j, labels in enumerate(hyps):
                labels = np.asarray(labels).reshape(-1)
                uniq, inv = np.unique(labels, return_inverse=True)
                if not ref.ok or labels.size != ref.starts.size or uniq.size > MAX_DEVICE_SPEAKERS:
                    host.append((k, j))
                    continue
                taken = True
                where.append((k, j))
                hyp.append((len(refs), uniq.size))
                labs.append(inv.astype(np.int32))
                names.append([int(u) for u in uniq])
            if taken:
                refs.append(ref)
        t1 = t2 = time.perf_counter()
        if where:
            rec_counts = [(r.starts.size, r.rb.size, len(r.ref_names), r.edges.size) for r in refs]
            flat, info = _capi.labels_score(
                _capi.default_context(int(device)), rec_counts, np.concatenate([a for r in refs for a in (r.starts, r.ends)]),
                np.concatenate([np.stack([r.rb, r.re], axis=1) for r in refs]), np.concatenate([r.rs for r in refs]),
                np.concatenate([r.edges for r in refs]), hyp, np.concatenate(labs), collar, ignore_overlaps)
            t2 = time.perf_counter()
            off = 0
            for (k, j), (r, n_sys), lab_names, inf in zip(where, hyp, names, info):
                ref, n_ref = refs[r], len(refs[r].ref_names)
                tot = flat[off:off + 4].copy()
                C = flat[off + 4:off + 4 + n_ref * n_sys].reshape(n_ref, n_sys)
                off += 4 + n_ref * n_sys
                mask = (int(inf[3]) & 0xffffffff) << 32 | (int(inf[2]) & 0xffffffff)
                cols = sorted((c for c in range(n_sys) if mask >> c & 1), key=lambda c: str(lab_names[c]))     # the order of _Pair
                out[k][j] = _record(_Names(ref.ref_names, [lab_names[c] for c in cols]), tot, np.ascontiguousarray(C[:, cols]))
    if host:
        records = score_turns([(items[k][0], labels_turns(items[k][1], items[k][2], items[k][3][j])) for k, j in host], collar,
                              ignore_overlaps, None)
        for (k, j), rec in zip(host, records):
            out[k][j] = rec
    if timing is not None:
        timing.update(prepare=t1 - t0, device=t2 - t1, mapping=time.perf_counter() - t2)
    return out


def _pool(records):
    """OVERALL: the error times and the reference time pooled over the recordings (not the mean of their rates)."""
    keep = [r for r in records if r['ref_time'] > 0]
    miss, fa, conf, ref = (float(sum(r[k] for r in keep)) for k in ('miss', 'fa', 'confusion', 'ref_time'))
    return dict(der=100.0 * (miss + fa + conf) / ref if ref > 0 else float('nan'), miss=miss, fa=fa, confusion=conf, ref_time=ref)


def _read_all(paths):
    out = {}
    for path in ([paths] if isinstance(paths, (str, os.PathLike)) else paths):
        for rec, turns in read_turns(path).items():
            out.setdefault(rec, []).extend(turns)
    return out


def score_rttm(ref_paths, sys_paths, collar=0.0, ignore_overlaps=False, device=None):
    """Score the system RTTM files against the reference RTTM files (a path or a list of paths each; a file may hold
    several recordings).  -> ``({recording: record of score_turns}, overall)`` in the order of the sorted recording names;
    ``overall`` pools miss, fa, confusion and ref_time over the recordings.  A recording of the reference without system
    turns is all miss; a recording only the system has raises ``ValueError`` naming it."""
    ref, hyp = _read_all(ref_paths), _read_all(sys_paths)
    unknown = sorted(set(hyp) - set(ref))
    if unknown:
        raise ValueError('the system output holds recordings the reference does not: ' + ', '.join(unknown))
    names = sorted(ref)
    records = score_turns([(ref[n], hyp.get(n, [])) for n in names], collar, ignore_overlaps, device)
    by_name = dict(zip(names, records))
    return by_name, _pool(records)


def score_written(out_rttm_dir, names, ref_rttm_dir, collar=0.25, ignore_overlaps=False, device=None):
    """What the drivers do with ``--ref-rttm-dir``: the files ``out_rttm_dir/<name>.rttm`` as written (their text parsed
    back, so that ``python -m vbx_amd.score`` on them gives the same bits) against ``ref_rttm_dir/<name>.rttm``."""
    names = list(names)
    if not names:
        return {}, _pool([])
    return score_rttm([os.path.join(ref_rttm_dir, f'{n}.rttm') for n in names],
                      [os.path.join(out_rttm_dir, f'{n}.rttm') for n in names], collar, ignore_overlaps, device)


def format_table(records, overall):
    """The table ``python -m vbx_amd.score`` prints: File, DER, Miss, FA, Conf in percent of the scored reference time."""
    def row(name, r):
        if not r['ref_time'] > 0:
            return [name] + ['nan'] * 4
        return [name, f"{r['der']:.2f}"] + [f"{100.0 * r[k] / r['ref_time']:.2f}" for k in ('miss', 'fa', 'confusion')]
    rows = [['File', 'DER', 'Miss', 'FA', 'Conf']] + [row(n, r) for n, r in records.items()] + [row('*** OVERALL ***', overall)]
    width = [max(len(r[c]) for r in rows) for c in range(5)]
    lines = ['  '.join([r[0].ljust(width[0])] + [r[c].rjust(width[c]) for c in range(1, 5)]) for r in rows]
    lines.insert(1, '  '.join('-' * w for w in width))
    return '\n'.join(lines)


def build_parser():
    p = argparse.ArgumentParser(prog='python -m vbx_amd.score', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('-r', dest='ref_rttm_fns', nargs='+', required=True, metavar='REF', help='reference RTTM files')
    p.add_argument('-s', dest='sys_rttm_fns', nargs='+', required=True, metavar='SYS', help='system RTTM files')
    p.add_argument('-u', '--uem', dest='uemf', default=None, metavar='UEM', help='not supported: the scored extent is the extent of the turns')
    p.add_argument('--collar', type=float, default=0.0, metavar='DUR',
                   help='no-score zone of +-DUR seconds round every reference turn boundary (default: %(default)s)')
    p.add_argument('--ignore_overlaps', action='store_true', help='do not score where two or more reference speakers speak')
    p.add_argument('--device', type=int, default=None, metavar='N', help='sum on GPU N (default: in numpy on the host)')
    return p


def main(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if args.uemf is not None:
        p.error('-u/--uem is not supported: the scored extent of a recording runs from its first turn start to its last '
                'turn end (reference and system)')
    if not args.collar >= 0.0:
        p.error('--collar must be >= 0')
    try:
        records, overall = score_rttm(args.ref_rttm_fns, args.sys_rttm_fns, args.collar, args.ignore_overlaps, args.device)
    except (ValueError, OSError) as exc:
        p.error(str(exc))
    print(format_table(records, overall))
    return 0


if __name__ == '__main__':
    sys.exit(main())
