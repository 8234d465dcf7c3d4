#!/usr/bin/env python
"""python -m vbx_amd.tune: grid search over Fa, Fb and loopP on a labelled development set, scored with md-eval's DER or
with any other column of dscore's table.

    python -m vbx_amd.tune --xvec-ark-file x.ark --segments-file x.seg --xvec-transform transform.h5 --plda-file plda \\
        --threshold -0.015 --lda-dim 128 --ref-rttm-dir ref --Fa 0.2 0.3 0.4 --Fb 11 17 --loopP 0.9 0.99

The reference's recipes fix Fa, Fb and loopP per corpus (DIHARD2_run.sh:45-47); the values come from such a search.  The
grid is the product of the values given, Fa outermost, loopP innermost.  The archive is read and projected ONCE and the AHC
initialisation, which does not depend on the three parameters, runs ONCE per recording; the VB-HMM then runs for every grid
point on those AHC labels -- the very calls ``python -m vbx_amd.vbhmm`` makes at that point, so the labels are its labels.  ALL
label sequences of all points and recordings are scored against ``<ref-rttm-dir>/<recording>.rttm`` in one device call that
builds the turns and the cell edges itself (``score.score_labels``, vbx_labels_score.hpp).  Printed: one line per grid point,
``Fa Fb loopP DER Miss FA Conf`` in percent of the scored reference time pooled over the recordings (the ``*** OVERALL ***``
row of ``python -m vbx_amd.score``), in grid order; then the best point, the first in grid order among equals.

``--criterion COLUMN`` judges the grid by another column of ``python -m vbx_amd.metrics``: ``jer``, ``b3_precision``,
``b3_recall``, ``b3_f1``, ``gkt_ref_sys``, ``gkt_sys_ref``, ``h_ref_sys``, ``h_sys_ref``, ``mi``, ``nmi`` (``--step``: their frame step,
0.010 s).  DER is time-weighted: a point that swallows a short speaker into a long one looks good; JER weighs every
reference speaker the same.  The label sequences then go through ``metrics.score_labels`` (vbx_labels_frame.hpp beside
vbx_labels_score.hpp), the table holds all eleven columns pooled by the OVERALL rules of ``vbx_amd.metrics``, and the best
point is the smallest ``der``, ``jer``, ``h_ref_sys`` or ``h_sys_ref`` or the largest of any other column; a figure that is
nan never wins.  Without ``--criterion`` and ``--step`` nothing of this is computed and the output is what it always was.

tune scores the TURNS, not RTTM TEXT.  ``vbhmm --ref-rttm-dir`` scores the text it wrote, whose start and duration are printed
to six decimals; a figure here can differ from that table by the rounding of the text, at most 1 us per system boundary.
Nothing else differs.

``--init random_N`` (default ``AHC+VB``) runs no AHC: every grid point runs ``--random-restarts`` restarts per recording from
random labels over N speakers (``--seed``; ``vbhmm.DeviceStages.vb_random``) and scores the winner by final ELBO -- again the
labels ``python -m vbx_amd.vbhmm --init random_N`` writes at that point.

``--init RTTM+VB --init-rttm-dir DIR`` runs no AHC either: every grid point starts from the same given diarization,
``DIR/<recording>.rttm`` resampled onto the x-vector windows on the device (``vbhmm.DeviceStages.vb_turns``; DESIGN section
24), so no T x T matrix is held and nothing is drawn.  ``RTTM`` alone is refused like ``AHC`` alone: it runs no VB-HMM.

One process: refused under ``torchrun`` with several ranks, as ``--ref-rttm-dir`` is, because every rank would see only its
share of the recordings.  As a library: ``tune`` (reads the files), ``tune_recordings`` (data in memory), ``format_table``.
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

from . import score
from .start import ahc_options_ignored, from_args
from .kaldi_formats import read_xvector_timing_dict

__all__ = ['main', 'tune', 'tune_recordings', 'grid_points', 'best_point', 'format_table', 'build_parser']

FIGURES = ('der', 'miss', 'fa', 'confusion', 'ref_time')
SMALLER_IS_BETTER = ('der', 'jer', 'h_ref_sys', 'h_sys_ref')        # of metrics.COLUMNS; larger is better for the others


def grid_points(Fa, Fb, loopP):
    """[(Fa, Fb, loopP)]: the product of the three value lists, Fa outermost, loopP innermost."""
    points = [(float(a), float(b), float(p)) for a, b, p in itertools.product(Fa, Fb, loopP)]
    if not points:
        raise ValueError('the grid is empty: Fa, Fb and loopP need at least one value each')
    for _a, _b, p in points:
        if not 0 <= p <= 1:
            raise ValueError(f'Expecting loopP between 0 and 1, got {p} instead.')
    return points


def best_point(pooled, criterion='der'):
    """Index of the best pooled figure of ``criterion``: the smallest DER, JER or conditional entropy, the largest of any
    other column; the first in grid order among equals; a figure that is nan (a DER without scored reference time) is never
    better than one that is not."""
    sign = 1.0 if criterion in SMALLER_IS_BETTER else -1.0
    cost = [sign * p[criterion] if p[criterion] == p[criterion] else float('inf') for p in pooled]
    return int(np.argmin(cost))                                      # (argmin: the first of the smallest)


def check_criterion(criterion, step):
    """(criterion, step) as given, or ValueError.  ``step`` None: the default of ``vbx_amd.metrics`` where a criterion needs one."""
    from .metrics import COLUMNS
    if criterion not in COLUMNS:
        raise ValueError(f'--criterion {criterion}: not one of ' + ', '.join(COLUMNS))
    if step is not None and not (float(step) > 0.0 and float(step) != float('inf')):
        raise ValueError('--step must be > 0')
    return criterion, (None if step is None else float(step))


def check_one_rank(world=None):
    if world is None:
        from .vbhmm import _rank_world
        world = max(_rank_world()[1], int(os.environ.get('WORLD_SIZE', 1)))
    if world > 1:
        raise ValueError('python -m vbx_amd.tune is not supported with more than one rank: every rank sees only its share of '
                         'the recordings, and a grid point is judged on all of them')


def check_init(args):
    """(N or None, restarts, seed) of ``args.init`` (default ``'AHC+VB'``), ``args.random_restarts`` and ``args.seed``, or
    ValueError (``start.check_options``): the grid is one of VB-HMM parameters, so ``AHC`` alone and ``RTTM`` alone are refused."""
    start = from_args(args, need_vb=True)
    return start.n_random, start.restarts, start.seed


def read_reference(ref_rttm_dir, names):
    """{recording: turns} from ``<ref_rttm_dir>/<recording>.rttm``."""
    if not os.path.isdir(ref_rttm_dir):
        raise ValueError(f'--ref-rttm-dir {ref_rttm_dir}: no such directory')
    out = {}
    for name in names:
        path = os.path.join(ref_rttm_dir, f'{name}.rttm')
        if not os.path.isfile(path):
            raise ValueError(f'--ref-rttm-dir {ref_rttm_dir}: no reference {name}.rttm')
        out[name] = score.read_turns(path).get(name, [])
    return out


def tune_recordings(recordings, segs_dict, models, args, grid, ref_turns, stages=None, log=print, ahc_scores=None,
                    t_start=None, t_read=None):
    """The grid search for recordings in memory: ``recordings`` = ``[(name, seg_names, x)]``, ``segs_dict``, ``models`` and
    ``args`` (threshold, lda_dim, init_smoothing and, optionally, precision, ahc_scores, target_energy, collar,
    ignore_overlaps, criterion, step, decode) as ``vbhmm.diarize_recordings`` takes them, ``grid`` = ``[(Fa, Fb, loopP)]``, ``ref_turns`` =
    ``{name: [(start, end, speaker)]}``.  ``stages`` defaults to ``DeviceStages()``; with injected host stages (an object
    without a device context) the scoring runs in numpy.

    -> dict: ``grid``, ``names``, ``labels`` [point][recording] (first speaker per segment: what ``diarize_recordings`` gives
    at that point), ``records`` [point][recording] (records of ``score.score_labels``), ``pooled`` [point], ``best`` (index
    into the grid) and ``timing`` (seconds: read, project, ahc, vb, score_prepare, score_device, score_mapping, total).

    ``args.criterion`` (default ``'der'``) names the column of ``metrics.COLUMNS`` that ``best`` follows, ``args.step`` (default
    None) the frame step.  With anything but the two defaults the records are those of ``metrics.score_labels`` (all eleven
    columns and their integers), ``pooled`` the OVERALL rows of ``metrics._overall``, and the dict also holds ``criterion`` and
    ``step``."""
    from concurrent.futures import ThreadPoolExecutor
    from ._capi import MAX_DECODE_STATES, MAX_SPEAKERS
    from .vbhmm import DECODES, DeviceStages, _ahc_kw, driver_threads, tune_host_process
    decode = getattr(args, 'decode', 'posterior')
    if decode not in DECODES:
        raise ValueError(f'decode must be one of {DECODES}, not {decode!r}')
    most = MAX_DECODE_STATES if decode == 'viterbi' else MAX_SPEAKERS
    criterion, step = check_criterion(getattr(args, 'criterion', 'der'), getattr(args, 'step', None))
    extended = criterion != 'der' or step is not None
    grid = [tuple(float(v) for v in g) for g in grid]
    if not grid:
        raise ValueError('the grid is empty: Fa, Fb and loopP need at least one value each')
    for _a, _b, p in grid:
        assert 0 <= p <= 1, f'Expecting loopP between 0 and 1, got {p} instead.'
    names = [r[0] for r in recordings]
    missing = [n for n in names if n not in ref_turns]
    if missing:
        raise ValueError('no reference turns for: ' + ', '.join(missing))
    ahc_kw = _ahc_kw(args, ahc_scores)
    start = from_args(args, need_vb=True)                            # the one place that knows which kind of start this is
    def refuse_too_many(labels):
        for name, lab in zip(names, labels):
            if start.states(name, lab) > most:
                raise ValueError(start.too_many(start.states(name, lab), tune_name=name, most=most))
    start.read(names, segs_dict)
    ahc = [None] * len(recordings)
    if not start.runs_ahc:                                           # (no AHC: known before anything runs)
        refuse_too_many(ahc)
    if t_read is None:
        t_read = time.perf_counter()
    if t_start is None:
        t_start = t_read
    own_stages = stages is None
    if own_stages:
        stages = DeviceStages()
    device = getattr(getattr(stages, 'ctx', None), 'device', None)
    try:
        stages.project(recordings, models, args.lda_dim)
        t_proj = time.perf_counter()
        for name in names:
            log(name)
        # the AHC initialisation does not depend on the grid: once per recording, a few recordings side by side as in the driver
        if start.runs_ahc:
            with tune_host_process(), ThreadPoolExecutor(max_workers=driver_threads()) as pool:
                ahc = list(pool.map(lambda k: start.stage1(stages, k, names[k], args.threshold, ahc_kw)[0], range(len(recordings))))
            if hasattr(stages, 'close_thread_contexts'):
                stages.close_thread_contexts()
            refuse_too_many(ahc)
        for name, seg_names, _x in recordings:
            assert np.all(segs_dict[name][0] == seg_names)                                # vbhmm.py:166
        t_ahc = time.perf_counter()
        ks = list(range(len(recordings)))
        labels = []
        for Fa, Fb, loopP in grid:                                   # the call diarize_recordings makes at this point
            common = dict(init_smoothing=args.init_smoothing, maxIters=40, epsilon=1e-6, precision=getattr(args, 'precision', 'fp64'),
                          loopProb=loopP, Fa=Fa, Fb=Fb)
            if decode != 'posterior':                                # (every point is read out the same way)
                common['decode'] = decode
            res = start.run(stages, ks, names, ahc, common) if ks else []
            labels.append([np.asarray(r[0]) for r in res])
        t_vb = time.perf_counter()
        items = []
        for k, name in enumerate(names):
            begin, end = segs_dict[name][1].T
            items.append((ref_turns[name], begin, end, [labels[g][k] for g in range(len(grid))]))
        split = {}
        collar, ignore_overlaps = getattr(args, 'collar', 0.25), getattr(args, 'ignore_overlaps', False)
        if extended:
            from . import metrics
            step = 0.010 if step is None else step
            per_rec = metrics.score_labels(items, collar, ignore_overlaps, step, device, timing=split)
        else:
            per_rec = score.score_labels(items, collar, ignore_overlaps, device, timing=split)
        t_score = time.perf_counter()
    finally:
        if own_stages:
            stages.close()
    records = [[per_rec[k][g] for k in range(len(names))] for g in range(len(grid))]
    pooled = [metrics._overall(rs) if extended else score._pool(rs) for rs in records]
    timing = dict(read=t_read - t_start, project=t_proj - t_read, ahc=t_ahc - t_proj, vb=t_vb - t_ahc,
                  score_prepare=split.get('prepare', 0.0), score_device=split.get('device', 0.0),
                  score_mapping=split.get('mapping', 0.0), score=t_score - t_vb, total=time.perf_counter() - t_start,
                  recordings=len(names), points=len(grid), xvectors=int(sum(len(r[1]) for r in recordings)))
    result = dict(grid=grid, names=names, labels=labels, records=records, pooled=pooled, best=best_point(pooled, criterion), timing=timing)
    if decode != 'posterior':
        result['decode'] = decode
    if extended:
        result.update(criterion=criterion, step=step)
    return result


def write_best_rttm(result, out_dir, recordings, segs_dict):
    """The RTTM files of the best point, written as ``python -m vbx_amd.vbhmm`` writes them at that point."""
    from .vbhmm import _write_rttm_files
    ns = argparse.Namespace(out_rttm_dir=out_dir, output_2nd=False, init='AHC+VB')
    for k, (name, seg_names, _x) in enumerate(recordings):
        _write_rttm_files(ns, name, dict(seg_names=seg_names, labels1st=result['labels'][result['best']][k], labels2nd=None), segs_dict)


def _percent(r):
    if not r['ref_time'] > 0:
        return ['nan'] * 4
    return [f"{r['der']:.2f}"] + [f"{100.0 * r[k] / r['ref_time']:.2f}" for k in ('miss', 'fa', 'confusion')]


def _columns(r):
    from .metrics import COLUMNS
    return ['nan' if r[k] != r[k] else f'{r[k]:.2f}' for k in COLUMNS]                   # (metrics.format_table's numbers)


def format_table(result):
    """One line per grid point, in grid order: Fa Fb loopP DER Miss FA Conf (pooled, percent); then the best point.  A
    result judged by ``--criterion`` or counted with ``--step``: Fa Fb loopP and the eleven columns of ``vbx_amd.metrics``
    (the pooled OVERALL row of the point), then the best point with the column it was chosen by."""
    if 'criterion' in result:
        from .metrics import COLUMNS, HEADER
        rows = [['Fa', 'Fb', 'loopP'] + HEADER[1:]] + [[f'{v:g}' for v in g] + _columns(p) for g, p in zip(result['grid'], result['pooled'])]
        best = f'{HEADER[1 + COLUMNS.index(result["criterion"])]}={_columns(result["pooled"][result["best"]])[COLUMNS.index(result["criterion"])]}'
    else:
        rows = [['Fa', 'Fb', 'loopP', 'DER', 'Miss', 'FA', 'Conf']]
        rows += [[f'{v:g}' for v in g] + _percent(p) for g, p in zip(result['grid'], result['pooled'])]
        best = f'DER={_percent(result["pooled"][result["best"]])[0]}'
    width = [max(len(r[c]) for r in rows) for c in range(len(rows[0]))]
    lines = ['  '.join(r[c].rjust(width[c]) for c in range(len(rows[0]))) for r in rows]
    if 'decode' in result:                                           # (--decode other than the default: said above the header row)
        lines.insert(0, f'decode: {result["decode"]}')
    Fa, Fb, loopP = result['grid'][result['best']]
    lines.append(f'best: Fa={Fa:g} Fb={Fb:g} loopP={loopP:g} {best}')
    return '\n'.join(lines)


def to_json(result, args=None):
    keys = FIGURES
    if 'criterion' in result:
        from .metrics import COLUMNS
        keys = tuple(COLUMNS) + FIGURES[1:]

    def figures(r):
        return {k: (None if r[k] != r[k] else float(r[k])) for k in keys}
    points = []
    for g, pooled, recs in zip(result['grid'], result['pooled'], result['records']):
        points.append(dict(Fa=g[0], Fb=g[1], loopP=g[2], pooled=figures(pooled),
                           recordings={n: figures(r) for n, r in zip(result['names'], recs)}))
    b = result['best']
    out = dict(collar=getattr(args, 'collar', None), ignore_overlaps=getattr(args, 'ignore_overlaps', None), points=points,
               best=dict(index=b, Fa=result['grid'][b][0], Fb=result['grid'][b][1], loopP=result['grid'][b][2],
                         pooled=figures(result['pooled'][b])), timing=result['timing'])
    if 'criterion' in result:
        out.update(criterion=result['criterion'], step=result['step'])
    if 'decode' in result:
        out.update(decode=result['decode'])
    return out


def tune(args, stages=None, log=print):
    """The whole archive: reads the files ``args`` names, then ``tune_recordings``.  Prints nothing; writes ``args.out_json``
    and the files of ``args.best_rttm_dir`` where given.  -> the dict of ``tune_recordings``."""
    from .vbhmm import _ahc_kw, _read_recordings, load_models
    check_one_rank()
    grid = grid_points(args.Fa, args.Fb, args.loopP)
    check_criterion(getattr(args, 'criterion', 'der'), getattr(args, 'step', None))
    _ahc_kw(args, None)
    check_init(args)
    if not os.path.isdir(args.ref_rttm_dir):                          # (found before the run, not after it)
        raise ValueError(f'--ref-rttm-dir {args.ref_rttm_dir}: no such directory')
    if getattr(args, 'init_rttm_dir', None) is not None:
        from .turn_init import check_init_rttm_dir
        check_init_rttm_dir(args.init_rttm_dir)
    t_start = time.perf_counter()
    segs_dict = read_xvector_timing_dict(args.segments_file)
    models = load_models(args.xvec_transform, args.plda_file)
    recordings = _read_recordings(args.xvec_ark_file)
    ref_turns = read_reference(args.ref_rttm_dir, [r[0] for r in recordings])
    t_read = time.perf_counter()
    result = tune_recordings(recordings, segs_dict, models, args, grid, ref_turns, stages, log=log, t_start=t_start, t_read=t_read)
    if getattr(args, 'best_rttm_dir', None):
        write_best_rttm(result, args.best_rttm_dir, recordings, segs_dict)
    if getattr(args, 'out_json', None):
        with open(args.out_json, 'w') as fp:
            json.dump(to_json(result, args), fp, indent=1)
    return result


def build_parser():
    from .vbhmm import add_decode_argument, add_init_arguments
    p = argparse.ArgumentParser(prog='python -m vbx_amd.tune', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--xvec-ark-file', required=True, type=str,
                   help='Kaldi ark file with x-vectors from one or more input recordings (all x-vectors of one recording consecutive)')
    p.add_argument('--segments-file', required=True, type=str, help='File with x-vector timing info')
    p.add_argument('--xvec-transform', required=True, type=str, help='x-vector transformation: h5 (or npz) file')
    p.add_argument('--plda-file', required=True, type=str, help='PLDA model in Kaldi format')
    p.add_argument('--threshold', required=True, type=float, help='threshold (bias) used for AHC')
    add_init_arguments(p, default='AHC+VB')
    p.add_argument('--lda-dim', required=True, type=int, help='x-vectors are reduced to this dimensionality for VB-HMM')
    p.add_argument('--Fa', required=True, type=float, nargs='+', help='grid values of Fa (outermost)')
    p.add_argument('--Fb', required=True, type=float, nargs='+', help='grid values of Fb')
    p.add_argument('--loopP', required=True, type=float, nargs='+', help='grid values of loopP (innermost)')
    p.add_argument('--target-energy', required=False, type=float, default=1.0, help='see python -m vbx_amd.vbhmm')
    p.add_argument('--ahc-scores', required=False, type=str, default='cos', choices=['cos', 'plda'], help='similarity of the AHC stage')
    p.add_argument('--init-smoothing', required=False, type=float, default=5.0,
                   help='smoothing of the hard AHC labels into the initial soft assignments')
    p.add_argument('--precision', default='fp64', choices=['fp64', 'fp32', 'fp32-split'], help='arithmetic of the VB-HMM kernels')
    add_decode_argument(p)
    p.add_argument('--ref-rttm-dir', required=True, type=str, help='reference turns: <dir>/<recording>.rttm for every recording of the archive')
    p.add_argument('--collar', required=False, type=float, default=0.25,
                   help='no-score zone round every reference turn boundary, seconds (default: %(default)s)')
    p.add_argument('--ignore_overlaps', action='store_true', help='do not score where two or more reference speakers speak')
    p.add_argument('--criterion', required=False, type=str, default='der', metavar='COLUMN',
                   help='the column the best point is chosen by: der (default), jer, b3_precision, b3_recall, b3_f1, gkt_ref_sys, '
                        'gkt_sys_ref, h_ref_sys, h_sys_ref, mi or nmi; anything but der prints all eleven columns per point')
    p.add_argument('--step', required=False, type=float, default=None, metavar='DUR',
                   help='frame step of the columns other than DER in seconds (default: 0.010); given, it prints all eleven columns')
    p.add_argument('--out-json', required=False, type=str, default=None, metavar='FILE',
                   help='write the points, the per-recording and pooled figures, the best point and the stage timings')
    p.add_argument('--best-rttm-dir', required=False, type=str, default=None, metavar='DIR',
                   help='write the RTTM files of the best point, as python -m vbx_amd.vbhmm writes them at that point')
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        check_one_rank(int(os.environ.get('WORLD_SIZE', 1)))
        grid_points(args.Fa, args.Fb, args.loopP)
        if not os.path.isdir(args.ref_rttm_dir):
            raise ValueError(f'--ref-rttm-dir {args.ref_rttm_dir}: no such directory')
        if not args.collar >= 0.0:
            raise ValueError('--collar must be >= 0')
        check_criterion(args.criterion, args.step)
        check_init(args)
        if ahc_options_ignored(args.init) is not None:
            print(f'warning: {ahc_options_ignored(args.init)}', file=sys.stderr)
    except ValueError as exc:
        parser.error(str(exc))
    try:
        result = tune(args, log=lambda *a, **k: None)              # (the table is all this program prints)
    except (ValueError, OSError, RuntimeError) as exc:
        print(f'tune: {type(exc).__name__}: {exc}', file=sys.stderr)
        return 1
    print(format_table(result))
    return 0


if __name__ == '__main__':
    sys.exit(main())
