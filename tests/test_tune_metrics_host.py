"""``metrics.score_labels`` and ``python -m vbx_amd.tune --criterion`` without a GPU: the numpy route against the dense referee
``tests/metrics_ref.py`` on the turns ``score.labels_turns`` gives, a hand case worked out below, the four segment layouts of
DESIGN section 18 with boundaries where quotient, product and literal disagree; the grid search on injected host stages that
return prescribed labels (which column picks which point, ties, nan); table, JSON, parser; the entry point in the header.
"""
import argparse
import json
import math
import os
import re

import numpy as np
import pytest

import metrics_ref
from test_tune_host import sliding_windows

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOATS = ('jer', 'b3_precision', 'b3_recall', 'b3_f1', 'gkt_ref_sys', 'gkt_sys_ref', 'h_ref_sys', 'h_sys_ref', 'mi', 'nmi')

# the four layouts of section 18 with segment boundaries at 0.07, 0.29 and 0.57 s, where 0.07 / 0.01 = 7.000000000000001,
# 0.29 / 0.01 = 28.999999999999996 and 0.01 * 57 = 0.5700000000000001: name -> (starts, ends)
DECIMAL_LAYOUTS = {
    'gaps': ([0.0, 0.1, 0.29, 0.6], [0.07, 0.29, 0.57, 1.0]),                                    # 0.07 | 0.1 and 0.57 | 0.6 are gaps
    'touching': ([0.0, 0.07, 0.29, 0.57], [0.07, 0.29, 0.57, 1.0]),
    'overlap': ([0.0, 0.04, 0.25, 0.5], [0.1, 0.33, 0.64, 1.0]),                                 # midpoints 0.07, 0.29, 0.57
    'identical': ([0.0, 0.07, 0.07, 0.07, 0.29, 0.57], [0.07, 0.29, 0.29, 0.29, 0.57, 1.0]),     # three share both times
}
DECIMAL_REF = [(0.0, 0.29, 'A'), (0.07, 0.57, 'B'), (0.57, 1.0, 'A'), (0.9, 1.2, 'C')]


def decimal_items(shift=0.0):
    """one item per layout: three label sequences each (alternating, one label, 0 1 1 ... 2)"""
    items = []
    for starts, ends in DECIMAL_LAYOUTS.values():
        T = len(starts)
        hyps = [np.arange(T) % 2, np.zeros(T, dtype=np.int64), np.array([0] + [1] * (T - 2) + [2])]
        items.append(([(b + shift, e + shift, s) for b, e, s in DECIMAL_REF], np.array(starts) + shift, np.array(ends) + shift, hyps))
    return items


def assert_floats_close(got, want, what=''):
    """1e-12 relative, the bound of tests/test_metrics_host.py: both sides sum at most a few thousand float64 terms from the
    same integers"""
    for k in FLOATS:
        print(what, k, repr(got[k]), repr(want[k]))
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (what, k, got[k], want[k])


def assert_same_record(a, b, what=''):
    """two records of metrics.score_turns / frame_counts: the same keys, every array and float the same bytes"""
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k, a[k], b[k])
        elif isinstance(a[k], float):
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (what, k, a[k], b[k])
        else:
            assert type(a[k]) is type(b[k]) and a[k] == b[k], (what, k, a[k], b[k])


def assert_item_against_referee(item, got, collar=0.0, ignore=False, what=''):
    from vbx_amd import metrics, score
    ref, starts, ends, hyps = item
    assert len(got) == len(hyps)
    for j, labels in enumerate(hyps):
        turns = score.labels_turns(starts, ends, labels)
        want = metrics_ref.counts(ref, turns)
        metrics_ref.assert_counts_equal(got[j], want, f'{what} hypothesis {j}')
        assert_floats_close(got[j], metrics_ref.columns(want), f'{what} hypothesis {j}')
        # the definition: score_turns on the turns of merge_adjacent_labels
        assert_same_record(got[j], metrics.score_turns([(ref, turns)], collar, ignore)[0], f'{what} hypothesis {j}')


# ---- score_labels(device=None) against the dense referee --------------------------------------------------------------------
@pytest.mark.parametrize('collar,ignore', [(0.0, False), (0.25, True)])
def test_numpy_route_equals_the_referee_and_the_definition(collar, ignore):
    from vbx_amd import metrics
    items = []
    for seed, T in ((1, 1), (2, 2), (3, 40), (4, 257)):
        ref, starts, ends, labels = sliding_windows(seed, T)
        items.append((ref, starts, ends, [labels, (labels + 1) % 3, np.zeros_like(labels)]))
    timing = {}
    got = metrics.score_labels(items, collar, ignore, timing=timing)
    assert {'prepare', 'device', 'mapping'} <= set(timing) and all(v >= 0.0 for v in timing.values())
    for k, item in enumerate(items):
        assert_item_against_referee(item, got[k], collar, ignore, f'item {k}')
    counts = metrics.frame_counts_labels(items)
    for k in range(len(items)):
        for j in range(3):
            metrics_ref.assert_counts_equal(counts[k][j], got[k][j], f'item {k} hypothesis {j}')


@pytest.mark.parametrize('shift', [0.0, 1234.5])
def test_the_four_layouts_on_the_crafted_boundaries(shift):
    from vbx_amd import metrics, score
    items = decimal_items(shift)
    got = metrics.score_labels(items)
    for name, item, recs in zip(DECIMAL_LAYOUTS, items, got):
        assert_item_against_referee(item, recs, what=f'{name} + {shift}')
    if shift == 0.0:
        # the overlapping windows do meet where the layout says, and the three identical windows give a turn without duration
        meet = score.labels_turns(*items[2][1:3], items[2][3][0])
        assert [t[1] for t in meet[:3]] == [(0.1 + 0.04) / 2.0, (0.33 + 0.25) / 2.0, (0.64 + 0.5) / 2.0]
        same = score.labels_turns(*items[3][1:3], items[3][3][0])
        assert any(b == e for b, e, _ in same) and all(b < e for b, e, _ in meet)


def test_shapes_and_refusals():
    from vbx_amd import metrics
    assert metrics.score_labels([]) == [] and metrics.score_labels([([(0.0, 1.0, 'x')], [0.0], [1.0], [])]) == [[]]
    with pytest.raises(ValueError, match='step'):
        metrics.score_labels([], step=0.0)
    with pytest.raises(ValueError, match='collar'):
        metrics.score_labels([], collar=-1.0)
    empty = metrics.score_labels([([(0.0, 1.0, 'x')], [], [], [[]])])[0][0]              # no segment: nothing but the reference
    assert empty['jer'] == 100.0 and empty['sys_speakers'] == [] and empty['ref_durs'].tolist() == [100]
    # what the device would refuse runs in numpy whatever the device: 65 labels, times that decrease, a segment without duration
    T = 130
    wide = ([(0.0, 2.0, 'x')], 0.1 * np.arange(T), 0.1 * np.arange(T) + 0.1, [np.arange(T) % 65])
    back = ([(0.0, 2.0, 'x')], [0.5, 0.0], [1.0, 0.5], [[0, 1]])
    flat = ([(0.0, 2.0, 'x')], [0.0, 1.0], [1.0, 1.0], [[0, 1]])
    a, b = metrics.frame_counts_labels([wide, back, flat], device=None), metrics.frame_counts_labels([wide, back, flat], device=0)
    for x, y in zip(a, b):
        metrics_ref.assert_counts_equal(y[0], x[0])
    assert len(a[0][0]['sys_speakers']) == 65 and a[2][0]['sys_speakers'] == [0]


# ---- the hand case ------------------------------------------------------------------------------------------------------
HAND_REF = [(0.0, 90.0, 'A'), (90.0, 100.0, 'B')]
HAND_STARTS, HAND_ENDS = np.arange(100.0), np.arange(100.0) + 1.0
HAND_ONE = np.zeros(100, dtype=np.int64)
HAND_THREE = np.array([0] * 60 + [2] * 30 + [1] * 10)


def test_the_criteria_disagree_on_the_hand_case():
    """100 segments of 1 s: 10 000 frames.  Reference A on [0, 90), B on [90, 100): 9000 and 1000 frames.

    All labels 0.  cm = [[9000], [1000]].
      DER  label 0 is mapped to A; B's 10 s are confusion: 100 * 10 / 100 = 10.
      JER  A: 1 - 9000 / 10000 = 0.1; B is unmapped: 1; 100 * (0.1 + 1) / 2 = 55.
      B3   precision (9000^2 + 1000^2) / 10000 / 10000 = 0.82, recall 1, F1 = 2 * 0.82 / 1.82 = 0.9011.
      NMI  H(sys) = 0 and H(ref) > 0: 0 by the degenerate rule.
    Labels 0 on segments 0-59, 2 on 60-89, 1 on 90-99.  cm = [[6000, 3000, 0], [0, 0, 1000]] (classes in order of appearance).
      DER  A -> 0 (60 s), B -> 1 (10 s); label 2's 30 s under A are confusion: 30.
      JER  A against 0: 1 - 6000 / 9000 = 1/3; B against 1: 0; 100 * (1/3 + 0) / 2 = 16.67.
      B3   every column lies in one row: precision 1; recall (6000^2 / 9000 + 3000^2 / 9000 + 1000^2 / 1000) / 10000 = 0.6;
           F1 = 2 * 0.6 / 1.6 = 0.75.
      NMI  H(ref|sys) = 0, so MI = H(ref) = H(0.9, 0.1) = 0.4690 bits; H(sys) = H(0.6, 0.3, 0.1) = 1.2955 bits;
           NMI = 0.4690 / sqrt(0.4690 * 1.2955) = sqrt(0.4690 / 1.2955) = 0.6017.
    DER and B3-F1 prefer the first sequence, JER and NMI the second."""
    from vbx_amd import metrics
    one, three = metrics.score_labels([(HAND_REF, HAND_STARTS, HAND_ENDS, [HAND_ONE, HAND_THREE])])[0]
    assert one['cm'].tolist() == [[9000], [1000]] and three['cm'].tolist() == [[6000, 3000, 0], [0, 0, 1000]]
    assert three['sys_classes'] == [(0,), (2,), (1,)] and three['sys_speakers'] == [0, 1, 2] and three['sys_durs'].tolist() == [6000, 1000, 3000]
    assert one['der'] == pytest.approx(10.0, abs=1e-9) and three['der'] == pytest.approx(30.0, abs=1e-9)
    assert one['jer'] == pytest.approx(55.0, abs=1e-9) and three['jer'] == pytest.approx(100.0 / 6.0, abs=1e-9)
    assert one['b3_f1'] == pytest.approx(2 * 0.82 / 1.82, abs=1e-12) and three['b3_f1'] == pytest.approx(0.75, abs=1e-12)
    h = lambda *p: -sum(x * math.log2(x) for x in p)
    assert one['nmi'] == 0.0 and three['nmi'] == pytest.approx(math.sqrt(h(0.9, 0.1) / h(0.6, 0.3, 0.1)), abs=1e-12)
    assert [round(three[k], 4) for k in ('jer', 'b3_f1', 'nmi')] == [16.6667, 0.75, 0.6017] and round(one['b3_f1'], 4) == 0.9011


# ---- the grid search on injected host stages -------------------------------------------------------------------------------
class PrescribedStages:
    """host stages (no device context: the scoring runs in numpy) whose VB-HMM returns the labels prescribed for the point"""

    def __init__(self, by_fa):
        self.by_fa, self.T = by_fa, None

    def project(self, recordings, models, lda_dim):
        self.T = [len(r[1]) for r in recordings]

    def ahc(self, k, threshold, **kw):
        return (np.zeros(self.T[k], dtype=np.int64),)

    def vb(self, ks, ahc, Fa=None, **kw):
        return [(np.asarray(self.by_fa[Fa][k]),) for k in ks]


def hand_search(criterion='der', step=None, ref=HAND_REF, sequences=(HAND_ONE, HAND_THREE, HAND_THREE, HAND_ONE), **extra):
    """four grid points Fa = 0.1 .. 0.4 on one recording: the first and the last give all labels 0, the two in the middle the
    three labels"""
    from vbx_amd import tune
    seg_names = np.array([f'rec_{k:04d}' for k in range(100)])
    recordings = [('rec', seg_names, np.zeros((100, 1)))]
    segs_dict = {'rec': (seg_names, np.stack([HAND_STARTS, HAND_ENDS], axis=1))}
    grid = [(0.1, 17.0, 0.9), (0.2, 17.0, 0.9), (0.3, 17.0, 0.9), (0.4, 17.0, 0.9)]
    args = argparse.Namespace(threshold=0.0, lda_dim=1, init_smoothing=5.0, collar=0.0, **extra)
    if criterion is not None:
        args.criterion = criterion
    if step is not None:
        args.step = step
    stages = PrescribedStages({g[0]: [seq] for g, seq in zip(grid, sequences)})
    return tune.tune_recordings(recordings, segs_dict, {}, args, grid, {'rec': ref}, stages=stages, log=lambda *a: None), args


def test_every_criterion_picks_its_point_and_the_first_among_equals():
    from vbx_amd import metrics, tune
    assert set(tune.SMALLER_IS_BETTER) <= set(metrics.COLUMNS)
    picks = {c: hand_search(c)[0]['best'] for c in metrics.COLUMNS}
    # the first and the last point are equal, and so are the two in the middle: always the first of a pair
    assert picks['der'] == 0 and picks['b3_f1'] == 0 and picks['jer'] == 1 and picks['nmi'] == 1
    assert picks == dict(der=0, jer=1, b3_precision=1, b3_recall=0, b3_f1=0, gkt_ref_sys=0, gkt_sys_ref=1, h_ref_sys=1, h_sys_ref=0,
                         mi=1, nmi=1)
    # the same with the equal points in the other order
    flipped = (HAND_THREE, HAND_ONE, HAND_ONE, HAND_THREE)
    assert [hand_search(c, sequences=flipped)[0]['best'] for c in ('der', 'b3_f1', 'jer', 'nmi')] == [1, 1, 0, 0]
    nan = float('nan')
    for c in metrics.COLUMNS:                                          # a figure that is nan never wins, whichever way the column runs
        assert tune.best_point([{c: nan}, {c: 0.5}, {c: nan}, {c: 0.5}], c) == 1 and tune.best_point([{c: nan}] * 3, c) == 0
    assert tune.best_point([dict(jer=5.0), dict(jer=3.0), dict(jer=3.0)], 'jer') == 1
    assert tune.best_point([dict(nmi=0.5), dict(nmi=0.7), dict(nmi=0.7)], 'nmi') == 1
    # no reference: every pooled DER is nan, none wins, the first point stands; the table says nan
    result, _ = hand_search('der', step=0.01, ref=[])
    assert result['best'] == 0 and all(math.isnan(p['der']) for p in result['pooled']) and result['pooled'][0]['jer'] == 100.0
    assert re.split(r'\s{2,}', tune.format_table(result).splitlines()[1].strip())[3] == 'nan'


def test_records_pooled_rows_table_and_json_of_a_criterion(tmp_path):
    from vbx_amd import metrics, score, tune
    result, args = hand_search('jer')
    assert result['criterion'] == 'jer' and result['step'] == 0.010 and result['best'] == 1
    want = metrics.score_labels([(HAND_REF, HAND_STARTS, HAND_ENDS, [HAND_ONE, HAND_THREE, HAND_THREE, HAND_ONE])], 0.0, False, 0.010)[0]
    for g in range(4):
        assert_same_record(result['records'][g][0], want[g], f'point {g}')
        pooled = metrics._overall(result['records'][g])
        assert all(np.float64(result['pooled'][g][k]).tobytes() == np.float64(pooled[k]).tobytes() for k in metrics.COLUMNS)
    assert set(result['timing']) == set(hand_search(None)[0]['timing'])          # nothing but the split the call reports
    lines = tune.format_table(result).splitlines()
    assert len(lines) == 6 and len({len(l) for l in lines[:5]}) == 1
    assert re.split(r'\s{2,}', lines[0].strip()) == ['Fa', 'Fb', 'loopP'] + metrics.HEADER[1:]
    for g in range(4):
        assert re.split(r'\s{2,}', lines[1 + g].strip()) == [f'{0.1 * (g + 1):g}', '17', '0.9'] + [f'{result["pooled"][g][k]:.2f}' for k in metrics.COLUMNS]
    assert lines[1].split()[3:8] == ['10.00', '55.00', '0.82', '1.00', '0.90'] and lines[2].split()[3:8] == ['30.00', '16.67', '1.00', '0.60', '0.75']
    assert lines[5] == 'best: Fa=0.2 Fb=17 loopP=0.9 JER=16.67'
    assert tune.format_table(hand_search('gkt_sys_ref')[0]).splitlines()[5] == 'best: Fa=0.2 Fb=17 loopP=0.9 GKT(sys, ref)=1.00'
    doc = json.loads(json.dumps(tune.to_json(result, args)))
    assert doc['criterion'] == 'jer' and doc['step'] == 0.010 and doc['best']['index'] == 1 and doc['collar'] == 0.0
    for point, pooled in zip(doc['points'], result['pooled']):
        assert set(metrics.COLUMNS) <= set(point['pooled']) and set(metrics.COLUMNS) <= set(point['recordings']['rec'])
        assert all(point['pooled'][k] == pooled[k] for k in metrics.COLUMNS)
    # --step alone: the eleven columns, the best point still by DER
    by_der, _ = hand_search('der', step=0.02)
    assert by_der['criterion'] == 'der' and by_der['step'] == 0.02 and by_der['best'] == 0
    assert by_der['records'][0][0]['cm'].tolist() == [[4500], [500]]
    assert tune.format_table(by_der).splitlines()[5] == 'best: Fa=0.1 Fb=17 loopP=0.9 DER=10.00'


def test_the_default_computes_nothing_new(monkeypatch):
    from vbx_amd import metrics, score, tune
    monkeypatch.setattr(metrics, 'score_labels', lambda *a, **k: pytest.fail('the default criterion must not count frames'))
    for criterion in (None, 'der'):                                   # an args object of before this option, and the default
        result, args = hand_search(criterion)
        assert set(result) == {'grid', 'names', 'labels', 'records', 'pooled', 'best', 'timing'} and result['best'] == 0
        assert 'jer' not in result['records'][0][0] and result['pooled'] == [score._pool(r) for r in result['records']]
        lines = tune.format_table(result).splitlines()
        assert lines[0].split() == ['Fa', 'Fb', 'loopP', 'DER', 'Miss', 'FA', 'Conf'] and lines[5] == 'best: Fa=0.1 Fb=17 loopP=0.9 DER=10.00'
        doc = tune.to_json(result, args)
        assert 'criterion' not in doc and 'step' not in doc and set(doc['points'][0]['pooled']) == set(tune.FIGURES)
    with pytest.raises(ValueError, match='criterion'):
        hand_search('accuracy')
    with pytest.raises(ValueError, match='step'):
        hand_search('jer', step=0.0)


# ---- parser ---------------------------------------------------------------------------------------------------------------
def test_parser_takes_a_column_and_a_step(tmp_path, capsys):
    from vbx_amd import metrics, tune
    base = ['--xvec-ark-file', 'none.ark', '--segments-file', 'none.seg', '--xvec-transform', 'none.h5', '--plda-file', 'none', '--threshold',
            '-0.015', '--lda-dim', '128', '--ref-rttm-dir', str(tmp_path), '--Fa', '0.3', '--Fb', '17', '--loopP', '0.99']
    args = tune.build_parser().parse_args(base)
    assert args.criterion == 'der' and args.step is None
    for column in metrics.COLUMNS:
        assert tune.build_parser().parse_args(base + ['--criterion', column, '--step', '0.02']).criterion == column
    for bad, word in ((['--criterion', 'accuracy'], '--criterion'), (['--step', '0'], '--step'), (['--step', '-0.01'], '--step'),
                      (['--criterion', 'jer', '--step', 'nan'], '--step')):
        with pytest.raises(SystemExit):                               # refused before anything is read: none of the files exists
            tune.main(base + bad)
        assert word in capsys.readouterr().err
    with pytest.raises(SystemExit):
        tune.main(['--help'])
    text = capsys.readouterr().out
    assert '--criterion' in text and '--step' in text and 'TURNS, not RTTM TEXT' in text


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_listed_and_built_from_its_header():
    from vbx_amd import _capi, build, metrics
    header = open(os.path.join(REPO, 'include', 'vbx_hip.h')).read()
    assert re.search(r'\bint vbx_labels_frame_counts\s*\(', header) and 'vbx_labels_frame_counts' in _capi.ABI_SYMBOLS
    assert '#define VBX_ABI_VERSION 7' in header and callable(_capi.labels_frame_counts)
    assert 'vbx_labels_frame.hpp' in build.HEADERS and 'vbx_labels_frame.hpp' not in build.ITERATION_SOURCES
    capi = open(os.path.join(build.CSRC, 'vbx_capi.hip')).read()
    assert capi.index('#include "vbx_labels_score.hpp"') < capi.index('#include "vbx_frame_score.hpp"') < capi.index('#include "vbx_labels_frame.hpp"')
    src = open(os.path.join(build.CSRC, 'vbx_labels_frame.hpp')).read()
    assert 'atomic' not in src.split('#pragma once')[1]                      # scans and sums in a fixed order
    # one plan for both entry points: the kernels of section 20 are launched from the plan's functions and nowhere else
    frame = open(os.path.join(build.CSRC, 'vbx_frame_score.hpp')).read()
    for kernel in ('frame_bounds_kernel', 'frame_sort_kernel', 'frame_cells_kernel', 'frame_masks_kernel', 'frame_firsts_kernel',
                   'frame_classes_kernel', 'frame_acc_kernel'):
        assert frame.count(f'hipLaunchKernelGGL(vbx::{kernel}') == 1 and f'vbx::{kernel}' not in src
    assert 'frm_plan_sums(' in src and 'frm_plan_classes(' in src and 'labels_turns_kernel' in src
    assert {'frame_counts_labels', 'score_labels'} <= set(metrics.__all__)
