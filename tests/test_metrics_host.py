"""``vbx_amd.metrics`` without a GPU: the numpy route (``device=None``) against the one published row there is, against the
dense referee ``tests/metrics_ref.py`` and against cases worked out by hand; the table, the refusals, the entry point in the
header and the ABI list.

The anchor: the reference's README prints dscore's table for its example recording ES2005a under ``--collar 0.25
--ignore_overlaps``.  ``tests/golden/es2005a_dscore_table.txt`` holds those four lines, ``tests/golden/es2005a_ref.rttm`` is
the recipe's reference RTTM and ``es2005a.npz: rttm_committed`` the system RTTM the reference ships for it.
"""
import math
import os
import re

import numpy as np
import pytest

import metrics_ref
from metrics_util import CLASSES_OVER_CAP, CRAFTED, SPEAKERS_64, SPEAKERS_65, chain, grid_pair
from test_score_host import REF_RTTM, es2005a, rttm_text  # noqa: F401  (es2005a: the fixture that writes the system RTTM)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, 'tests', 'golden')
FLOATS = ('jer', 'b3_precision', 'b3_recall', 'b3_f1', 'gkt_ref_sys', 'gkt_sys_ref', 'h_ref_sys', 'h_sys_ref', 'mi', 'nmi')
HOST_PAIRS = dict(CRAFTED, **SPEAKERS_64, **SPEAKERS_65, classes_over_cap=CLASSES_OVER_CAP, chain_257=(chain(257), chain(3, 'x')),
                  grid_28_4=grid_pair(28, 4))


def assert_floats_close(got, want, what=''):
    """1e-12 relative: both sides sum at most a few thousand float64 terms from the same integers"""
    for k in FLOATS:
        print(what, k, repr(got[k]), repr(want[k]))
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (what, k, got[k], want[k])


# ---- the ES2005a anchor -------------------------------------------------------------------------------------------------
def test_es2005a_prints_the_published_table(es2005a, capsys):  # noqa: F811
    from vbx_amd import metrics
    assert metrics.main(['-r', REF_RTTM, '-s', es2005a, '--collar', '0.25', '--ignore_overlaps']) == 0
    got = [l.rstrip() for l in capsys.readouterr().out.splitlines()]
    want = [l.rstrip() for l in open(os.path.join(GOLDEN, 'es2005a_dscore_table.txt')).read().splitlines()]
    assert len(want) == 4 and got == want


def test_es2005a_class_matrix_and_referee(es2005a):  # noqa: F811
    from vbx_amd import metrics, score
    records, overall = metrics.score_rttm(REF_RTTM, es2005a, collar=0.25, ignore_overlaps=True)
    got = records['ES2005a']
    assert got['cm'].shape == (15, 8) and () in got['ref_classes'] and () in got['sys_classes']
    # collar and ignore_overlaps act on the DER column alone
    plain = metrics.score_rttm(REF_RTTM, es2005a)[0]['ES2005a']
    assert all(plain[k] == got[k] for k in FLOATS) and plain['der'] != got['der']
    want = metrics_ref.counts(score._read_all(REF_RTTM)['ES2005a'], score._read_all(es2005a)['ES2005a'])
    metrics_ref.assert_counts_equal(got, want)
    assert_floats_close(got, metrics_ref.columns(want), 'ES2005a')
    # the values the published row rounds (worked out with a throwaway dense script before any of this was written)
    assert [round(got[k], 3) for k in FLOATS[1:]] == [0.645, 0.780, 0.706, 0.712, 0.564, 1.143, 0.589, 1.717, 0.669]
    assert round(got['jer'], 4) == 29.9910
    assert all(overall[k] == got[k] for k in FLOATS + ('der',))    # one recording: OVERALL is its row


# ---- integers and floating-point columns against the dense referee ------------------------------------------------------
def test_the_crafted_boundaries_defeat_the_shortcuts():
    """What product_edges* and starts_after_zero rest on.  In float64 0.07 / 0.01 = 7.000000000000001, 0.29 / 0.01 =
    28.999999999999996 although 0.01 * 29 == 0.29, and 0.01 * 57 = 0.5700000000000001 != 0.57 with 0.57 / 0.01 =
    56.99999999999999: at each of them the quotient is no integer, at two its floor is not the frame, at one the product is
    not the literal."""
    assert [0.01 * i == float(f'0.{i:02d}') for i in (7, 29, 57)] == [True, True, False]
    assert [math.floor(float(f'0.{i:02d}') / 0.01) for i in (7, 29, 57)] == [7, 28, 56]
    assert all(float(f'0.{i:02d}') / 0.01 != i for i in (7, 29, 57))
    from vbx_amd import metrics
    assert metrics._frame_index([0.07, 0.29, 0.57], 0.01, 100).tolist() == [7, 29, 57]


@pytest.mark.parametrize('name', list(HOST_PAIRS))
def test_host_route_equals_the_referee(name):
    from vbx_amd import metrics
    ref, hyp = HOST_PAIRS[name]
    got = metrics.frame_counts([(ref, hyp)])[0]
    want = metrics_ref.counts(ref, hyp)
    metrics_ref.assert_counts_equal(got, want, name)
    assert int(got['cm'].sum()) == int(want['cm'].sum())
    rec = metrics.score_turns([(ref, hyp)])[0]
    assert_floats_close(rec, metrics_ref.columns(want), name)
    metrics_ref.assert_counts_equal(rec, want, name)


@pytest.mark.parametrize('step', [0.01, 0.02, 0.003, 0.25])
def test_other_steps(step):
    from vbx_amd import metrics
    for name in ('product_edges', 'three_overlapping', 'starts_after_zero'):
        ref, hyp = CRAFTED[name]
        metrics_ref.assert_counts_equal(metrics.frame_counts([(ref, hyp)], step=step)[0], metrics_ref.counts(ref, hyp, step), name)


def test_a_turn_shorter_than_a_frame_is_dropped_from_jer():
    from vbx_amd import metrics
    rec = metrics.score_turns([CRAFTED['shorter_than_a_frame']])[0]
    assert rec['ref_speakers'] == ['A', 'B', 'C'] and rec['ref_durs'].tolist() == [100, 100, 0]
    assert set(rec['jer_speakers']) == {'A', 'B'} and rec['sys_durs'].tolist() == [200, 0]
    # A and B each share 100 of x's 200 frames: one is mapped at 1 - 100 / 200, the other scores 1
    assert rec['jer'] == 75.0


def test_more_than_64_speakers_run_on_the_numpy_route_whatever_the_device():
    """65 speakers on a side: the record comes from the numpy route even with a device named -- no GPU is touched here."""
    from vbx_amd import metrics
    for name, (ref, hyp) in SPEAKERS_65.items():
        a = metrics.frame_counts([(ref, hyp)], device=None)[0]
        b = metrics.frame_counts([(ref, hyp)], device=0)[0]
        metrics_ref.assert_counts_equal(b, a, name)
        assert max(len(a['ref_speakers']), len(a['sys_speakers'])) == 65


# ---- hand-worked cases ----------------------------------------------------------------------------------------------------
def test_perfect_agreement_under_relabelling():
    from vbx_amd import metrics
    ref = [(0.0, 1.0, 'A'), (0.5, 2.0, 'B'), (3.0, 4.0, 'A')]
    rec = metrics.score_turns([(ref, [(b, e, {'A': 'two', 'B': 'one'}[s]) for b, e, s in ref])])[0]
    assert rec['jer'] == 0.0 and (rec['b3_precision'], rec['b3_recall'], rec['b3_f1']) == (1.0, 1.0, 1.0)
    assert rec['h_ref_sys'] == 0.0 and rec['h_sys_ref'] == 0.0 and rec['nmi'] == pytest.approx(1.0, abs=1e-15)
    assert rec['gkt_ref_sys'] == pytest.approx(1.0, abs=1e-15) and rec['gkt_sys_ref'] == pytest.approx(1.0, abs=1e-15)
    assert rec['cm'].tolist() == [[150, 0, 0, 0], [0, 50, 0, 0], [0, 0, 100, 0], [0, 0, 0, 100]]      # {A}: [0, 0.5) and [3, 4)
    assert rec['ref_classes'] == [('A',), ('A', 'B'), ('B',), ()] and rec['sys_classes'] == [('two',), ('one', 'two'), ('one',), ()]


def test_one_system_speaker_against_two_equal_reference_speakers():
    """A speaks [0, 1), B [1, 2), x all of [0, 2): 200 frames, cm = [[100], [100]].
    JER: J[A][x] = J[B][x] = 1 - 100 / 200; one is mapped, the other scores 1: 100 (0.5 + 1) / 2 = 75.
    B3: precision (100^2 / 200 + 100^2 / 200) / 200 = 0.5, recall (100^2 / 100 + 100^2 / 100) / 200 = 1, F1 = 2/3.
    V(sys) = 0: GKT(ref, sys) = 1 by the degenerate rule.  V(ref) = 1/2 = V(ref|sys): GKT(sys, ref) = 0.
    H(ref) = 1 bit = H(ref|sys), H(sys) = H(sys|ref) = 0, MI = 0; exactly one entropy is 0: NMI = 0."""
    from vbx_amd import metrics
    rec = metrics.score_turns([([(0.0, 1.0, 'A'), (1.0, 2.0, 'B')], [(0.0, 2.0, 'x')])])[0]
    assert rec['cm'].tolist() == [[100], [100]] and rec['inter'].tolist() == [[100], [100]]
    assert rec['jer'] == 75.0 and sorted(rec['jer_speakers'].values()) == [50.0, 100.0]
    assert (rec['b3_precision'], rec['b3_recall']) == (0.5, 1.0) and rec['b3_f1'] == 2.0 * 0.5 / 1.5
    assert (rec['gkt_ref_sys'], rec['gkt_sys_ref']) == (1.0, 0.0)
    assert (rec['h_ref_sys'], rec['h_sys_ref'], rec['mi'], rec['nmi']) == (1.0, 0.0, 0.0, 0.0)


def test_degenerate_rules():
    from vbx_amd import metrics
    # one class on both sides: both V and both entropies are 0 -> GKT 1 and 1, NMI 1
    rec = metrics.score_turns([([(0.0, 1.0, 'A')], [(0.0, 1.0, 'x')])])[0]
    assert (rec['gkt_ref_sys'], rec['gkt_sys_ref'], rec['nmi'], rec['mi'], rec['jer']) == (1.0, 1.0, 1.0, 0.0, 0.0)
    # no reference speaker: JER 100 where the system has a speech frame, 0 where it has none
    speech, silent, nothing = metrics.score_turns([CRAFTED['empty_reference_with_speech'], CRAFTED['empty_reference_without_frames'],
                                                   CRAFTED['both_empty']])
    assert (speech['jer'], silent['jer'], nothing['jer']) == (100.0, 0.0, 0.0)
    assert math.isnan(speech['der'])
    # no counted frame at all: B3 1 / 1 / 1, GKT 1, entropies and MI 0, NMI 1
    for rec in (silent, nothing, metrics.score_turns([CRAFTED['below_one_frame']])[0]):
        assert int(rec['cm'].sum()) == 0
        assert [rec[k] for k in FLOATS[1:]] == [1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    # an empty system: every reference speaker is unmapped
    assert metrics.score_turns([CRAFTED['empty_system']])[0]['jer'] == 100.0
    with pytest.raises(ValueError, match='step'):
        metrics.frame_counts([([], [])], step=0.0)


# ---- the table and the OVERALL row ----------------------------------------------------------------------------------------
@pytest.fixture()
def corpus(tmp_path):
    """recA: x for A, then nobody for B.  recB: one system speaker for two reference speakers.  recC: in the reference only."""
    ref = {'recA': [(0.0, 1.0, 'A'), (1.0, 2.0, 'B')], 'recB': [(0.0, 1.0, 'A'), (1.0, 2.0, 'B')], 'recC': [(0.0, 1.0, 'A')]}
    hyp = {'recA': [(0.0, 1.0, 1)], 'recB': [(0.0, 2.0, 1)]}
    (tmp_path / 'ref.rttm').write_text(''.join(rttm_text(k, v) for k, v in ref.items()))
    (tmp_path / 'sys.rttm').write_text(''.join(rttm_text(k, v) for k, v in hyp.items()))
    return tmp_path


def test_table_layout_and_overall_row(corpus, capsys):
    from vbx_amd import metrics
    assert metrics.main(['-r', str(corpus / 'ref.rttm'), '-s', str(corpus / 'sys.rttm')]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert re.split(r'\s{2,}', lines[0]) == metrics.HEADER and set(lines[1]) == {'-', ' '}
    assert [l.split()[0] for l in lines[2:5]] == ['recA', 'recB', 'recC'] and lines[5].startswith('*** OVERALL ***  ')
    assert len({len(l) for l in lines}) == 1                       # every column as wide in every line
    assert all(re.fullmatch(r'-?\d+\.\d\d', v) for l in lines[2:] for v in l.replace('*** OVERALL ***', 'all').split()[1:])
    records, overall = metrics.score_rttm(str(corpus / 'ref.rttm'), str(corpus / 'sys.rttm'))
    # JER per file: recA (0 + 1) / 2, recB (0.5 + 1) / 2, recC 1; OVERALL: the five reference speakers weigh the same
    assert [records[k]['jer'] for k in ('recA', 'recB', 'recC')] == [50.0, 75.0, 100.0]
    assert overall['jer'] == 100.0 * (0.0 + 1.0 + 0.5 + 1.0 + 1.0) / 5.0
    # DER pooled as vbx_amd.score pools it: (1 + 1 + 1) s of error in 5 s
    assert overall['der'] == 100.0 * 3.0 / 5.0
    # the block-diagonal sum: recA [[100, 0], [0, 100]], recB [[100], [100]], recC [[100]]; classes of two files never meet
    assert overall['cm'].tolist() == [[100, 0, 0, 0], [0, 100, 0, 0], [0, 0, 100, 0], [0, 0, 100, 0], [0, 0, 0, 100]]
    # precision (100 + 100 + 50 + 50 + 100) / 500, recall 1
    assert overall['b3_precision'] == pytest.approx(0.8, rel=1e-15) and overall['b3_recall'] == 1.0
    assert overall['h_sys_ref'] == 0.0 and overall['h_ref_sys'] == pytest.approx(0.4, rel=1e-14)      # 200 of 500 frames: 1 bit


def test_refusals(corpus, capsys):
    from vbx_amd import metrics
    ref, hyp = str(corpus / 'ref.rttm'), str(corpus / 'sys.rttm')
    with pytest.raises(SystemExit):                                          # no UEM
        metrics.main(['-r', ref, '-s', hyp, '-u', 'all.uem'])
    assert 'not supported' in capsys.readouterr().err
    (corpus / 'stray.rttm').write_text(rttm_text('recZ', [(0.0, 1.0, 1)]))
    with pytest.raises(ValueError, match='recZ'):
        metrics.score_rttm(ref, [hyp, str(corpus / 'stray.rttm')])
    with pytest.raises(SystemExit):
        metrics.main(['-r', ref, '-s', hyp, str(corpus / 'stray.rttm')])
    assert 'recZ' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        metrics.main(['-r', ref, '-s', hyp, '--step', '0'])
    assert '--step' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        metrics.main(['--help'])
    text = capsys.readouterr().out
    assert all(w in text for w in ('JER', 'B3-Precision', 'GKT(ref, sys)', 'NMI', '--step', '--collar', '--ignore_overlaps'))


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_listed_and_built_from_its_header():
    from vbx_amd import _capi, build, metrics
    header = open(os.path.join(REPO, 'include', 'vbx_hip.h')).read()
    assert re.search(r'\bint vbx_frame_counts\s*\(', header) and 'vbx_frame_counts' in _capi.ABI_SYMBOLS
    assert '#define VBX_ABI_VERSION 7' in header
    assert 'vbx_frame_score.hpp' in build.HEADERS and 'vbx_frame_score.hpp' not in build.ITERATION_SOURCES
    src = open(os.path.join(build.CSRC, 'vbx_frame_score.hpp')).read()
    const = {k: int(v) for k, v in re.findall(r'constexpr int (kFrm\w+) = (\d+);', src)}
    assert (_capi.FRAME_BLOCK, _capi.FRAME_MAX_SPEAKERS, _capi.FRAME_MAX_CLASSES) == (const['kFrmBlock'], const['kFrmMaxSpk'], const['kFrmMaxCls'])
    assert (metrics.MAX_DEVICE_SPEAKERS, metrics.MAX_DEVICE_CLASSES) == (const['kFrmMaxSpk'], const['kFrmMaxCls'])
    assert 'atomic' not in src.split('#pragma once')[1]                      # integer sums, one thread per entry
    assert '#include "vbx_frame_score.hpp"' in open(os.path.join(build.CSRC, 'vbx_capi.hip')).read()
