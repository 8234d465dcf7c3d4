"""``vbx_amd.tune`` and ``score.score_labels`` without a GPU: the numpy route against the exact referee ``tests/score_ref.py`` and
against hand cases worked out below; the grid order, the pooled figure and the tie rule; the refusals and the parser; the whole
flow on the stand-in host stages of ``tests/test_driver.py``; the new entry point in the header and the ABI list.
"""
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import score_ref
from score_util import assert_within_bound
from test_driver import OracleStages, _write_inputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- score_labels(device=None) against the referee --------------------------------------------------------------------------
def sliding_windows(seed, T, step=0.24, win=1.44, n_spk=3):
    """T overlapping windows as the x-vector extractor cuts them, some VAD gaps, labels in runs; reference turns of its own"""
    rng = np.random.default_rng(seed)
    starts = np.round(np.cumsum(np.where(rng.random(T) < 0.1, rng.uniform(1.5, 3.0, T), step)), 3)
    ends = np.round(starts + win, 3)
    labels = np.repeat(rng.integers(0, n_spk, T), rng.integers(1, 6, T))[:T]
    ref = [(round(float(b), 3), round(float(b + d), 3), f'r{s}') for b, d, s in
           zip(rng.uniform(0, ends[-1], 25), rng.uniform(0.2, 8.0, 25), rng.integers(0, 3, 25))]
    return ref, starts, ends, labels


@pytest.mark.parametrize('collar,ignore', [(0.0, False), (0.25, False), (0.25, True)])
def test_numpy_route_within_the_rounding_bound_of_the_referee(collar, ignore):
    from vbx_amd import score
    items = [sliding_windows(seed, T) for seed, T in ((1, 1), (2, 2), (3, 40), (4, 257))]
    hyps = [[it[3], (it[3] + 1) % 3, np.zeros_like(it[3])] for it in items]
    got = score.score_labels([(it[0], it[1], it[2], h) for it, h in zip(items, hyps)], collar, ignore)
    assert [len(g) for g in got] == [3] * 4
    for k, (it, hs) in enumerate(zip(items, hyps)):
        for j, labels in enumerate(hs):
            turns = score.labels_turns(it[1], it[2], labels)
            exact = score_ref.score_exact([(Fraction(str(b)), Fraction(str(e)), s) for b, e, s in it[0]],
                                          [(Fraction(b), Fraction(e), s) for b, e, s in turns], Fraction(str(collar)), ignore)
            assert_within_bound(got[k][j], exact, f'item {k} hypothesis {j}')
            assert got[k][j]['sys_speakers'] == sorted({int(l) for l in labels}, key=str)
            # the definition: score_turns on the turns of merge_adjacent_labels
            same = score.score_turns([(it[0], turns)], collar, ignore)[0]
            assert all(np.float64(same[key]).tobytes() == np.float64(got[k][j][key]).tobytes() for key in ('der', 'miss', 'fa', 'confusion', 'ref_time'))


# ---- hand cases -------------------------------------------------------------------------------------------------------------
def test_overlapping_windows_meet_in_the_middle():
    """Windows of 1.44 s every 0.24 s, labels A B A: [0, 1.44] [0.24, 1.68] [0.48, 1.92].  Neighbours with different labels
    overlap, so they meet at (1.44 + 0.24) / 2 = 0.84 and (1.68 + 0.48) / 2 = 1.08: turns A [0, 0.84], B [0.84, 1.08],
    A [1.08, 1.92].  Against the reference x [0, 0.8], y [0.8, 1.1], x [1.1, 1.92]: A speaks 0.04 s and then 0.02 s
    of y -> confusion 0.06 s of 1.92 s, no miss, no false alarm: DER 3.125."""
    from vbx_amd import score
    starts, ends, labels = [0.0, 0.24, 0.48], [1.44, 1.68, 1.92], [0, 1, 0]
    turns = score.labels_turns(starts, ends, labels)
    assert [t[2] for t in turns] == [0, 1, 0]
    assert (turns[0][1], turns[1][0]) == ((1.44 + 0.24) / 2.0,) * 2 and (turns[1][1], turns[2][0]) == ((1.68 + 0.48) / 2.0,) * 2
    assert turns[0][1] == pytest.approx(0.84, abs=1e-12) and turns[1][1] == pytest.approx(1.08, abs=1e-12)
    ref = [(0.0, 0.8, 'x'), (0.8, 1.1, 'y'), (1.1, 1.92, 'x')]
    got = score.score_labels([(ref, starts, ends, [labels])])[0][0]
    assert got['der'] == pytest.approx(3.125, abs=1e-9) and got['confusion'] == pytest.approx(0.06, abs=1e-12)
    assert got['miss'] == pytest.approx(0.0, abs=1e-12) and got['fa'] == pytest.approx(0.0, abs=1e-12)
    assert got['mapping'] == {'x': 0, 'y': 1} and got['sys_speakers'] == [0, 1]


def test_a_gap_isclose_closes_and_one_it_does_not():
    """np.isclose(end, start): |end - start| <= 1e-8 + 1e-5 |start|.
    At t = 3000 s the tolerance is 0.03 s: [2999, 3000] and [3000.02, 3001] with one label are ONE turn [2999, 3001]; against
    the reference [2999, 3001] nothing is missed.  At t = 1 s the tolerance is 1.001e-5 s: [0, 1] and [1.001, 2] stay TWO turns;
    against the reference [0, 2] the gap of 0.001 s is missed: DER 100 * 0.001 / 2 = 0.05.  A gap of 5e-6 s there is closed."""
    from vbx_amd import score
    far = score.labels_turns([2999.0, 3000.02], [3000.0, 3001.0], [4, 4])
    assert far == [(2999.0, 3001.0, 4)]
    rec = score.score_labels([([(2999.0, 3001.0, 'x')], [2999.0, 3000.02], [3000.0, 3001.0], [[4, 4]])])[0][0]
    assert (rec['miss'], rec['fa'], rec['confusion'], rec['ref_time'], rec['der']) == (0.0, 0.0, 0.0, 2.0, 0.0)
    near = score.labels_turns([0.0, 1.001], [1.0, 2.0], [4, 4])
    assert near == [(0.0, 1.0, 4), (1.001, 2.0, 4)]
    rec = score.score_labels([([(0.0, 2.0, 'x')], [0.0, 1.001], [1.0, 2.0], [[4, 4]])])[0][0]
    assert rec['miss'] == pytest.approx(0.001, abs=1e-12) and rec['der'] == pytest.approx(0.05, abs=1e-9)
    assert score.labels_turns([0.0, 1.000005], [1.0, 2.0], [4, 4]) == [(0.0, 2.0, 4)]
    assert score.labels_turns([0.0, 1.000005], [1.0, 2.0], [4, 5]) == [(0.0, 1.0, 4), (1.000005, 2.0, 5)]       # labels differ: a cut


def test_score_labels_shapes_and_refusals():
    from vbx_amd import score
    assert score.score_labels([]) == [] and score.score_labels([([(0.0, 1.0, 'x')], [0.0], [1.0], [])]) == [[]]
    with pytest.raises(ValueError, match='collar'):
        score.score_labels([], collar=-1.0)
    empty = score.score_labels([([(0.0, 1.0, 'x')], [], [], [[]])])[0][0]              # no segment: all miss
    assert empty['der'] == 100.0 and empty['sys_speakers'] == []


# ---- grid order, pooled figure, tie rule ------------------------------------------------------------------------------------
def test_grid_order_pool_and_ties():
    from vbx_amd import score, tune
    assert tune.grid_points([0.2, 0.3], [11, 17], [0.9, 0.99]) == [(0.2, 11.0, 0.9), (0.2, 11.0, 0.99), (0.2, 17.0, 0.9), (0.2, 17.0, 0.99),
                                                                  (0.3, 11.0, 0.9), (0.3, 11.0, 0.99), (0.3, 17.0, 0.9), (0.3, 17.0, 0.99)]
    with pytest.raises(ValueError, match='empty'):
        tune.grid_points([0.3], [], [0.9])
    with pytest.raises(ValueError, match='loopP'):
        tune.grid_points([0.3], [17], [1.5])
    nan = float('nan')
    assert tune.best_point([dict(der=5.0), dict(der=3.0), dict(der=3.0), dict(der=4.0)]) == 1        # the first of the equals
    assert tune.best_point([dict(der=nan), dict(der=7.0), dict(der=nan)]) == 1 and tune.best_point([dict(der=nan)] * 2) == 0
    # pooled: times, not rates: (10 + 5) / (100 + 10) = 13.64 %, not the mean 30 % of the two rates
    recs = [dict(miss=10.0, fa=0.0, confusion=0.0, ref_time=100.0, der=10.0), dict(miss=0.0, fa=0.0, confusion=5.0, ref_time=10.0, der=50.0)]
    result = dict(grid=[(0.3, 17.0, 0.99), (0.4, 17.0, 0.99)], names=['a', 'b'], records=[recs, recs[:1]],
                  pooled=[score._pool(recs), score._pool(recs[:1])], best=1, timing={})
    assert result['pooled'][0]['der'] == 100.0 * 15.0 / 110.0
    lines = tune.format_table(result).splitlines()
    assert lines[0].split() == ['Fa', 'Fb', 'loopP', 'DER', 'Miss', 'FA', 'Conf']
    assert lines[1].split() == ['0.3', '17', '0.99', '13.64', '9.09', '0.00', '4.55']
    assert lines[2].split() == ['0.4', '17', '0.99', '10.00', '10.00', '0.00', '0.00']
    assert lines[3] == 'best: Fa=0.4 Fb=17 loopP=0.99 DER=10.00' and len(lines) == 4
    doc = tune.to_json(result)
    assert doc['best']['index'] == 1 and doc['points'][0]['recordings']['b']['der'] == 50.0 and json.dumps(doc)


# ---- parser and refusals ----------------------------------------------------------------------------------------------------
def argv_of(paths, ref, extra=()):
    return ['--xvec-ark-file', paths['ark'], '--segments-file', paths['seg'], '--xvec-transform', paths['transform'], '--plda-file',
            paths['plda'], '--threshold', '-0.015', '--lda-dim', '128', '--ref-rttm-dir', ref] + list(extra)


def test_parser_defaults_and_help(capsys):
    from vbx_amd import tune
    none = dict(ark='a', seg='s', transform='t', plda='p')
    args = tune.build_parser().parse_args(argv_of(none, 'ref', ['--Fa', '0.2', '0.3', '--Fb', '17', '--loopP', '0.9', '0.99']))
    assert (args.Fa, args.Fb, args.loopP) == ([0.2, 0.3], [17.0], [0.9, 0.99])
    assert (args.collar, args.ignore_overlaps, args.out_json, args.best_rttm_dir) == (0.25, False, None, None)
    assert (args.precision, args.ahc_scores, args.init_smoothing, args.target_energy) == ('fp64', 'cos', 5.0, 1.0)
    with pytest.raises(SystemExit):                                   # the reference directory is required
        tune.build_parser().parse_args(argv_of(none, 'ref')[:-2] + ['--Fa', '0.3', '--Fb', '17', '--loopP', '0.9'])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        tune.main(['--help'])
    text = capsys.readouterr().out
    assert all(flag in text for flag in ('--Fa', '--Fb', '--loopP', '--out-json', '--best-rttm-dir', '--collar', '--ignore_overlaps'))
    assert 'TURNS, not RTTM TEXT' in text and 'six decimals' in text and '1 us per system boundary' in text


def test_refusals(tmp_path, capsys, monkeypatch):
    from vbx_amd import tune
    none = dict(ark='none.ark', seg='none.seg', transform='none.h5', plda='none')
    grid = ['--Fa', '0.3', '--Fb', '17', '--loopP', '0.99']
    with pytest.raises(SystemExit):                                   # a missing reference directory, before anything is read
        tune.main(argv_of(none, str(tmp_path / 'nowhere'), grid))
    assert 'no such directory' in capsys.readouterr().err
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit):
        tune.main(argv_of(none, str(tmp_path), grid))
    assert 'more than one rank' in capsys.readouterr().err
    with pytest.raises(ValueError, match='more than one rank'):
        tune.tune(tune.build_parser().parse_args(argv_of(none, str(tmp_path), grid)))
    monkeypatch.setenv('WORLD_SIZE', '1')
    with pytest.raises(ValueError, match='empty'):
        tune.tune_recordings([], {}, {}, None, [], {})


# ---- the whole flow on host stages ------------------------------------------------------------------------------------------
def test_tune_end_to_end_on_host_stages(tmp_path, capsys, monkeypatch):
    from vbx_amd import score, tune, vbhmm
    paths = _write_inputs(tmp_path)
    g = np.load(os.path.join(REPO, 'tests', 'golden', 'driver_split3.npz'))
    ref_dir = tmp_path / 'ref'                                       # the reference: the RTTM the reference driver wrote
    ref_dir.mkdir()
    for rec in ('recA', 'recB', 'recC'):
        (ref_dir / f'{rec}.rttm').write_bytes(g['rttm_' + rec].tobytes())
    points = [(0.3, 17.0, 0.99), (0.3, 17.0, 0.2)]
    extra = ['--Fa', '0.3', '--Fb', '17', '--loopP', '0.99', '0.2', '--out-json', str(tmp_path / 'tune.json'), '--best-rttm-dir',
             str(tmp_path / 'best')]
    args = tune.build_parser().parse_args(argv_of(paths, str(ref_dir), extra))
    stages = OracleStages()
    result = tune.tune(args, stages=stages, log=lambda *a: None)
    assert result['grid'] == points and result['names'] == ['recA', 'recB', 'recC'] and stages.vb_calls == 2
    assert capsys.readouterr().out == ''
    # every point: the labels and the files of the driver run at that point; the figures of the numpy route on those labels;
    # the pooled DER within the rounding of the RTTM text of what the driver's --ref-rttm-dir step reports
    for gi, (Fa, Fb, loopP) in enumerate(points):
        out = str(tmp_path / f'vbhmm{gi}')
        vargs = vbhmm.build_parser().parse_args(['--init', 'AHC+VB', '--out-rttm-dir', out] + argv_of(paths, str(ref_dir))
                                                + ['--Fa', str(Fa), '--Fb', str(Fb), '--loopP', str(loopP)])
        capsys.readouterr()
        state, _ = vbhmm.diarize(vargs, stages=OracleStages(), log=lambda *a: None)
        table = capsys.readouterr().out
        n_turns = 0
        for k, name in enumerate(result['names']):
            assert np.array_equal(result['labels'][gi][k], state[name]['labels1st']), (gi, name)
            n_turns += len(open(os.path.join(out, name + '.rttm')).read().splitlines())
        written, overall = score.score_written(out, result['names'], str(ref_dir), 0.25, False)
        assert table == score.format_table(written, overall) + '\n'
        pooled = result['pooled'][gi]
        assert pooled == score._pool(result['records'][gi]) and pooled['ref_time'] > 0
        bound = 100.0 * 3 * 2 * n_turns * 1e-6 / overall['ref_time']
        print(f'point {gi}: tune {pooled["der"]!r}, text {overall["der"]!r}, bound {bound:.3e}')
        assert abs(pooled['der'] - overall['der']) <= bound
        if gi == result['best']:
            best = {f: open(os.path.join(out, f), 'rb').read() for f in sorted(os.listdir(out))}
    assert result['best'] == tune.best_point(result['pooled'])
    assert {f: open(tmp_path / 'best' / f, 'rb').read() for f in sorted(os.listdir(tmp_path / 'best'))} == best and len(best) == 3
    # the reference IS the output at the first point: nothing but the rounding of its text is left there
    assert result['best'] == 0 and result['pooled'][0]['der'] < 1e-3
    doc = json.load(open(tmp_path / 'tune.json'))
    assert [(p['Fa'], p['Fb'], p['loopP']) for p in doc['points']] == points
    assert doc['best']['index'] == 0 and doc['collar'] == 0.25 and set(doc['points'][0]['recordings']) == {'recA', 'recB', 'recC'}
    assert doc['points'][1]['pooled']['der'] == result['pooled'][1]['der']
    # the program prints the table and nothing else
    monkeypatch.setattr(tune, 'tune', lambda a, log=print: result)
    capsys.readouterr()
    assert tune.main(argv_of(paths, str(ref_dir), extra)) == 0
    assert capsys.readouterr().out == tune.format_table(result) + '\n'


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_listed_and_built_from_its_header():
    from vbx_amd import _capi, build
    header = open(os.path.join(REPO, 'include', 'vbx_hip.h')).read()
    assert re.search(r'\bint vbx_labels_score\s*\(', header) and 'vbx_labels_score' in _capi.ABI_SYMBOLS
    assert '#define VBX_ABI_VERSION 7' in header
    assert 'vbx_labels_score.hpp' in build.HEADERS and 'vbx_labels_score.hpp' not in build.ITERATION_SOURCES
    capi = open(os.path.join(build.CSRC, 'vbx_capi.hip')).read()
    assert capi.index('#include "vbx_rttm_score.hpp"') < capi.index('#include "vbx_labels_score.hpp"')
    src = open(os.path.join(build.CSRC, 'vbx_labels_score.hpp')).read()
    const = {k: int(v) for k, v in re.findall(r'constexpr int (kLab\w+) = (\d+);', src)}
    assert _capi.LABELS_BLOCK == const['kLabBlock'] and const['kLabInfo'] == 4
    assert 'atomic' not in src.split('#pragma once')[1]                      # scans and sums in a fixed order
    assert '__dmul_rn' in src and '__dadd_rn' in src                         # isclose's tolerance: two roundings, no FMA
