"""The device route of ``metrics.frame_counts_labels`` / ``metrics.score_labels`` (vbx_labels_frame.hpp: labels_turns_kernel,
labels_frames_kernel and the frame kernels of vbx_frame_score.hpp on what they wrote) against the numpy route of the same
module, against the dense referee ``tests/metrics_ref.py`` and against the existing device route ``metrics.frame_counts(device)``
on the turns numpy's ``merge_adjacent_labels`` gives; ``python -m vbx_amd.tune --criterion jer`` against ``vbx_amd.vbhmm`` point
by point.

The counts are integers: everything must be EQUAL, no tolerance.  Shapes sit at every pass boundary of the scans (kLabBlock)
and of the frame kernels (kFrmBlock), one either side.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import metrics_ref
import tune_util
from metrics_util import CLASSES_OVER_CAP
from test_gpu_labels_score import GRID, build_cases, grid_argv, reference, segments
from test_tune_metrics_host import DECIMAL_LAYOUTS, HAND_ONE, HAND_REF, HAND_STARTS, HAND_ENDS, HAND_THREE, assert_same_record, decimal_items

pytestmark = pytest.mark.gpu
COUNT_KEYS = ('ref_speakers', 'sys_speakers', 'ref_durs', 'sys_durs', 'inter', 'ref_classes', 'sys_classes', 'cm')
HOST_ROUTE = ('S65', 'nref65', 'classes_over_cap')      # more than 64 speakers a side, more than 256 reference classes


def touching(T, frames=2, t0=1.0):
    """T segments of `frames` frames back to back from t0: with alternating labels T turns, T + 1 distinct frame indices"""
    s = np.round(t0 + 0.01 * frames * np.arange(T), 2)
    return s, np.round(s + 0.01 * frames, 2)


def entries_case(n_ref, n_sys):
    """n_ref reference speakers one after the other, n_sys labels one after the other over the same extent: n_ref and n_sys
    classes, a result of n_ref + n_sys + 2 n_ref n_sys entries"""
    s, e = touching(2 * n_sys, 3, 0.0)
    cut = np.round(np.linspace(0.0, e[-1], n_ref + 1), 3)
    cut[-1] = e[-1]
    return [(cut[i], cut[i + 1], f'r{i:02d}') for i in range(n_ref)], s, e, np.arange(2 * n_sys) // 2


def build_all():
    """name -> (reference turns, starts, ends, labels)"""
    cases = dict(build_cases())                   # T at 1, 2, 127 .. 513, one label, alternating, runs on the block edge in the
    #                                               four layouts, a label without duration, 1 .. 65 labels, 64 and 65 reference speakers
    for n, item in zip(DECIMAL_LAYOUTS, decimal_items()):                       # 0.07, 0.29, 0.57 as starts and as ends
        for j, labels in enumerate(item[3]):
            cases[f'decimal_{n}_{j}'] = (item[0], item[1], item[2], labels)
    for n, item in zip(DECIMAL_LAYOUTS, decimal_items(1234.5)):                 # a recording that starts at 1234.5 s
        cases[f'late_{n}'] = (item[0], item[1], item[2], item[3][0])
    # boundaries of a hypothesis: 2 (1 reference turn + T turns) + 2 = 254, 256, 258; one reference turn round everything:
    # T + 3 distinct frame indices, T + 2 cells: 255, 256, 257 and 511, 512, 513
    for T in (125, 126, 127, 253, 254, 255, 509, 510, 511):
        s, e = touching(T)
        cases[f'cells_{T + 2}'] = ([(0.5, e[-1] + 0.5, 'x')], s, e, np.arange(T) % 2)
    for n_ref, n_sys in ((3, 36), (13, 9), (2, 51)):                            # 255, 256, 257 result entries
        cases[f'entries_{n_ref + n_sys + 2 * n_ref * n_sys}'] = entries_case(n_ref, n_sys)
    # label 1's only turn [0.4711, 0.4712) falls between the frame times 0.47 and 0.48: a speaker without a frame
    cases['shorter_than_a_frame'] = ([(0.0, 1.0, 'A'), (0.123, 0.127, 'C'), (1.0, 2.0, 'B')], [0.0, 0.4711, 0.4712], [0.4711, 0.4712, 2.0],
                                     np.array([0, 1, 0]))
    s, e = touching(60, 10, 0.0)
    cases['three_overlapping'] = ([(0.0, 3.0, 'A'), (1.0, 4.0, 'B'), (2.0, 5.0, 'C')], s, e, np.arange(60) // 7 % 3)
    cases['no_reference'] = ([], s, e, np.arange(60) // 7 % 3)
    cases['reference_outside_the_segments'] = ([(0.0, 0.5, 'A'), (7.0, 9.0, 'B')], s + 1.0, e + 1.0, np.arange(60) // 7 % 2)
    s, e = touching(64, 16, 0.0)                                                # 10.24 s under 512 reference classes
    cases['classes_over_cap'] = (CLASSES_OVER_CAP[0], s, e, np.arange(64) // 5 % 3)
    cases['hand_one'] = (HAND_REF, HAND_STARTS, HAND_ENDS, HAND_ONE)
    cases['hand_three'] = (HAND_REF, HAND_STARTS, HAND_ENDS, HAND_THREE)
    return {k: (v[0], np.asarray(v[1], dtype=np.float64), np.asarray(v[2], dtype=np.float64), np.asarray(v[3])) for k, v in cases.items()}


def case_names():
    return list(build_all())


@pytest.fixture(scope='module')
def counted():
    """every case: ONE frame_counts_labels call on the device, the numpy route, and the existing device route on numpy's turns"""
    from vbx_amd import metrics, score
    cases = build_all()
    names = list(cases)
    items = [(cases[n][0], cases[n][1], cases[n][2], [cases[n][3]]) for n in names]
    turns = {n: score.labels_turns(*cases[n][1:]) for n in names}
    dev = {n: g[0] for n, g in zip(names, metrics.frame_counts_labels(items, device=0))}
    host = {n: g[0] for n, g in zip(names, metrics.frame_counts_labels(items, device=None))}
    old = dict(zip(names, metrics.frame_counts([(cases[n][0], turns[n]) for n in names], device=0)))
    return cases, turns, dev, host, old


@pytest.mark.parametrize('name', case_names())
def test_label_sequences_equal_numpy_the_referee_and_the_turn_route(name, counted):
    cases, turns, dev, host, old = counted
    got = dev[name]
    assert set(got) == set(COUNT_KEYS)
    want = metrics_ref.counts(cases[name][0], turns[name])
    metrics_ref.assert_counts_equal(got, want, name)
    assert_same_record(got, host[name], name)
    assert_same_record(got, old[name], name)                         # the bytes of metrics.frame_counts(device) on numpy's turns
    if name == 'zero_length_only':
        assert 7 not in got['sys_speakers'] and got['sys_speakers'] == [0, 1]
    elif name == 'shorter_than_a_frame':
        assert got['sys_speakers'] == [0, 1] and got['sys_durs'].tolist() == [200, 0] and got['ref_durs'].tolist() == [100, 100, 0]
    elif name.startswith('S') and name[1:].isdigit():
        assert len(got['sys_speakers']) == int(name[1:])
    elif name.startswith('nref'):
        assert len(got['ref_speakers']) == int(name[4:])
    elif name.startswith('entries_'):
        assert got['ref_durs'].size + got['sys_durs'].size + got['inter'].size + got['cm'].size == int(name[8:])
    elif name == 'classes_over_cap':
        assert len(got['ref_classes']) == 512
    elif name == 'no_reference':
        assert got['ref_speakers'] == [] and got['cm'].shape[0] == 1 and got['sys_durs'].sum() == 600
    elif name == 'hand_three':
        assert got['cm'].tolist() == [[6000, 3000, 0], [0, 0, 1000]] and got['sys_classes'] == [(0,), (2,), (1,)]


# ---- the entry point itself -------------------------------------------------------------------------------------------------
def raw(recs, hyps, step=0.01):
    """vbx_labels_frame_counts on recs = [(reference turns, starts, ends)] and hyps = [(recording, labels, n_sys)]
    -> ([the bytes that came back per hypothesis], info [n_hyp][4], masks [n_hyp])"""
    from vbx_amd import _capi, metrics
    refs = [metrics._LabelsFrames(r, s, e, step) for r, s, e in recs]
    assert all(r.ok for r in refs)
    info, classes, flat, masks = _capi.labels_frame_counts(
        _capi.default_context(0), [(r.starts.size, r.rs.size, len(r.ref_names)) for r in refs],
        np.concatenate([a for r in refs for a in (r.starts, r.ends)]), np.concatenate([r.turns for r in refs]),
        np.concatenate([r.rs for r in refs]), [(h[0], h[2]) for h in hyps], np.concatenate([np.asarray(h[1], dtype=np.int32) for h in hyps]), step)
    out, off = [], 0
    for k, (rec, _lab, n_sys) in enumerate(hyps):
        n_ref = len(refs[rec].ref_names)
        fits = info[k][1] <= 256 and info[k][2] <= 256
        n = n_ref + n_sys + n_ref * n_sys + (int(info[k][1]) * int(info[k][2]) if fits else 0)
        out.append(info[k].tobytes() + classes[k].tobytes() + flat[off:off + n].tobytes() + masks[k].tobytes())
        off += n
    return out, info, masks


def test_cells_classes_and_masks_that_came_back(counted):
    """the cells are as many as the distinct frame indices numpy finds less one; a label that never occurs is a zero column and
    no bit of the mask; the classes are the host route's"""
    from vbx_amd import metrics
    cases, turns, dev, host, old = counted
    names = [n for n in cases if n not in HOST_ROUTE]
    recs = [cases[n][:3] for n in names]
    hyps = [(k, cases[n][3], min(int(cases[n][3].max()) + 2, 64)) for k, n in enumerate(names)]        # one label more than occur
    _, info, masks = raw(recs, hyps)
    for n, inf, mask in zip(names, info, masks.tolist()):
        p = metrics._Frames(cases[n][0], turns[n])
        nf = p.n_frames(0.01)
        u = np.unique(np.concatenate([metrics._frame_index(a, 0.01, nf) for a in (p.rb, p.re, p.sb, p.se, [p.lo, p.hi])]))
        assert inf[0] == u.size - 1, n
        assert (inf[1], inf[2]) == (len(dev[n]['ref_classes']), len(dev[n]['sys_classes'])), n
        assert [s for s in range(64) if mask >> s & 1] == sorted(dev[n]['sys_speakers']), n
        if n.startswith('cells_'):
            assert inf[0] == int(n[6:]), n


def test_a_hypothesis_has_the_same_bytes_wherever_it_stands_in_a_batch():
    B = 256
    rng = np.random.default_rng(5)
    recs = []
    for k, (layout, T) in enumerate([('overlap', 2 * B + 77), ('gaps', 40), ('touching', B), ('identical', 3 * B), ('overlap', 1)]):
        s, e = segments(layout, T, 400 + k)
        ref = [(round(b + 0.0007, 4), round(x + 0.0013, 4), spk) for b, x, spk in reference(500 + k, s[0], e[-1], 4, 30)]
        recs.append((ref, s, e))

    def random_hyp(r):
        T = recs[r][1].size
        S = int(rng.integers(1, 9))
        return (r, np.repeat(rng.integers(0, S, T), rng.integers(1, 7, T))[:T], S)
    probe = (0, np.repeat(rng.integers(0, 5, 2 * B + 77), rng.integers(1, 3, 2 * B + 77))[:2 * B + 77], 5)
    others = [random_hyp(k % len(recs)) for k in range(40)]
    alone, info, _ = raw(recs[:1], [probe])
    assert info[0][0] > B and info[0][2] > 1                         # more cells than one block, more than one system class
    assert raw(recs, [probe] + others)[0][0] == alone[0]
    assert raw(recs, others + [probe])[0][40] == alone[0]
    assert raw(recs, others[:20] + [probe] + others[20:])[0][20] == alone[0]
    same_rec = [probe if k == 7 else random_hyp(0) for k in range(16)]                          # 16 hypotheses of one recording
    assert raw(recs[:1], same_rec)[0][7] == alone[0]
    assert raw(recs[:1], [probe, probe])[0] == [alone[0], alone[0]] and raw(recs[:1], [probe])[0] == alone


def test_score_labels_is_score_turns_on_the_turns():
    """the whole record, DER part and columns, in one call for several recordings and hypotheses; other steps"""
    from vbx_amd import metrics, score
    cases = build_all()
    names = ['runs_overlap', 'random_gaps', 'decimal_identical_0', 'late_overlap', 'three_overlapping', 'S65', 'classes_over_cap', 'no_reference']
    items = [(cases[n][0], cases[n][1], cases[n][2], [cases[n][3], (cases[n][3] + 1) % 2]) for n in names]
    for collar, ignore, step in ((0.25, False, 0.01), (0.0, True, 0.003)):
        timing = {}
        got = metrics.score_labels(items, collar, ignore, step, device=0, timing=timing)
        assert {'prepare', 'device', 'mapping'} <= set(timing)
        want = metrics.score_turns([(it[0], score.labels_turns(it[1], it[2], lab)) for it in items for lab in it[3]], collar, ignore, step, device=0)
        for k, n in enumerate(names):
            for j in range(2):
                assert_same_record(got[k][j], want[2 * k + j], f'{n} hypothesis {j}')
                metrics_ref.assert_counts_equal(got[k][j], metrics_ref.counts(items[k][0], score.labels_turns(*items[k][1:3], items[k][3][j]), step), n)


def test_entry_point_refuses_bad_arguments():
    """all of these are refused on the host, before anything is launched"""
    from vbx_amd import _capi
    ctx = _capi.default_context(0)
    rec, seg, turns, spk = [[2, 1, 1]], [0.0, 1.0, 1.0, 2.0], [[0.0, 2.0]], [0]

    def call(rec=rec, seg=seg, turns=turns, spk=spk, hyp=((0, 2),), labels=(0, 1), step=0.01):
        return _capi.labels_frame_counts(ctx, rec, seg, turns, spk, list(hyp), list(labels), step)
    info, classes, out, masks = call()
    # 200 frames, one reference class, two system classes: ref_durs, sys_durs, inter [1][2], cm [1][2]
    assert info.tolist() == [[2, 1, 2, 0]] and masks.tolist() == [3]
    assert out[:7].tolist() == [200, 100, 100, 100, 100, 100, 100] and classes[0, 1, :3].tolist() == [1, 2, 0] and classes[0, 0, :2].tolist() == [1, 0]
    for match, kw in (('label 2 of segment 1 outside', dict(labels=(0, 2))), ('label -1 of segment 0 outside', dict(labels=(-1, 0))),
                      ('times decrease at segment 1', dict(seg=[1.0, 0.5, 2.0, 2.5])), ('times decrease at segment 1', dict(seg=[0.0, 0.5, 2.0, 1.5])),
                      ('no positive finite duration', dict(seg=[0.0, 1.0, 1.0, 1.0])), ('no positive finite duration', dict(seg=[0.0, 1.0, 1.0, float('nan')])),
                      ('speaker 1 of reference turn 0', dict(spk=[1])), ('not a finite interval', dict(turns=[[2.0, 0.0]])),
                      ('not a finite interval', dict(turns=[[0.0, float('inf')]])), ('at most 64', dict(hyp=((0, 65),))),
                      ('at most 64', dict(rec=[[2, 1, 65]])), ('2\\^40 frames', dict(step=1e-13)), ('step', dict(step=0.0)),
                      ('step', dict(step=float('nan')))):
        with pytest.raises(_capi.VbxError, match=match):
            call(**kw)

    def direct(rec=rec, seg=seg, turns=turns, spk=spk, hyp=((0, 2),), labels=(0, 1), cap=64, keep=('info', 'classes', 'out', 'masks')):
        f64 = lambda a: None if a is None else np.array(a, dtype=np.float64)
        i32 = lambda a: None if a is None else np.array(a, dtype=np.int32)
        arrays = [i32(rec), f64(seg), f64(turns), i32(spk), i32(hyp), i32(labels)]               # (alive during the call)
        res = dict(info=np.zeros(4, dtype=np.int32), classes=np.zeros(512, dtype=np.uint64), out=np.zeros(64, dtype=np.int64), masks=np.zeros(1, dtype=np.uint64))
        ptr = [_capi._ptr(a) for a in arrays]
        ctx.check(ctx._lib.vbx_labels_frame_counts(ctx._h, 1, *ptr[:4], 1, *ptr[4:], 0.01, *[_capi._ptr(res[k]) if k in keep else None for k in ('info', 'classes')],
                                                   _capi._ptr(res['out']) if 'out' in keep else None, cap, _capi._ptr(res['masks']) if 'masks' in keep else None),
                  'vbx_labels_frame_counts')
        return res
    assert direct()['out'][:7].tolist() == out[:7].tolist()
    for match, kw in (('names recording 1 of 1', dict(hyp=((1, 2),))), ('negative or oversized count', dict(rec=[[2, -1, 1]])),
                      ('negative or oversized count', dict(rec=[[-2, 1, 1]])), ('negative or oversized count', dict(hyp=((0, -1),))),
                      ('bad argument', dict(seg=None)), ('bad argument', dict(hyp=None)), ('bad argument', dict(labels=None)),
                      ('bad argument', dict(keep=('info', 'classes', 'out'))), ('bad argument', dict(keep=('classes', 'out', 'masks'))),
                      ('bad argument', dict(cap=-1)), ('NULL argument', dict(turns=None))):
        with pytest.raises(_capi.VbxError, match=match):
            direct(**kw)
    with pytest.raises(_capi.VbxError, match='out has room for 6'):  # refused after the first phase, as vbx_frame_counts refuses it
        direct(cap=6)
    again = call()                                                    # and the context still works
    assert again[0].tolist() == info.tolist() and again[2][:7].tobytes() == out[:7].tobytes() and again[3].tolist() == [3]


# ---- the driver -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tuned(tmp_path_factory):
    """--criterion jer: the library call, the program in a fresh child process, and the driver run at every grid point"""
    from vbx_amd import tune, vbhmm
    tmp = tmp_path_factory.mktemp('tune_jer')
    p = tune_util.make_dev_set(tmp, 3, 120, seed=3)
    argv = tune_util.data_argv(p) + grid_argv() + ['--criterion', 'jer']
    lib_args = tune.build_parser().parse_args(argv + ['--best-rttm-dir', str(tmp / 'best_lib'), '--out-json', str(tmp / 'lib.json')])
    result = tune.tune(lib_args, log=lambda *a: None)
    child = subprocess.run([sys.executable, '-m', 'vbx_amd.tune'] + argv + ['--best-rttm-dir', str(tmp / 'best_cli'), '--out-json', str(tmp / 'cli.json')],
                           env=dict(os.environ, PYTHONPATH=tune_util.REPO), cwd=tune_util.REPO, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-3000:]
    runs = []
    for gi, (Fa, Fb, loopP) in enumerate(result['grid']):
        out = str(tmp / f'vbhmm{gi}')
        vargs = vbhmm.build_parser().parse_args(['--init', 'AHC+VB', '--out-rttm-dir', out] + tune_util.data_argv(p)[:-2]
                                                + ['--Fa', str(Fa), '--Fb', str(Fb), '--loopP', str(loopP)])
        state, _ = vbhmm.diarize(vargs, log=lambda *a: None)
        runs.append(dict(out=out, state=state))
    return p, tmp, result, child.stdout, runs


def test_tune_by_jer_equals_the_driver_and_score_turns_at_every_grid_point(tuned):
    from vbx_amd import metrics, score, tune
    from vbx_amd.kaldi_formats import read_xvector_timing_dict
    p, tmp, result, printed, runs = tuned
    assert result['grid'] == tune.grid_points(**GRID) and len(runs) == 8 and result['names'] == p['names']
    assert result['criterion'] == 'jer' and result['step'] == 0.010
    ref = {n: score.read_turns(os.path.join(p['ref'], n + '.rttm'))[n] for n in p['names']}
    segs = read_xvector_timing_dict(p['seg'])
    pairs = []
    for g, run in enumerate(runs):
        for k, n in enumerate(p['names']):
            assert np.array_equal(result['labels'][g][k], run['state'][n]['labels1st']), (g, n)          # integer equality
            pairs.append((ref[n], score.labels_turns(*segs[n][1].T, result['labels'][g][k])))
    want = metrics.score_turns(pairs, 0.25, False, 0.010, device=0)
    for g in range(8):
        for k, n in enumerate(p['names']):
            assert_same_record(result['records'][g][k], want[3 * g + k], f'point {g} {n}')
        pooled = metrics._overall(result['records'][g])
        assert all(np.float64(result['pooled'][g][c]).tobytes() == np.float64(pooled[c]).tobytes() for c in metrics.COLUMNS)
    best = result['best']
    jer = [r['jer'] for r in result['pooled']]
    print('pooled JER per point:', jer, 'pooled DER per point:', [r['der'] for r in result['pooled']])
    assert best == tune.best_point(result['pooled'], 'jer') == jer.index(min(jer))
    files = {f: open(os.path.join(runs[best]['out'], f), 'rb').read() for f in sorted(os.listdir(runs[best]['out']))}
    for d in ('best_lib', 'best_cli'):
        assert {f: open(tmp / d / f, 'rb').read() for f in sorted(os.listdir(tmp / d))} == files and len(files) == 3
    # the program: the eleven-column table of the library call, and the same JSON but for the timings
    assert printed == tune.format_table(result) + '\n' and printed.splitlines()[-1].startswith('best: Fa=') and ' JER=' in printed.splitlines()[-1]
    assert len(printed.splitlines()) == 10 and 'B3-Precision' in printed.splitlines()[0] and 'NMI' in printed.splitlines()[0]
    lib, cli = json.load(open(tmp / 'lib.json')), json.load(open(tmp / 'cli.json'))
    assert lib['points'] == cli['points'] and lib['best'] == cli['best'] and lib['best']['index'] == best and len(lib['points']) == 8
    assert lib['criterion'] == cli['criterion'] == 'jer' and lib['step'] == 0.010 and set(metrics.COLUMNS) <= set(lib['points'][0]['pooled'])
