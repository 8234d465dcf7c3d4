"""The device path of ``vbx_amd.score`` (vbx_rttm_score.hpp: rttm_cells / rttm_acc / rttm_fin behind vbx_rttm_score) against
the exact referee ``tests/score_ref.py``, and the ``--ref-rttm-dir`` step of the two drivers.

Kernel inputs are dyadic: every turn time is a multiple of 2^-10 s below 2^12 s and so is the collar.  Every cell length,
every product with a speaker count and every partial sum (below 64 * 2^12 s, in units of 2^-10: 2^28) is then exact in
float64, so the device's numbers must EQUAL the referee's -- no tolerance.  Shapes sit at each constant of the header and one
either side of it.  Where sums do round (millisecond decimals) a pair is held to the referee's rounding bound, and to the same
bytes wherever it stands in a batch.
"""
import os
from fractions import Fraction

import numpy as np
import pytest

import diarize_util as du
import score_ref
from score_util import KEYS, assert_within_bound, random_pair

pytestmark = pytest.mark.gpu
Q = 2.0 ** -10                     # the grid of the dyadic inputs
SPAN = 2 ** 22                     # grid points below 2^12 s


def constants():
    from vbx_amd import _capi
    return _capi.RTTM_CLS_BLOCK, _capi.RTTM_TURN_CHUNK, _capi.RTTM_GROUP_CELLS, _capi.RTTM_ACC_CHUNK, _capi.RTTM_MAX_SPEAKERS


def dyadic_pair(seed, sides, n_ref, n_sys, extras=0):
    """A pair with exactly len(sides) cells (at collar 0): len(sides) + 1 random grid points cut [lo, hi] into intervals, and
    interval i is one turn of the reference (sides[i] == 0) or of the system (1).  The speakers 0 .. ceil(n / 2) - 1 of a side
    take its interval turns in rotation (so all occur once the side has that many turns); the other speakers take ``extras``
    long turns each between two of the grid points, which overlap whatever lies under them.  -> (ref turns, sys turns)."""
    rng = np.random.default_rng(seed)
    pts = np.sort(rng.choice(SPAN, size=len(sides) + 1, replace=False)) * Q
    n = (n_ref, n_sys)
    short = [(n_ref + 1) // 2, (n_sys + 1) // 2]
    out, used = ([], []), [0, 0]
    for i, s in enumerate(sides):
        out[s].append((float(pts[i]), float(pts[i + 1]), f'{"rs"[s]}{used[s] % short[s]:02d}'))
        used[s] += 1
    for s in (0, 1):
        for spk in range(short[s], n[s]):
            for _ in range(max(extras, 1)):
                a, b = sorted(rng.choice(len(pts), size=2, replace=False))
                out[s].append((float(pts[a]), float(pts[b]), f'{"rs"[s]}{spk:02d}'))
    return out


def assert_equal_to_referee(got, ref, hyp, collar=0.0, ignore_overlaps=False, cells=None):
    exact = score_ref.score_exact(ref, hyp, Fraction(collar), ignore_overlaps)
    if cells is not None:
        assert exact['n_cells'] == cells                           # (the shape this case is about)
    for key in KEYS:
        assert Fraction(got[key]) == exact[key], (key, got[key], float(exact[key]))
    names = {(r, s): got['C'][i, j] for i, r in enumerate(got['ref_speakers']) for j, s in enumerate(got['sys_speakers'])}
    assert set(names) == set(exact['C'])
    wrong = [(k, names[k], float(v)) for k, v in exact['C'].items() if Fraction(float(names[k])) != v]
    assert not wrong, wrong[:5]
    if exact['der'] is None:
        assert np.isnan(got['der'])
    else:                                                          # the same float expression on the same (exact) floats
        assert got['der'] == 100.0 * (float(exact['miss']) + float(exact['fa']) + float(exact['confusion'])) / float(exact['ref_time'])
    return exact


def alternate(n, first=0):
    return [(first + i) % 2 for i in range(n)]


def cell_counts():
    cls, _, group, acc, _ = constants()
    return sorted({1, 2, cls - 1, cls, cls + 1, acc - 1, acc, acc + 1, group - 1, group, group + 1, 2 * group + 1})


def score_all_cases():
    """Every dyadic shape case scored in ONE call per protocol (what the entry point is for), looked up by the tests."""
    from vbx_amd import score
    cls, chunk, group, acc, maxspk = constants()
    cases = {}
    for k, cells in enumerate(cell_counts()):                      # cells per pair; two speakers a side, one of them long turns
        cases[f'cells{cells}'] = (dyadic_pair(100 + k, alternate(cells, k), 2, 2), cells)
    # turns per pair: one turn; the LDS chunk -+ 1 in total, and with the reference / system split either side of the cut
    cases['turns1'] = (dyadic_pair(200, [0], 1, 0), 1)
    for k, (nr, ns) in enumerate([(chunk - 2, 1), (chunk - 1, 1), (chunk, 1), (1, chunk), (chunk + 1, chunk - 1), (3, chunk + 40)]):
        cases[f'turns{nr}+{ns}'] = (dyadic_pair(210 + k, [0] * nr + [1] * ns, 1, 1), nr + ns)
    # speakers per side
    for k, (nr, ns) in enumerate([(1, 1), (8, 8), (9, 9), (32, 32), (33, 33), (maxspk, maxspk), (maxspk, 1), (1, maxspk), (33, 8)]):
        cases[f'spk{nr}x{ns}'] = (dyadic_pair(300 + k, alternate(2 * max(nr, ns) + 7), nr, ns, extras=2), 2 * max(nr, ns) + 7)
    cases['spk65'] = (dyadic_pair(400, alternate(150), maxspk + 1, 3, extras=1), 150)       # runs on the host path
    names = list(cases)
    out = {}
    for proto, kw in PROTOCOLS.items():
        records = score.score_turns([cases[n][0] for n in names], device=0, **kw)
        out[proto] = dict(zip(names, records))
    return cases, out


@pytest.fixture(scope='module')
def device_records():
    return score_all_cases()


PROTOCOLS = {'full': dict(collar=0.0, ignore_overlaps=False), 'collar': dict(collar=256 * Q, ignore_overlaps=False),
             'forgiving': dict(collar=300 * Q, ignore_overlaps=True)}


def case_names():
    cls, chunk, group, acc, maxspk = constants()
    names = [f'cells{c}' for c in cell_counts()] + ['turns1']
    names += [f'turns{a}+{b}' for a, b in [(chunk - 2, 1), (chunk - 1, 1), (chunk, 1), (1, chunk), (chunk + 1, chunk - 1), (3, chunk + 40)]]
    names += [f'spk{a}x{b}' for a, b in [(1, 1), (8, 8), (9, 9), (32, 32), (33, 33), (maxspk, maxspk), (maxspk, 1), (1, maxspk), (33, 8)]]
    return names + ['spk65']


@pytest.mark.parametrize('proto', list(PROTOCOLS))
@pytest.mark.parametrize('name', case_names())
def test_device_totals_equal_the_referee_bit_for_bit(name, proto, device_records):
    cases, records = device_records
    (ref, hyp), cells = cases[name]
    kw = PROTOCOLS[proto]
    got = records[proto][name]
    exact = assert_equal_to_referee(got, ref, hyp, kw['collar'], kw['ignore_overlaps'], cells if proto == 'full' else None)
    if name.startswith('spk'):
        nr, ns = (65, 3) if name == 'spk65' else (int(v) for v in name[3:].split('x'))
        assert (len(got['ref_speakers']), len(got['sys_speakers'])) == (nr, ns)
    if proto == 'full':
        assert exact['ref_time'] > 0


def test_edge_pairs():
    from vbx_amd import score
    ref3 = [(1.0, 9.0, 'A'), (2.0, 8.0, 'B'), (3.0, 7.0, 'C'), (9.0, 12.0, 'B')]
    hyp3 = [(1.0, 5.0, 1), (5.0, 12.0, 2)]
    tight = ([(1.0, 1.25, 'A'), (1.25, 1.5, 'B')], [(1.0, 1.5, 1)])
    pairs = [([(1.0, 4.0, 'A'), (3.0, 6.5, 'B')], []),              # no system turn: all miss
             ([], [(0.5, 2.0, 1), (1.0, 3.0, 2)]),                  # no reference turn: nothing to divide by
             tight,                                                 # collar 0.5 leaves no scored cell
             (ref3, hyp3),                                          # three reference speakers at once
             ([], []),                                              # nothing at all
             ([(2.0, 2.0, 'A')], [(3.0, 1.0, 1)])]                  # turns of no and of negative duration only
    for kw in (dict(collar=0.0), dict(collar=0.5), dict(collar=0.0, ignore_overlaps=True), dict(collar=0.25, ignore_overlaps=True)):
        got = score.score_turns(pairs, device=0, **kw)
        for (ref, hyp), g in zip(pairs, got):
            assert_equal_to_referee(g, ref, hyp, kw['collar'], kw.get('ignore_overlaps', False))
    full = score.score_turns(pairs, device=0)
    assert (full[0]['miss'], full[0]['ref_time'], full[0]['der']) == (6.5, 6.5, 100.0)
    assert np.isnan(full[1]['der']) and full[1]['fa'] == 3.5 and full[1]['ref_time'] == 0.0
    assert np.isnan(full[4]['der']) and np.isnan(full[5]['der']) and full[4]['C'].shape == (0, 0)
    wide = score.score_turns(pairs, collar=0.5, device=0)
    assert np.isnan(wide[2]['der']) and wide[2]['ref_time'] == 0.0 and not wide[2]['C'].any()
    # [3, 7] has three speakers, [2, 3] and [7, 8] two: with overlaps ignored [1, 2], [8, 9] of A and [9, 12] of B are left
    lone = score.score_turns(pairs, ignore_overlaps=True, device=0)[3]
    assert lone['ref_time'] == 5.0 and score.score_turns(pairs, device=0)[3]['ref_time'] == 8.0 + 6.0 + 4.0 + 3.0


def decimal_pairs():
    """37 pairs with millisecond decimals and mixed shapes: sums that round, several groups, empty sides, many speakers"""
    _, _, group, _, maxspk = constants()
    shapes = [(2, 2, 30), (4, 3, 300), (1, 1, 1), (6, 5, 80), (3, 9, 700), (maxspk, 40, 200), (2, 2, group // 2 + 20)]
    pairs = []
    for k in range(37):
        n_ref, n_sys, n_turns = shapes[k % len(shapes)]
        (ref, _), (hyp, _) = random_pair(500 + k, n_ref, n_sys, n_turns, seconds=600)
        pairs.append(([], hyp) if k == 11 else (ref, []) if k == 23 else (ref, hyp))
    return pairs


def test_a_pair_has_the_same_bytes_wherever_it_stands_in_a_batch():
    from vbx_amd import score
    _, _, group, _, _ = constants()
    collar, ignore = 0.25, False
    (ref, _), (hyp, _) = random_pair(77, 5, 7, group + 100, seconds=900)               # two boundaries a turn and side: > 2 groups
    probe = score._Pair(ref, hyp, collar)
    assert probe.edges.size - 1 > 2 * group
    others = [score._Pair(r, h, collar) for r, h in decimal_pairs()]
    assert len(others) == 37 and any(p.edges.size - 1 > group for p in others)

    def run(batch, at):
        tot, C = score._device_totals(batch, collar, ignore, 0)[at]
        return tot.tobytes() + C.tobytes()
    alone = run([probe], 0)
    assert np.frombuffer(alone, dtype=np.float64)[0] > 0
    assert run([probe] + others[1:], 0) == alone
    assert run(others[:-1] + [probe], 36) == alone
    assert run(others[:18] + [probe] + others[19:], 18) == alone
    assert run([probe, probe], 1) == alone and run([probe], 0) == alone               # and from run to run


def test_decimal_inputs_within_the_rounding_bound():
    from vbx_amd import score
    _, _, group, _, _ = constants()
    (ref, ref_x), (hyp, hyp_x) = random_pair(78, 4, 5, group + 100, seconds=900)
    for collar, ignore in ((0.0, False), (0.25, False), (0.25, True)):
        got = score.score_turns([(ref, hyp)], collar=collar, ignore_overlaps=ignore, device=0)[0]
        exact = score_ref.score_exact(ref_x, hyp_x, Fraction(str(collar)), ignore)
        assert exact['n_cells'] > 2 * group
        assert_within_bound(got, exact, f'collar {collar} ignore {ignore}')


def test_entry_point_refuses_bad_arguments():
    from vbx_amd import _capi
    ctx = _capi.default_context(0)
    edges, turns = np.array([0.0, 1.0]), np.array([[0.0, 1.0], [0.0, 1.0]])
    ok = _capi.rttm_score(ctx, [[2, 1, 1, 1, 1]], edges, turns, [0, 0], 0.0, False)
    assert ok.tolist() == [1.0, 0.0, 0.0, 1.0, 1.0]
    with pytest.raises(_capi.VbxError, match='speaker 1 of turn 1'):                   # an index that would be a row past C
        _capi.rttm_score(ctx, [[2, 1, 1, 1, 1]], edges, turns, [0, 1], 0.0, False)
    with pytest.raises(_capi.VbxError, match='at most 64'):
        _capi.rttm_score(ctx, [[2, 1, 1, 65, 1]], edges, turns, [0, 0], 0.0, False)
    with pytest.raises(_capi.VbxError, match='collar'):
        _capi.rttm_score(ctx, [[2, 1, 1, 1, 1]], edges, turns, [0, 0], -1.0, False)
    assert _capi.rttm_score(ctx, [[2, 1, 1, 1, 1]], edges, turns, [0, 0], 0.0, False).tolist() == ok.tolist()


# ---- the drivers ----------------------------------------------------------------------------------------------------------
THRESHOLD, FA, FB = 0.0, 4.0, 1.0             # (tests/test_gpu_diarize.py: what keeps the generated voices apart)


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    """two short generated recordings, their true turns as reference RTTM files with millisecond decimals"""
    tmp = tmp_path_factory.mktemp('score')
    a, b = du.synth_recording(21, 16000, 12, 2), du.synth_recording(22, 8000, 12, 2)
    p = du.write_corpus(tmp, {'recA': (a[0], 16000, a[1]), 'recB': (b[0], 8000, b[1])})
    p.update(du.write_models(tmp), ckpt=du.write_checkpoint(tmp), tmp=str(tmp), ref=str(tmp / 'ref'))
    os.makedirs(p['ref'])
    for name, turns in (('recA', a[2]), ('recB', b[2])):
        with open(os.path.join(p['ref'], name + '.rttm'), 'w') as f:
            f.write(''.join(f'SPEAKER {name} 1 {s:.3f} {e - s:.3f} <NA> <NA> voice{v} <NA> <NA>\n' for s, e, v in turns))
    return p


# The drivers run in ONE fresh child process (PyTorch has to start the GPU runtime itself, as in tests/test_gpu_diarize.py): both
# routes with and without the flag, what each printed and returned kept for the tests below.
DRIVER_CALLS = r"""
import contextlib, io, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
p = json.load(open(sys.argv[2]))
from vbx_amd import diarize, vbhmm


def captured(fn, *args, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = fn(*args, **kw)
    return res, buf.getvalue()


def plain(state):
    return {n: {k: None if v is None else np.asarray(v).tolist() for k, v in st.items()} for n, st in state.items()}


def files(out, **kw):
    (state, timing), printed = captured(diarize.diarize_files, ['recA', 'recB'], p['wav'], p['lab'], p['ckpt'], p['transform'], p['plda'],
                                        out_rttm_dir=out, threshold=p['threshold'], Fa=p['Fa'], Fb=p['Fb'], batch_size=16, **kw)
    return dict(state=plain(state), timing=sorted(timing), printed=printed)


def argv(out, extra=()):
    return ['--init', 'AHC+VB', '--out-rttm-dir', out, '--xvec-ark-file', p['ark'], '--segments-file', p['seg'], '--xvec-transform',
            p['transform'], '--plda-file', p['plda'], '--threshold', str(p['threshold']), '--lda-dim', '128', '--Fa', str(p['Fa']),
            '--Fb', str(p['Fb']), '--loopP', '0.99'] + list(extra)


def program(out, extra=()):
    rc, printed = captured(vbhmm.main, argv(out, extra))
    return dict(rc=rc, printed=printed)


def library(out, extra=()):
    (state, timing), printed = captured(vbhmm.diarize, vbhmm.build_parser().parse_args(argv(out, extra)))
    return dict(state=plain(state), timing=sorted(timing), printed=printed)


res = {}
res['files_plain'] = files(p['out'] + '/files_plain', out_ark_fn=p['ark'], out_seg_fn=p['seg'])
res['files_scored'] = files(p['out'] + '/files_scored', ref_rttm_dir=p['ref'], collar=0.25, ignore_overlaps=True)
try:
    files(None, ref_rttm_dir=p['ref'])
except ValueError as exc:
    res['files_no_out'] = str(exc)
res['main_plain'] = program(p['out'] + '/main_plain')
res['main_scored'] = program(p['out'] + '/main_scored', ['--ref-rttm-dir', p['ref']])        # default protocol: collar 0.25
res['lib_plain'] = library(p['out'] + '/lib_plain')
res['lib_scored'] = library(p['out'] + '/lib_scored', ['--ref-rttm-dir', p['ref'], '--collar', '0.5', '--ignore_overlaps'])
json.dump(res, open(p['json'], 'w'))
print('driver calls OK')
"""


@pytest.fixture(scope='module')
def driven(corpus):
    import json
    import subprocess
    import sys
    p = dict(corpus, out=os.path.join(corpus['tmp'], 'out'), ark=os.path.join(corpus['tmp'], 'x.ark'),
             seg=os.path.join(corpus['tmp'], 'x.seg'), json=os.path.join(corpus['tmp'], 'res.json'), threshold=THRESHOLD, Fa=FA, Fb=FB)
    with open(os.path.join(corpus['tmp'], 'p.json'), 'w') as f:
        json.dump(p, f)
    res = subprocess.run([sys.executable, '-c', DRIVER_CALLS, du.REPO, os.path.join(corpus['tmp'], 'p.json')],
                         env=dict(os.environ, PYTHONPATH=du.REPO), cwd=du.REPO, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and 'driver calls OK' in res.stdout, res.stderr[-3000:]
    return p, json.load(open(p['json']))


def assert_scored_as_the_command_scores(state, table, out, p, collar, ignore, capsys):
    """every der in the state is score_rttm's on the files as written, and the table is what vbx_amd.score prints for them"""
    from vbx_amd import score
    refs, outs = ([os.path.join(d, f'{n}.rttm') for n in ('recA', 'recB')] for d in (p['ref'], out))
    records, overall = score.score_rttm(refs, outs, collar=collar, ignore_overlaps=ignore, device=0)
    for name in ('recA', 'recB'):
        assert np.float64(state[name]['der']).tobytes() == np.float64(records[name]['der']).tobytes(), name
        assert records[name]['ref_time'] > 0
    capsys.readouterr()
    assert score.main(['-r'] + refs + ['-s'] + outs + ['--collar', str(collar), '--device', '0'] + (['--ignore_overlaps'] if ignore else [])) == 0
    assert capsys.readouterr().out == table
    assert table.splitlines()[0].split() == ['File', 'DER', 'Miss', 'FA', 'Conf'] and '*** OVERALL ***' in table


def assert_only_der_is_new(plain, scored):
    """without the flag: the same timing keys and, but for der, the same state"""
    assert plain['timing'] == scored['timing'] and list(plain['state']) == list(scored['state']) == ['recA', 'recB']
    for name, st in plain['state'].items():
        assert 'der' not in st and set(scored['state'][name]) == set(st) | {'der'}
        assert all(scored['state'][name][key] == value for key, value in st.items()), name


def test_diarize_files_scores_what_it_wrote(driven, capsys):
    p, res = driven
    plain, scored = res['files_plain'], res['files_scored']
    out0, out1 = p['out'] + '/files_plain', p['out'] + '/files_scored'
    assert plain['printed'] == ''                                  # nothing printed, and the same files
    assert du.rttm_dir(out0) == du.rttm_dir(out1) and sorted(du.rttm_dir(out0)) == ['recA.rttm', 'recB.rttm']
    assert_only_der_is_new(plain, scored)
    assert_scored_as_the_command_scores(scored['state'], scored['printed'], out1, p, 0.25, True, capsys)
    assert 'out_rttm_dir' in res['files_no_out']


def test_vbhmm_scores_what_it_wrote(driven, capsys):
    p, res = driven
    out = {k: p['out'] + '/' + k for k in ('main_plain', 'main_scored', 'lib_plain', 'lib_scored', 'files_plain')}
    assert res['main_plain']['rc'] == res['main_scored']['rc'] == 0
    files = du.rttm_dir(out['main_plain'])
    assert sorted(files) == ['recA.rttm', 'recB.rttm'] and files == du.rttm_dir(out['files_plain'])
    assert all(du.rttm_dir(out[k]) == files for k in ('main_scored', 'lib_plain', 'lib_scored'))
    # the program: the flag adds the table to what is printed and nothing else
    printed0, printed1 = res['main_plain']['printed'], res['main_scored']['printed']
    assert printed1.startswith(printed0) and 'DER' not in printed0
    # the library call: der into the state; the table under the program's default protocol and under the flags given
    assert_only_der_is_new(res['lib_plain'], res['lib_scored'])
    assert res['lib_plain']['printed'] == printed0
    table = res['lib_scored']['printed'][len(printed0):]
    assert_scored_as_the_command_scores(res['lib_scored']['state'], table, out['lib_scored'], p, 0.5, True, capsys)
    from vbx_amd import score
    refs, outs = ([os.path.join(d, f'{n}.rttm') for n in ('recA', 'recB')] for d in (p['ref'], out['main_scored']))
    records, overall = score.score_rttm(refs, outs, collar=0.25, ignore_overlaps=False, device=0)
    assert printed1[len(printed0):] == score.format_table(records, overall) + '\n'
