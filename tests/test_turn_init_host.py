"""``--init RTTM`` / ``--init RTTM+VB`` without a GPU: the referee of tests/turn_init_ref.py against cases worked by hand, the
ticks, the command lines, the files that may be missing, the driver's route around AHC and the C header.  The device side is
tests/test_gpu_turn_init.py."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest

import turn_init_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VBHMM = ['--out-rttm-dir', 'out', '--xvec-ark-file', 'x.ark', '--segments-file', 'x.seg', '--xvec-transform', 't.h5', '--plda-file',
         'plda', '--threshold', '-0.015', '--lda-dim', '128', '--Fa', '0.3', '--Fb', '17', '--loopP', '0.99']
DIARIZE = ['--gpus', '0', '--checkpoint', 'c.pth', '--in-file-list', 'l.txt', '--in-lab-dir', 'lab', '--in-wav-dir', 'wav',
           '--out-rttm-dir', 'out', '--xvec-transform', 't.h5', '--plda-file', 'plda', '--threshold', '-0.015', '--lda-dim', '128',
           '--Fa', '0.3', '--Fb', '17', '--loopP', '0.99']
TUNE = ['--xvec-ark-file', 'x.ark', '--segments-file', 'x.seg', '--xvec-transform', 't.h5', '--plda-file', 'plda', '--threshold',
        '-0.015', '--lda-dim', '128', '--Fa', '0.3', '--Fb', '17', '--loopP', '0.99', '--ref-rttm-dir', 'ref']

# ---- the referee against cases worked by hand ----------------------------------------------------------------------------
# Every case: the SPEAKER lines (start, duration, speaker) in seconds, ONE window (start, end), and by hand: S, the overlaps
# d in microseconds, the weights and the label.  tests/test_gpu_turn_init.py places the same cases at the edges of a block.
HAND = {
    'inside one turn': dict(lines=[(0.0, 10.0, 'A'), (10.0, 5.0, 'B')], window=(2.0, 3.5), S=2, d=[1500000, 0], w=[1.0, 0.0], label=0),
    'half in A, half in B': dict(lines=[(0.0, 3.0, 'A'), (3.0, 4.0, 'B')], window=(2.0, 4.0), S=2, d=[1000000, 1000000], w=[0.5, 0.5],
                                 label=0),
    'A and B overlapped throughout': dict(lines=[(0.0, 9.0, 'A'), (1.0, 5.0, 'B')], window=(2.0, 3.0), S=2, d=[1000000, 1000000],
                                          w=[0.5, 0.5], label=0),
    'only touches a turn': dict(lines=[(5.0, 1.0, 'A'), (1.0, 2.0, 'B')], window=(3.0, 5.0), S=2, d=[0, 0], w=[1.0, 0.0], label=0),
    'equidistant between 1 and 0': dict(lines=[(6.0, 1.0, 'A'), (1.0, 1.0, 'B')], window=(3.0, 5.0), S=2, d=[0, 0], w=[1.0, 0.0],
                                        label=0),
    'nearer to 1': dict(lines=[(6.5, 1.0, 'A'), (1.0, 1.0, 'B')], window=(3.0, 5.0), S=2, d=[0, 0], w=[0.0, 1.0], label=1),
    'overlapping turns of one speaker': dict(lines=[(0.0, 3.0, 'A'), (2.0, 3.0, 'A'), (0.0, 1.0, 'B'), (3.5, 1.0, 'B')],
                                             window=(2.0, 4.0), S=2, d=[2000000, 500000], w=[0.8, 0.2], label=0),
    'a turn of no duration': dict(lines=[(2.5, 0.0, 'Z'), (0.0, 2.5, 'A'), (2.5, 1.0, 'B')], window=(2.0, 3.0), S=3,
                                  d=[0, 500000, 500000], w=[0.0, 0.5, 0.5], label=1),
    'numbered by first appearance': dict(lines=[(4.0, 1.0, 'zed'), (0.0, 4.0, 'abe'), (5.0, 1.0, 'zed')], window=(3.0, 4.5), S=2,
                                         d=[500000, 1000000], w=[1.0 / 3.0, 2.0 / 3.0], label=1),
    'three speakers by duration': dict(lines=[(0.0, 1.0, 'A'), (1.0, 2.0, 'B'), (3.0, 1.0, 'C')], window=(0.5, 3.25), S=3,
                                       d=[500000, 2000000, 250000], w=[500000 / 2750000, 2000000 / 2750000, 250000 / 2750000], label=1),
}


def hand_case(name):
    """(a, b, u, v, spk, S) of one hand-worked case, through the referee's parser."""
    c = HAND[name]
    u, v, spk, S = ref.prepare(c['lines'])
    a, b = ref.windows([c['window']])
    return a, b, u, v, spk, S


@pytest.mark.parametrize('name', sorted(HAND))
def test_the_referee_gives_the_hand_worked_rows(name):
    c = HAND[name]
    a, b, u, v, spk, S = hand_case(name)
    assert S == c['S']
    labels, w, d = ref.weights(a, b, u, v, spk, S)
    assert d.tolist() == [c['d']] and labels.tolist() == [c['label']]
    assert w.tolist() == [c['w']]                                  # (bit for bit: one division of exact integers)
    q = ref.qinit(w, 5.0)
    assert abs(q.sum() - 1.0) < 1e-15 and int(np.argmax(q[0])) == c['label']
    if max(c['w']) == 1.0:                                         # the reference's softmax(init_smoothing * onehot(label))
        z = np.exp(-5.0)
        onehot = np.where(np.arange(S) == c['label'], 1.0, z) / (1.0 + (S - 1) * z)
        assert np.allclose(q[0], onehot, rtol=0, atol=1e-16)
    elif c['w'] == [0.5, 0.5]:
        assert q.tolist() == [[0.5, 0.5]]


def test_the_merged_turns_of_a_speaker_are_not_counted_twice_and_touching_turns_become_one():
    u, v, spk, S = ref.prepare(HAND['overlapping turns of one speaker']['lines'])
    assert (u.tolist(), v.tolist(), spk.tolist(), S) == ([0, 0, 3500000], [5000000, 1000000, 4500000], [0, 1, 1], 2)
    u, v, spk, S = ref.prepare([(0.0, 1.0, 'A'), (1.0, 1.0, 'A'), (2.000001, 1.0, 'A')])
    assert (u.tolist(), v.tolist(), spk.tolist(), S) == ([0, 2000001], [2000000, 3000001], [0, 0], 1)
    with pytest.raises(ValueError):
        ref.prepare([(1.0, 0.0, 'A'), (2.0, -1.0, 'B')])


def test_the_host_parser_gives_the_referees_turns():
    from vbx_amd import turn_init
    for name in sorted(HAND):
        u, v, spk, names = turn_init.turn_ticks(HAND[name]['lines'], 'rec')
        ru, rv, rspk, S = ref.prepare(HAND[name]['lines'])
        assert (u.tolist(), v.tolist(), spk.tolist(), len(names)) == (ru.tolist(), rv.tolist(), rspk.tolist(), S), name
        assert u.dtype == v.dtype == np.int64 and spk.dtype == np.int32
        assert names == list(ref.rename_by_first_appearance([l[2] for l in HAND[name]['lines']]))
    a, b = turn_init.window_ticks([[0.1 + 0.2, 1.74], [0.24, 1.68]])
    assert (a.tolist(), b.tolist()) == ([300000, 240000], [1740000, 1680000]) and a.dtype == b.dtype == np.int64


# ---- ticks ---------------------------------------------------------------------------------------------------------------
def test_ticks_land_where_the_decimal_text_says():
    from vbx_amd import turn_init
    for tick in (ref.tick, turn_init.tick):
        assert tick(0.1 + 0.2) == 300000 and 0.1 + 0.2 != 0.3
        assert tick(1.005) == 1005000                          # (1.005 is below 1.005 as a double; the product rounds up)
        assert tick(0.24 * 7) == 1680000 and tick(0.1 * 3) == 300000
        assert tick(305.26) == 305260000 and tick(306.59) - tick(305.26) == 1330000
        assert tick(0.0000004) == 0 and tick(0.0000006) == 1
        assert tick(123456.789012) == 123456789012
        assert isinstance(tick(2.5), int)
    # a turn ends at u + tick(duration), not at tick(start + duration): both parsers
    u, v, _spk, _S = ref.prepare([(0.1, 0.2, 'A')])
    assert (u.tolist(), v.tolist()) == ([100000], [300000])
    u, v, _spk, _names = turn_init.turn_ticks([(0.1, 0.2, 'A')])
    assert (u.tolist(), v.tolist()) == ([100000], [300000])


# ---- the command lines ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('init', ['RTTM', 'RTTM+VB'])
def test_vbhmm_and_diarize_take_both_inits_and_warn_once_about_the_ahc_options(init, capsys):
    from vbx_amd import diarize, vbhmm
    p = vbhmm.build_parser()
    args = p.parse_args(['--init', init, '--init-rttm-dir', 'first'] + VBHMM)
    vbhmm.check_init_arguments(args, p.error)
    err = capsys.readouterr().err
    assert len(err.splitlines()) == 1 and all(w in err for w in ('warning', '--threshold', '--ahc-scores', '--target-energy', 'ignored'))
    assert args.init == init and args.init_rttm_dir == 'first' and args.random_restarts is None and args.seed is None
    args = diarize.parse_args(['--init', init, '--init-rttm-dir', 'first'] + DIARIZE)
    assert args.init == init and args.init_rttm_dir == 'first'
    assert len(capsys.readouterr().err.splitlines()) == 1
    assert vbhmm.random_init_states(init) is None and vbhmm.turn_init(init) and not vbhmm.runs_ahc(init)
    assert vbhmm.runs_vb(init) == (init == 'RTTM+VB')


def test_the_other_inits_are_what_they_were(capsys):
    from vbx_amd import vbhmm
    assert [vbhmm.random_init_states(i) for i in ('AHC', 'AHC+VB', 'random_7')] == [None, None, 7]
    assert [vbhmm.runs_vb(i) for i in ('AHC', 'AHC+VB', 'random_7')] == [False, True, True]
    assert [vbhmm.turn_init(i) for i in ('AHC', 'AHC+VB', 'random_7')] == [False] * 3
    assert [vbhmm.runs_ahc(i) for i in ('AHC', 'AHC+VB', 'random_7')] == [True, True, False]
    p = vbhmm.build_parser()
    vbhmm.check_init_arguments(p.parse_args(['--init', 'AHC+VB'] + VBHMM), p.error)
    assert capsys.readouterr().err == ''
    with pytest.raises(SystemExit):
        p.parse_args(['--init', 'RTTM+AHC'] + VBHMM)
    err = capsys.readouterr().err
    assert 'invalid choice' in err and 'random_<N>' in err and 'RTTM+VB' in err
    with pytest.raises(ValueError, match='random_<N>'):
        vbhmm.random_init_states('rttm')


def test_tune_takes_rttm_vb_and_refuses_rttm_alone():
    from vbx_amd import tune
    p = tune.build_parser()
    args = p.parse_args(TUNE + ['--init', 'RTTM+VB', '--init-rttm-dir', 'first'])
    assert tune.check_init(args) == (None, 1, 0) and args.init_rttm_dir == 'first'
    with pytest.raises(ValueError, match='runs no VB-HMM'):
        tune.check_init(p.parse_args(TUNE + ['--init', 'RTTM', '--init-rttm-dir', 'first']))
    with pytest.raises(ValueError, match='--init-rttm-dir'):
        tune.check_init(p.parse_args(TUNE + ['--init', 'RTTM+VB']))
    with pytest.raises(ValueError, match='--init-rttm-dir'):
        tune.check_init(p.parse_args(TUNE + ['--init-rttm-dir', 'first']))             # (the default, AHC+VB)
    with pytest.raises(ValueError, match='--init-rttm-dir'):
        tune.check_init(p.parse_args(TUNE + ['--init', 'random_3', '--init-rttm-dir', 'first']))
    with pytest.raises(ValueError, match='random_<N>'):
        tune.check_init(p.parse_args(TUNE + ['--init', 'RTTM+VB', '--init-rttm-dir', 'first', '--seed', '3']))


@pytest.mark.parametrize('init', ['AHC', 'AHC+VB', 'random_4'])
def test_the_directory_is_refused_without_the_two_inits(init, capsys):
    from vbx_amd import diarize, vbhmm
    p = vbhmm.build_parser()
    with pytest.raises(SystemExit) as exc:
        vbhmm.check_init_arguments(p.parse_args(['--init', init, '--init-rttm-dir', 'first'] + VBHMM), p.error)
    err = capsys.readouterr().err
    assert exc.value.code == 2 and '--init-rttm-dir needs --init RTTM or RTTM+VB' in err
    with pytest.raises(SystemExit):
        diarize.parse_args(['--init', init, '--init-rttm-dir', 'first'] + DIARIZE)
    assert '--init-rttm-dir needs --init RTTM or RTTM+VB' in capsys.readouterr().err


@pytest.mark.parametrize('init', ['RTTM', 'RTTM+VB'])
def test_the_two_inits_are_refused_without_the_directory(init, capsys):
    from vbx_amd import diarize, vbhmm
    p = vbhmm.build_parser()
    with pytest.raises(SystemExit) as exc:
        vbhmm.check_init_arguments(p.parse_args(['--init', init] + VBHMM), p.error)
    assert exc.value.code == 2 and f'--init {init} needs --init-rttm-dir' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        diarize.parse_args(['--init', init] + DIARIZE)
    assert f'--init {init} needs --init-rttm-dir' in capsys.readouterr().err
    with pytest.raises(ValueError, match='needs --init-rttm-dir'):
        diarize.diarize_files(['a'], 'wav', 'lab', 'c.pth', 't.h5', 'plda', init=init)
    with pytest.raises(ValueError, match='no such directory'):
        diarize.diarize_files(['a'], 'wav', 'lab', 'c.pth', 't.h5', 'plda', init=init, init_rttm_dir='/nowhere/at/all')
    with pytest.raises(ValueError, match='needs --init RTTM'):
        diarize.diarize_files(['a'], 'wav', 'lab', 'c.pth', 't.h5', 'plda', init='AHC+VB', init_rttm_dir='first')


# ---- the files -----------------------------------------------------------------------------------------------------------
def test_what_is_missing_is_named(tmp_path):
    from vbx_amd import turn_init
    with pytest.raises(ValueError, match='nowhere'):
        turn_init.read_init_turns(str(tmp_path / 'nowhere'), 'recA')
    with pytest.raises(ValueError, match='--init-rttm-dir'):
        turn_init.read_init_turns(None, 'recA')
    with pytest.raises(ValueError, match=r'recA\.rttm'):
        turn_init.read_init_turns(str(tmp_path), 'recA')
    (tmp_path / 'recA.rttm').write_text('SPEAKER recB 1 0.0 1.0 <NA> <NA> x <NA> <NA>\nSPKR-INFO recA 1 <NA> <NA> <NA> unknown x <NA> <NA>\n')
    with pytest.raises(ValueError, match='no SPEAKER line for recording recA'):
        turn_init.read_init_turns(str(tmp_path), 'recA')
    (tmp_path / 'recC.rttm').write_text('SPEAKER recC 1 1.0 0.0 <NA> <NA> x <NA> <NA>\nSPEAKER recC 1 2.0 -0.5 <NA> <NA> y <NA> <NA>\n')
    with pytest.raises(ValueError, match='recC'):
        turn_init.read_init_turns(str(tmp_path), 'recC')
    (tmp_path / 'recB.rttm').write_text('SPEAKER recB 1 0.1 0.2 <NA> <NA> x <NA> <NA>\nSPEAKER other 1 0.0 9.0 <NA> <NA> y <NA> <NA>\n'
                                        'SPEAKER recB 1 0.3 0.5 <NA> <NA> x <NA> <NA>\n')
    u, v, spk, names = turn_init.read_init_turns(str(tmp_path), 'recB')
    assert (u.tolist(), v.tolist(), spk.tolist(), names) == ([100000], [800000], [0], ['x'])
    ru, rv, rspk, S = ref.read(str(tmp_path), 'recB')
    assert (ru.tolist(), rv.tolist(), rspk.tolist(), S) == ([100000], [800000], [0], 1)


def test_read_turns_is_what_it_was_and_can_give_the_duration(tmp_path):
    from vbx_amd import score
    (tmp_path / 'a.rttm').write_text('SPEAKER recA 1 0.1 0.2 <NA> <NA> x <NA> <NA>\n')
    assert score.read_turns(str(tmp_path / 'a.rttm')) == {'recA': [(0.1, 0.1 + 0.2, 'x')]}
    assert score.read_turns(str(tmp_path / 'a.rttm'), durations=True) == {'recA': [(0.1, 0.1 + 0.2, 'x', 0.2)]}


# ---- the driver's route --------------------------------------------------------------------------------------------------
class _Stages:
    """Host stand-in for DeviceStages: answers ``turn_labels`` and ``vb_turns`` with the referee's labels and remembers what it
    was asked; AHC raises."""

    def __init__(self):
        self.calls = []

    def project(self, recordings, models, lda_dim):
        self.T = [len(r[1]) for r in recordings]

    def ahc(self, *a, **k):
        raise AssertionError('--init RTTM / RTTM+VB must not run AHC')

    def vb(self, *a, **k):
        raise AssertionError('--init RTTM+VB must not start from AHC labels')

    def turn_labels(self, k, turns, segments):
        self.calls.append(('turn_labels', k))
        (a, b), (u, v, spk, S) = segments, turns
        return ref.weights(a, b, u, v, spk, S)[0]

    def vb_turns(self, ks, turns, segments, **kw):
        self.calls.append(('vb_turns', list(ks), kw))
        return [(ref.weights(a, b, u, v, spk, S)[0], None, 4) for (a, b), (u, v, spk, S) in zip(segments, turns)]


def _archive(tmp_path, names=('recA', 'recB')):
    T = {'recA': 9, 'recB': 14, 'recC': 5}
    recordings = [(n, [f'{n}_{i}' for i in range(T[n])], np.zeros((T[n], 4), dtype=np.float32)) for n in names]
    segs = {n: (np.array([f'{n}_{i}' for i in range(T[n])]), np.stack([0.24 * np.arange(T[n]), 0.24 * np.arange(T[n]) + 1.44], 1))
            for n in names}
    first = tmp_path / 'first'
    first.mkdir(exist_ok=True)
    for n in names:
        (first / f'{n}.rttm').write_text(f'SPEAKER {n} 1 1.5 0.9 <NA> <NA> late <NA> <NA>\nSPEAKER {n} 1 0.0 0.9 <NA> <NA> early <NA> <NA>\n'
                                         f'SPEAKER {n} 1 2.5 9.0 <NA> <NA> third <NA> <NA>\n')
    return recordings, segs, str(first)


@pytest.mark.parametrize('init', ['RTTM', 'RTTM+VB'])
def test_the_driver_reads_only_its_recordings_files_skips_ahc_and_writes_the_labels(init, tmp_path):
    from vbx_amd import vbhmm
    recordings, segs, first = _archive(tmp_path)
    os.remove(os.path.join(first, 'recB.rttm'))
    args = argparse.Namespace(init=init, init_rttm_dir=first, threshold=0.0, lda_dim=4, Fa=0.3, Fb=17.0, loopP=0.9, init_smoothing=5.0,
                              output_2nd=False, out_rttm_dir=str(tmp_path / 'out'))
    with pytest.raises(ValueError, match=r'recB\.rttm'):               # (named before anything runs)
        vbhmm.diarize_recordings(recordings, segs, dict(plda_psi=np.ones(4)), args, _Stages(), log=lambda *a: None)
    stages = _Stages()
    state, _timing = vbhmm.diarize_recordings(recordings[:1], segs, dict(plda_psi=np.ones(4)), args, stages, log=lambda *a: None)
    u, v, spk, S = ref.read(first, 'recA')
    assert S == 3 and spk.tolist() == [0, 1, 2]
    want = ref.weights(*ref.windows(segs['recA'][1]), u, v, spk, S)[0]
    assert len(set(want.tolist())) == 3
    st = state['recA']
    assert np.array_equal(st['labels1st'], want) and st['thr'] != st['thr'] and st['n_iters'] == (4 if init == 'RTTM+VB' else 0)
    if init == 'RTTM':
        assert stages.calls == [('turn_labels', 0)]
    else:
        (what, ks, kw), = stages.calls
        assert what == 'vb_turns' and ks == [0] and kw['maxIters'] == 40 and kw['epsilon'] == 1e-6
        assert (kw['Fa'], kw['Fb'], kw['loopProb'], kw['init_smoothing']) == (0.3, 17.0, 0.9, 5.0)
    lines = open(tmp_path / 'out' / 'recA.rttm').read().splitlines()
    assert len(lines) == 3 and [l.split()[7] for l in lines] == [str(int(x) + 1) for x in dict.fromkeys(want.tolist())]


def test_the_library_call_refuses_the_directory_with_another_init(tmp_path):
    from vbx_amd import vbhmm
    recordings, segs, first = _archive(tmp_path, ('recA',))
    args = argparse.Namespace(init='AHC+VB', init_rttm_dir=first, threshold=0.0, lda_dim=4, Fa=0.3, Fb=17.0, loopP=0.9,
                              init_smoothing=5.0, output_2nd=False, out_rttm_dir=None)
    with pytest.raises(ValueError, match='--init-rttm-dir needs --init RTTM or RTTM\\+VB'):
        vbhmm.diarize_recordings(recordings, segs, dict(plda_psi=np.ones(4)), args, _Stages(), log=lambda *a: None)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_the_header_still_says_abi_7_and_declares_the_new_entry_points():
    from vbx_amd import _capi
    header = open(os.path.join(REPO, 'include', 'vbx_hip.h')).read()
    assert re.search(r'#define\s+VBX_ABI_VERSION\s+7\b', header)
    for sym in ('vbx_turn_weights', 'vbx_batch_set_recording_turns'):
        assert re.search(rf'\bint {sym}\s*\(', header) and sym in _capi.ABI_SYMBOLS
    assert callable(_capi.turn_weights) and callable(_capi.Batch.set_recording_turns)
    lib = _capi.load()
    assert lib.vbx_abi_version() == 7 and lib.vbx_turn_weights and lib.vbx_batch_set_recording_turns


GOOD = dict(seg_a=[0, 10], seg_b=[10, 20], turn_u=[0, 12, 5], turn_v=[8, 30, 9], turn_spk=[0, 0, 1], S=2)


@pytest.mark.parametrize('change,message', [
    (dict(seg_a=[], seg_b=[]), 'T=0'),
    (dict(turn_u=[], turn_v=[], turn_spk=[]), 'N=0'),
    (dict(turn_spk=[0, 0, 2]), 'speaker 2 of turn 2 outside [0, 2)'),
    (dict(turn_spk=[0, 0, -1]), 'speaker -1 of turn 2'),
    (dict(seg_b=[10, 10]), 'window 1 is empty'),
    (dict(seg_b=[10, 9]), 'window 1 is empty'),
    (dict(turn_u=[0, 12, 9]), 'turn 2 is empty'),
    (dict(turn_spk=[0, 1, 0]), 'turn 2 is out of order'),
    (dict(turn_u=[12, 0, 5], turn_v=[30, 8, 9]), 'turn 1 is out of order'),
    (dict(S=0), 'S=0'),
    (dict(S=1 << 20), 'S='),
    ({}, 'NULL context'),                                          # input in order: only the device is missing
])
def test_turn_weights_refuses_bad_input_before_the_device_is_touched(change, message):
    from vbx_amd import _capi
    a = dict(GOOD, **change)
    with pytest.raises(_capi.VbxError) as exc:
        _capi.turn_weights(None, a['seg_a'], a['seg_b'], a['turn_u'], a['turn_v'], a['turn_spk'], a['S'], 5.0)
    assert '(-1)' in str(exc.value) and message in str(exc.value), str(exc.value)      # VBX_ERR_INVALID


def test_the_c_entry_returns_vbx_err_invalid_itself():
    from vbx_amd import _capi
    lib = _capi.load()
    a = np.array([0], dtype=np.int64)
    b = np.array([0], dtype=np.int64)                               # a == b
    spk = np.array([0], dtype=np.int32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert lib.vbx_turn_weights(None, 1, p(a), p(b), 1, p(a), p(a + 1), p(spk), 1, 5.0, None, None, None) == -1
    assert b'window 0 is empty' in lib.vbx_last_error(None)
    with pytest.raises(ValueError, match='windows'):
        _capi.turn_weights(None, [0, 1], [2], [0], [1], [0], 1, 5.0)
