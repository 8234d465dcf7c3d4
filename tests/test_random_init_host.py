"""``--init random_N`` without a GPU: the referee's own conventions, the hash, the command lines, the winner rule, the order
independence of the labels and the C header.  The device side is tests/test_gpu_random_init.py."""
import argparse
import os
import re

import numpy as np
import pytest

import random_init_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VBHMM = ['--out-rttm-dir', 'out', '--xvec-ark-file', 'x.ark', '--segments-file', 'x.seg', '--xvec-transform', 't.h5', '--plda-file',
         'plda', '--threshold', '-0.015', '--lda-dim', '128', '--Fa', '0.3', '--Fb', '17', '--loopP', '0.99']
DIARIZE = ['--gpus', '0', '--checkpoint', 'c.pth', '--in-file-list', 'l.txt', '--in-lab-dir', 'lab', '--in-wav-dir', 'wav',
           '--out-rttm-dir', 'out', '--xvec-transform', 't.h5', '--plda-file', 'plda', '--threshold', '-0.015', '--lda-dim', '128',
           '--Fa', '0.3', '--Fb', '17', '--loopP', '0.99']
TUNE = ['--xvec-ark-file', 'x.ark', '--segments-file', 'x.seg', '--xvec-transform', 't.h5', '--plda-file', 'plda', '--threshold',
        '-0.015', '--lda-dim', '128', '--Fa', '0.3', '--Fb', '17', '--loopP', '0.99']


# ---- the generator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key,counter', [
    ([0, 0], [0, 0, 0, 0]),
    ([7, ref.name_hash('recA')], [0, 3, 0, 0]),
    ([(1 << 63) + 5, (1 << 64) - 1], [5, 1, 2, 3]),
    ([1, 2], [(1 << 64) - 2, 0, 0, 0]),                      # the first word overflows into the second after one block
    ([3, 4], [(1 << 64) - 2, (1 << 64) - 1, 5, 0]),          # ... and the carry runs through two words
])
def test_numpys_philox_is_ten_rounds_of_philox4x64_counter_stepped_first_words_in_order(key, counter):
    """What the definition relies on: numpy's generator is Philox4x64-10, it steps the 256-bit counter (word 0 the least
    significant, carries into the next words) BEFORE its first block, and hands the four words of a block out in order."""
    bg = np.random.Philox(key=np.array(key, dtype=np.uint64), counter=np.array(counter, dtype=np.uint64))
    got = [int(w) for w in bg.random_raw(14)]
    want, c = [], counter
    for _block in range(4):
        c = ref.increment(c)
        want += ref.philox4x64_10(c, key)
    assert got == want[:14]


def test_word_t_is_word_t_mod_4_of_the_block_with_counter_t_div_4_plus_1():
    seed, h, r = 11, ref.name_hash('dev007'), 2
    w = ref.words(seed, h, r, 23)
    for t in (0, 1, 3, 4, 5, 22):
        assert w[t] == ref.philox4x64_10([t // 4 + 1, r, 0, 0], [seed, h])[t % 4]
    assert ref.words(seed, h, r, 5) == w[:5]                 # (a prefix: the labels of a frame do not depend on T)


def test_labels_are_the_high_half_of_the_product():
    w = ref.words(3, 9, 0, 200)
    for N in (1, 2, 3, 7, 64, 65, 1000):
        lab = ref.labels_hashed(3, 9, 0, 200, N)
        assert lab.min() >= 0 and lab.max() < N
        assert all(int(l) * (1 << 64) <= x * N < (int(l) + 1) * (1 << 64) for l, x in zip(lab, w))
    assert np.all(ref.labels_hashed(3, 9, 0, 200, 1) == 0)
    assert len(set(ref.labels_hashed(3, 9, 0, 200, 4).tolist())) == 4


# ---- the hash --------------------------------------------------------------------------------------------------------
def test_fnv1a_known_answers():
    from vbx_amd import vbhmm
    assert ref.fnv1a64(b'') == 0xcbf29ce484222325
    assert ref.fnv1a64(b'a') == 0xaf63dc4c8601ec8c
    assert ref.fnv1a64(b'foobar') == 0x85944171f73967e8
    for name in ('', 'a', 'recA', 'ES2005a', 'réunion-会議'):
        assert vbhmm.name_hash(name) == ref.name_hash(name) == ref.fnv1a64(name.encode('utf-8'))
    assert ref.name_hash('recA') >> 63 == 0 and ref.name_hash('dev000') >> 63 == 1      # (the two names the device test draws under)


# ---- the command lines -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('init,N', [('random_1', 1), ('random_4', 4), ('random_8', 8), ('random_016', 16), ('random_1000', 1000)])
def test_random_n_is_accepted(init, N, capsys):
    from vbx_amd import diarize, tune, vbhmm
    assert vbhmm.random_init_states(init) == N and vbhmm.runs_vb(init)
    p = vbhmm.build_parser()
    args = p.parse_args(['--init', init] + VBHMM)
    vbhmm.check_init_arguments(args, p.error)
    assert (args.init, args.random_restarts, args.seed) == (init, 1, 0)
    args = p.parse_args(['--init', init, '--random-restarts', '5', '--seed', str((1 << 64) - 1)] + VBHMM)
    vbhmm.check_init_arguments(args, p.error)
    assert (args.random_restarts, args.seed) == (5, (1 << 64) - 1)
    args = diarize.parse_args(['--init', init, '--random-restarts', '3', '--seed', '7'] + DIARIZE)
    assert (args.init, args.random_restarts, args.seed) == (init, 3, 7)
    args = tune.build_parser().parse_args(['--init', init, '--random-restarts', '2', '--ref-rttm-dir', 'ref'] + TUNE)
    assert tune.check_init(args) == (N, 2, 0)
    capsys.readouterr()


def test_the_old_values_parse_as_before_and_tune_defaults_to_ahc_vb():
    from vbx_amd import diarize, tune, vbhmm
    for init in ('AHC', 'AHC+VB'):
        assert vbhmm.random_init_states(init) is None and vbhmm.runs_vb(init) == (init == 'AHC+VB')
        p = vbhmm.build_parser()
        args = p.parse_args(['--init', init] + VBHMM)
        vbhmm.check_init_arguments(args, p.error)
        assert (args.init, args.random_restarts, args.seed) == (init, None, None)
        assert diarize.parse_args(['--init', init] + DIARIZE).init == init
    args = tune.build_parser().parse_args(TUNE + ['--ref-rttm-dir', 'ref'])
    assert args.init == 'AHC+VB' and tune.check_init(args) == (None, 1, 0)
    assert tune.check_init(argparse.Namespace()) == (None, 1, 0)         # (a caller of tune_recordings from before the flag)
    with pytest.raises(ValueError, match='AHC runs no VB-HMM'):
        tune.check_init(argparse.Namespace(init='AHC'))


@pytest.mark.parametrize('init', ['random_', 'random_0', 'random_x', 'random_3+VB', 'Random_3', 'random', 'random_-2', 'random_ 3',
                                  'random_3.0', 'random__3', 'random_٣'])
def test_what_is_not_random_n_is_refused_with_a_message(init, capsys):
    from vbx_amd import diarize, tune, vbhmm
    with pytest.raises(ValueError, match='random_<N>'):
        vbhmm.random_init_states(init)
    for parse, argv in ((vbhmm.build_parser().parse_args, VBHMM), (diarize.parse_args, DIARIZE),
                        (tune.build_parser().parse_args, TUNE + ['--ref-rttm-dir', 'ref'])):
        with pytest.raises(SystemExit) as exc:
            parse(['--init=' + init] + argv)
        assert exc.value.code == 2
        err = capsys.readouterr().err
        assert 'argument --init' in err and 'random_<N>' in err
    with pytest.raises(ValueError, match='init must be'):
        diarize.diarize_files(['a'], 'wav', 'lab', 'c.pth', 't.h5', 'plda', init=init)


@pytest.mark.parametrize('extra,message', [
    (['--init', 'AHC+VB', '--random-restarts', '3'], '--random-restarts needs --init random_<N>'),
    (['--init', 'AHC', '--seed', '1'], '--seed needs --init random_<N>'),
    (['--init', 'AHC+VB', '--seed', '0'], '--seed needs --init random_<N>'),
    (['--init', 'random_4', '--random-restarts', '0'], 'must be >= 1'),
    (['--init', 'random_4', '--seed', '-1'], '--seed -1'),
    (['--init', 'random_4', '--seed', str(1 << 64)], '--seed'),
])
def test_restarts_and_seed_are_refused_without_random_n_or_out_of_range(extra, message, capsys):
    from vbx_amd import diarize, tune, vbhmm
    p = vbhmm.build_parser()
    with pytest.raises(SystemExit) as exc:
        vbhmm.check_init_arguments(p.parse_args(extra + VBHMM), p.error)
    assert exc.value.code == 2 and message in capsys.readouterr().err
    with pytest.raises(SystemExit):
        diarize.parse_args(extra + DIARIZE)
    assert message in capsys.readouterr().err
    if extra[1] != 'AHC':
        with pytest.raises(ValueError):
            tune.check_init(tune.build_parser().parse_args(extra + TUNE + ['--ref-rttm-dir', 'ref']))


def test_the_ahc_options_are_accepted_and_ignored_with_one_warning_line(capsys):
    from vbx_amd import diarize, vbhmm
    p = vbhmm.build_parser()
    args = p.parse_args(['--init', 'random_4', '--ahc-scores', 'plda', '--target-energy', '0.5'] + VBHMM)
    vbhmm.check_init_arguments(args, p.error)
    err = capsys.readouterr().err
    assert len(err.splitlines()) == 1 and all(w in err for w in ('warning', '--threshold', '--ahc-scores', '--target-energy', 'ignored'))
    said = []
    vbhmm.check_init_arguments(p.parse_args(['--init', 'random_4'] + VBHMM), p.error, warn=said.append)
    assert len(said) == 1 and capsys.readouterr().err == ''
    diarize.parse_args(['--init', 'random_4'] + DIARIZE)
    assert len(capsys.readouterr().err.splitlines()) == 1
    vbhmm.check_init_arguments(p.parse_args(['--init', 'AHC+VB'] + VBHMM), p.error)
    assert capsys.readouterr().err == ''


# ---- the winner ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('elbos,winner', [
    ([-3.0], 0), ([-3.0, -2.0, -2.5], 1), ([-2.0, -2.0, -3.0], 0), ([-3.0, -2.0, -2.0], 1),
    ([float('nan'), -5.0, -4.0], 2), ([-5.0, float('nan'), -6.0], 0), ([float('nan'), float('nan'), -7.0], 2),
    ([float('nan')] * 3, 0), ([float('nan')], 0), ([-1.0, float('inf'), float('nan')], 1),
    ([float('-inf'), float('nan')], 0), ([float('nan'), float('-inf')], 1),
])
def test_best_restart_largest_elbo_lowest_among_equals_never_a_nan(elbos, winner):
    from vbx_amd import vbhmm
    assert ref.best_restart(elbos) == winner
    assert vbhmm.best_restart(elbos) == winner
    assert vbhmm.best_restart(np.array(elbos)) == winner


class _Stages:
    """Host stand-in for DeviceStages: remembers what vb_random was asked and answers with the referee's labels of the restart
    whose ELBO it was told to favour."""

    def __init__(self):
        self.calls = []

    def project(self, recordings, models, lda_dim):
        self.T = [len(r[1]) for r in recordings]

    def ahc(self, *a, **k):
        raise AssertionError('--init random_N must not run AHC')

    def vb_random(self, ks, N, restarts, seed, names, **kw):
        self.calls.append((list(ks), N, restarts, seed, list(names), kw))
        out = []
        for k, name in zip(ks, names):
            elbos = [-float((ref.name_hash(name) >> (8 * r)) & 0xFF) for r in range(restarts)]
            win = ref.best_restart(elbos)
            out.append((ref.labels(seed, name, win, self.T[k], N), None, 3, win, elbos))
        return out


def _archive(order):
    T = {'recA': 9, 'recB': 14, 'recC': 5}
    recordings = [(n, [f'{n}_{i}' for i in range(T[n])], np.zeros((T[n], 4), dtype=np.float32)) for n in order]
    segs = {n: (np.array([f'{n}_{i}' for i in range(T[n])]), np.stack([0.24 * np.arange(T[n]), 0.24 * np.arange(T[n]) + 1.44], 1))
            for n in order}
    return recordings, segs


def test_labels_do_not_change_when_the_archive_order_changes(tmp_path):
    """The driver hands vb_random the recording's NAME with its index, skips AHC, reports thr = nan -- and the same recording
    gets the same labels (and the same RTTM bytes) wherever it stands in the archive."""
    from vbx_amd import vbhmm
    outs = {}
    for tag, order in (('abc', ['recA', 'recB', 'recC']), ('cba', ['recC', 'recB', 'recA']), ('b', ['recB'])):
        recordings, segs = _archive(order)
        args = argparse.Namespace(init='random_4', random_restarts=3, seed=7, threshold=0.0, lda_dim=4, Fa=0.3, Fb=17.0, loopP=0.9,
                                  init_smoothing=5.0, output_2nd=False, out_rttm_dir=str(tmp_path / tag))
        stages = _Stages()
        state, _timing = vbhmm.diarize_recordings(recordings, segs, dict(plda_psi=np.ones(4)), args, stages, log=lambda *a: None)
        (ks, N, restarts, seed, names, kw), = stages.calls
        assert (N, restarts, seed, names) == (4, 3, 7, order) and ks == list(range(len(order)))
        assert kw['maxIters'] == 40 and kw['epsilon'] == 1e-6 and (kw['Fa'], kw['Fb'], kw['loopProb']) == (0.3, 17.0, 0.9)
        for name in order:
            st = state[name]
            assert st['thr'] != st['thr'] and st['n_iters'] == 3 and st['restart'] == ref.best_restart(st['elbos'])
            assert np.array_equal(st['labels1st'], ref.labels(7, name, st['restart'], len(st['labels1st']), 4))
        outs[tag] = {n: open(tmp_path / tag / f'{n}.rttm', 'rb').read() for n in order}
    assert outs['abc'] == outs['cba'] and outs['b']['recB'] == outs['abc']['recB']
    for r in range(3):
        assert np.array_equal(ref.labels(7, 'recB', r, 14, 4)[:9], ref.labels(7, 'recB', r, 9, 4))
        assert not np.array_equal(ref.labels(7, 'recA', r, 9, 4), ref.labels(7, 'recB', r, 9, 4))
        assert not np.array_equal(ref.labels(7, 'recB', r, 14, 4), ref.labels(8, 'recB', r, 14, 4))
    assert not np.array_equal(ref.labels(7, 'recB', 0, 14, 4), ref.labels(7, 'recB', 1, 14, 4))


def test_restarts_and_seed_without_random_n_are_refused_by_the_library_call():
    from vbx_amd import vbhmm
    recordings, segs = _archive(['recA'])
    args = argparse.Namespace(init='AHC+VB', random_restarts=2, seed=None, threshold=0.0, lda_dim=4, Fa=0.3, Fb=17.0, loopP=0.9,
                              init_smoothing=5.0, output_2nd=False, out_rttm_dir=None)
    with pytest.raises(ValueError, match='--random-restarts needs --init random_<N>'):
        vbhmm.diarize_recordings(recordings, segs, dict(plda_psi=np.ones(4)), args, _Stages(), log=lambda *a: None)


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_the_header_still_says_abi_7_and_declares_the_new_entry_points():
    from vbx_amd import _capi
    header = open(os.path.join(REPO, 'include', 'vbx_hip.h')).read()
    assert re.search(r'#define\s+VBX_ABI_VERSION\s+7\b', header)
    for sym in ('vbx_random_labels', 'vbx_batch_set_recording_random'):
        assert re.search(rf'\bint {sym}\s*\(', header) and sym in _capi.ABI_SYMBOLS
    assert callable(_capi.random_labels) and callable(_capi.Batch.set_recording_random)
    lib = _capi.load()
    assert lib.vbx_abi_version() == 7 and lib.vbx_random_labels and lib.vbx_batch_set_recording_random


def test_random_labels_refuses_bad_arguments_before_the_device_is_touched():
    from vbx_amd import _capi
    for kw in (dict(T=0, N=4), dict(T=5, N=0), dict(T=5, N=4, restart=-1), dict(T=5, N=4, seed=-1), dict(T=5, N=4, seed=1 << 64),
               dict(T=5, N=4, name_hash=1 << 64)):
        a = dict(seed=0, name_hash=0, restart=0)
        a.update(kw)
        with pytest.raises(ValueError):
            _capi.random_labels(None, a['seed'], a['name_hash'], a['restart'], a['T'], a['N'])
    with pytest.raises(ValueError, match='out must be'):
        _capi.random_labels(None, 0, 0, 0, 5, 4, out=np.zeros(5, dtype=np.int64))
