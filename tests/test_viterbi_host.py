"""Viterbi decoding, the host side (no GPU): the longdouble referee of tests/viterbi_ref.py against the dense max-plus
recursion and against all paths, its tie rules, the ``--decode`` argument of the three command lines, and the driver's core on
injected stages (tests/test_driver.py: OracleStages)."""
import os

import numpy as np
import pytest

import viterbi_ref as vr
from test_driver import OracleStages, RECS, _argv, _write_inputs

STATES = [1, 2, 3, 63, 64, 65, 128, 129, 513, 1024]
FRAMES = [1, 2, 63, 64, 65, 129, 1000]


# ---- the referee ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', STATES)
def test_structured_recursion_equals_the_dense_one(S):
    for i, T in enumerate(FRAMES):
        if S * S * T > 3e7:                                   # (the dense recursion is S^2 T: the large corner at one length)
            T = 40
        lp = (0.5, 0.9, 0.99)[i % 3]
        lls, pi = vr.draw(1000 * S + T, T, S)
        path, logp, margin = vr.structured(lls, lp, pi)
        assert margin > 1e-9, (S, T, float(margin))
        d_path, d_logp = vr.dense(lls, lp, pi)
        assert np.array_equal(path, d_path), (S, T)
        assert abs(float(logp - d_logp)) <= 2e-11 and abs(float(vr.score(path, lls, lp, pi) - logp)) <= 2e-11


@pytest.mark.parametrize('S,T', [(3, 6), (2, 10)])
def test_structured_recursion_finds_the_best_of_all_paths(S, T):
    for seed, lp in ((1, 0.5), (2, 0.9), (3, 0.0), (4, 1.0)):
        lls, pi = vr.draw(seed, T, S, sigma=2.0)
        ip = np.random.default_rng(seed).dirichlet(np.ones(S))
        best, arg = vr.brute_force(lls, lp, pi, ip)
        path, logp, _ = vr.structured(lls, lp, pi, ip)
        assert len(arg) == 1 and tuple(path) == arg[0], (S, T, lp)
        assert abs(float(best - logp)) < 1e-14


@pytest.mark.parametrize('S', [1, 2, 3, 65])
def test_all_equal_input_gives_the_all_zero_path(S):
    for T in (1, 2, 7):
        path, logp, margin = vr.structured(np.zeros((T, S)), 0.9, np.full(S, 1.0 / S))
        assert not path.any() and (margin == 0 or S == 1 or (T == 1 and S == 1))
        assert np.array_equal(vr.dense(np.zeros((T, S)), 0.9, np.full(S, 1.0 / S))[0], path)


def test_a_tie_between_staying_and_entering_stays():
    # loopProb = 0 and uniform pi: stay_j = move_j, so every back-pointer of the best state's column ties.  "Equality counts as
    # stayed": the path ends in state 1 and never leaves it, where the dense recursion (first index among equals) enters from 0
    lls, pi = np.array([[0.0, 0.0], [0.0, 0.0], [0.0, 1.0]]), np.array([0.5, 0.5])
    path, logp, _ = vr.structured(lls, 0.0, pi)
    assert path.tolist() == [1, 1, 1]
    d_path, d_logp = vr.dense(lls, 0.0, pi)
    assert d_path.tolist() == [0, 0, 1] and abs(float(d_logp - logp)) < 1e-15
    assert abs(float(vr.score(path, lls, 0.0, pi) - vr.score(d_path, lls, 0.0, pi))) < 1e-15


# ---- the command lines ---------------------------------------------------------------------------------------------
VBHMM = ['--out-rttm-dir', 'o', '--xvec-ark-file', 'a', '--segments-file', 's', '--xvec-transform', 't', '--plda-file', 'p',
         '--threshold', '0', '--lda-dim', '128', '--Fa', '0.3', '--Fb', '17', '--loopP', '0.99']
DIARIZE = ['--gpus', '0', '--checkpoint', 'c.pth', '--in-file-list', 'l', '--in-lab-dir', 'lab', '--in-wav-dir', 'wav',
           '--out-rttm-dir', 'o', '--xvec-transform', 't', '--plda-file', 'p', '--threshold', '0', '--lda-dim', '128', '--Fa', '0.3',
           '--Fb', '17', '--loopP', '0.99']
TUNE = ['--xvec-ark-file', 'a', '--segments-file', 's', '--xvec-transform', 't', '--plda-file', 'p', '--threshold', '0',
        '--lda-dim', '128', '--Fa', '0.3', '--Fb', '17', '--loopP', '0.99', '--ref-rttm-dir', '.']


def _parse(program, argv):
    from vbx_amd import diarize, tune, vbhmm
    if program == 'vbhmm':
        p = vbhmm.build_parser()
        args = p.parse_args(argv)
        vbhmm.check_init_arguments(args, p.error, warn=lambda _m: None)
        vbhmm.check_decode_argument(args, p.error)
        return args
    if program == 'diarize':
        return diarize.parse_args(argv)
    return tune.build_parser().parse_args(argv)


@pytest.mark.parametrize('program,base', [('vbhmm', VBHMM), ('diarize', DIARIZE), ('tune', TUNE)])
def test_decode_defaults_to_posterior_and_takes_viterbi(program, base, capsys):
    init = [] if program == 'tune' else ['--init', 'AHC+VB']
    assert _parse(program, base + init).decode == 'posterior'
    assert _parse(program, base + init + ['--decode', 'viterbi']).decode == 'viterbi'
    assert _parse(program, base + ['--init', 'random_4', '--decode', 'viterbi']).decode == 'viterbi'
    with pytest.raises(SystemExit):
        _parse(program, base + init + ['--decode', 'map'])
    assert 'invalid choice' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _parse(program, base + init + ['--help'])
    text = capsys.readouterr().out
    assert '--decode {posterior,viterbi}' in text and 'most probable' in text


@pytest.mark.parametrize('program,base', [('vbhmm', VBHMM), ('diarize', DIARIZE)])
@pytest.mark.parametrize('init', ['AHC', 'RTTM'])
def test_viterbi_is_refused_with_an_init_that_runs_no_vb(program, base, init, capsys, tmp_path):
    extra = ['--init-rttm-dir', str(tmp_path)] if init == 'RTTM' else []
    assert _parse(program, base + ['--init', init] + extra).decode == 'posterior'
    with pytest.raises(SystemExit) as exc:
        _parse(program, base + ['--init', init, '--decode', 'viterbi'] + extra)
    assert exc.value.code == 2
    assert '--decode viterbi needs the VB-HMM' in capsys.readouterr().err


def test_tune_refuses_an_init_without_vb_whatever_the_decode(capsys):
    from vbx_amd import tune
    with pytest.raises(SystemExit):
        tune.main(TUNE + ['--init', 'AHC', '--decode', 'viterbi'])
    assert 'runs no VB-HMM' in capsys.readouterr().err


def test_the_library_call_takes_the_keyword_and_refuses_what_the_command_line_refuses():
    from vbx_amd import diarize
    with pytest.raises(ValueError, match='decode must be'):
        diarize.diarize_files(['a'], 'wav', 'lab', 'c.pth', 't.h5', 'plda', decode='map')
    with pytest.raises(ValueError, match='needs the VB-HMM'):
        diarize.diarize_files(['a'], 'wav', 'lab', 'c.pth', 't.h5', 'plda', init='AHC', decode='viterbi')


# ---- the driver's core on injected stages -----------------------------------------------------------------------------
class PathStages(OracleStages):
    """OracleStages whose VB stage reads the run out as it is asked to: with ``decode='viterbi'`` first / second are what its
    ``path`` returns -- here a sequence no arg-sort of responsibilities gives: the AHC label and the one after it."""
    def __init__(self):
        super().__init__()
        self.decodes = []

    def path(self, lab):
        first = np.asarray(lab, dtype=np.int64)
        return first, (first + 1) % (int(first.max()) + 1)

    def vb(self, ks, labels, init_smoothing, maxIters, epsilon, precision, decode='posterior', **hyper):
        self.decodes.append(decode)
        out = super().vb(ks, labels, init_smoothing, maxIters, epsilon, precision, **hyper)
        if decode == 'viterbi':
            out = [(*self.path(lab), n) for lab, (_f, _s, n) in zip(labels, out)]
        return out


def _args(paths, extra=()):
    from vbx_amd import vbhmm
    return vbhmm.build_parser().parse_args(_argv(paths, extra))


def test_labels1st_is_the_path_the_stage_returns(tmp_path):
    from vbx_amd import vbhmm
    paths = _write_inputs(tmp_path)
    stages = PathStages()
    state, _ = vbhmm.diarize(_args(paths, ['--decode', 'viterbi']), stages=stages, log=lambda *_: None)
    assert stages.decodes == ['viterbi'] and list(state) == list(RECS)
    for k, rec in enumerate(RECS):
        first, second = stages.path(stages.ahc(k, -0.015)[0])
        assert np.array_equal(state[rec]['labels1st'], first) and np.array_equal(state[rec]['labels2nd'], second), rec
        assert os.path.isfile(os.path.join(paths['out'], rec + '.rttm')) and os.path.isfile(os.path.join(paths['out'] + '2nd', rec + '.rttm'))


def test_without_the_flag_the_stage_is_called_without_the_keyword(tmp_path):
    from vbx_amd import vbhmm
    from test_driver import _check_rttm
    paths = _write_inputs(tmp_path)
    stages = OracleStages()                                   # (its vb() hands every keyword on to the oracle: 'decode' would fail)
    vbhmm.diarize(_args(paths), stages=stages, log=lambda *_: None)
    _check_rttm(paths)


def test_a_recording_over_the_state_limit_of_the_decode_is_left_out_by_name(tmp_path, monkeypatch):
    from vbx_amd import _capi, vbhmm
    assert _capi.MAX_DECODE_STATES == 1024
    monkeypatch.setattr(_capi, 'MAX_DECODE_STATES', 100)      # (the golden recordings are short: recB gets 290 clusters below)
    paths = _write_inputs(tmp_path)

    class Many(PathStages):
        def ahc(self, k, threshold):
            labels, thr = super().ahc(k, threshold)
            return (np.arange(len(labels)) % 290 if k == 1 else labels), thr
    stages = Many()
    with pytest.raises(RuntimeError, match=r'recB \(AHC left 290 clusters, the device path takes at most 100\)'):
        vbhmm.diarize(_args(paths, ['--decode', 'viterbi']), stages=stages, log=lambda *_: None)
    assert sorted(os.listdir(paths['out'])) == ['recA.rttm', 'recC.rttm']
