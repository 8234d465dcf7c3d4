"""The host side of ``vbx_amd.diarize`` (wav files to RTTM in one process): its command line, the way the segment times
take through their text form, the list of kept rows, and the core of the driver (``vbhmm.diarize_recordings``) on recordings
that never were a file -- with the CPU stages tests/test_driver.py injects."""
import os

import numpy as np
import pytest

from test_driver import OracleStages, RECS, _argv, _check_rttm, _write_inputs

REQUIRED = ['--in-file-list', 'l', '--in-lab-dir', 'lab', '--in-wav-dir', 'wav', '--init', 'AHC+VB', '--out-rttm-dir', 'out',
            '--xvec-transform', 't.h5', '--plda-file', 'plda', '--threshold', '-0.015', '--lda-dim', '128', '--Fa', '0.3',
            '--Fb', '17', '--loopP', '0.99']
BASE = ['--gpus', '0', '--checkpoint', 'raw_81.pth'] + REQUIRED


# ---- the command line ----------------------------------------------------------------------------------------------
def test_the_command_line_is_the_union_of_predict_and_vbhmm():
    from vbx_amd import diarize
    a = diarize.parse_args(BASE)
    assert (a.gpus, a.checkpoint, a.gemm, a.ndim, a.embed_dim, a.seg_len, a.seg_jump, a.batch_size) == \
        ('0', 'raw_81.pth', 'exact', 64, 256, 144, 24, 128)
    assert (a.in_file_list, a.in_lab_dir, a.in_wav_dir, a.no_dither, a.dither) == ('l', 'lab', 'wav', False, 'host')
    assert (a.init, a.out_rttm_dir, a.xvec_transform, a.plda_file) == ('AHC+VB', 'out', 't.h5', 'plda')
    assert (a.threshold, a.lda_dim, a.Fa, a.Fb, a.loopP) == (-0.015, 128, 0.3, 17.0, 0.99)
    assert (a.target_energy, a.ahc_scores, a.init_smoothing, a.output_2nd, a.precision, a.timing) == \
        (1.0, 'cos', 5.0, False, 'fp64', False)
    assert a.out_ark_fn is None and a.out_seg_fn is None                      # optional here
    b = diarize.parse_args(BASE + ['--gemm', 'split', '--seg-len', '100', '--seg-jump', '20', '--batch-size', '7', '--dither',
                                   'device', '--out-ark-fn', 'x.ark', '--out-seg-fn', 'x.seg', '--ahc-scores', 'plda',
                                   '--target-energy', '0.5', '--init-smoothing', '7', '--output-2nd', 'True', '--precision',
                                   'fp32', '--timing', '--embed-dim', '128'])
    assert (b.gemm, b.seg_len, b.seg_jump, b.batch_size, b.dither, b.out_ark_fn, b.out_seg_fn) == \
        ('split', 100, 20, 7, 'device', 'x.ark', 'x.seg')
    assert (b.ahc_scores, b.target_energy, b.init_smoothing, b.output_2nd, b.precision, b.timing, b.embed_dim) == \
        ('plda', 0.5, 7.0, True, 'fp32', True, 128)
    assert diarize.parse_args(BASE + ['--no-dither']).no_dither is True


@pytest.mark.parametrize('missing', ['--in-file-list', '--in-lab-dir', '--in-wav-dir', '--init', '--out-rttm-dir',
                                     '--xvec-transform', '--plda-file', '--threshold', '--lda-dim', '--Fa', '--Fb', '--loopP'])
def test_required_flags_are_required(missing, capsys):
    from vbx_amd import diarize
    i = BASE.index(missing)
    with pytest.raises(SystemExit):
        diarize.parse_args(BASE[:i] + BASE[i + 2:])
    assert missing in capsys.readouterr().err


@pytest.mark.parametrize('extra,message', [
    (['--model-file', 'm.pt'], '--model-file is not supported'),
    (['--backend', 'onnx'], '--backend onnx is not supported'),
    (['--model', 'ResNet101'], '--model/--weights are not supported'),
    (['--weights', 'w.pth'], '--model/--weights are not supported'),
    (['--no-dither', '--dither', 'device'], 'exclude each other'),
    (['--ndim', '40'], '--ndim must be 64'),
    (['--batch-size', '0'], 'must be positive'),
    (['--out-ark-fn', 'x.ark'], 'go together'),
    (['--out-seg-fn', 'x.seg'], 'go together'),
    (['--loopP', '1.5'], 'loopP between 0 and 1'),
    (['--init', 'VB'], 'invalid choice'),
])
def test_what_the_route_does_not_do_is_refused_with_a_message(extra, message, capsys):
    from vbx_amd import diarize
    with pytest.raises(SystemExit) as exc:
        diarize.parse_args(BASE + extra)
    assert exc.value.code == 2
    assert message in capsys.readouterr().err


def test_a_run_without_a_gpu_or_a_checkpoint_is_refused(capsys):
    from vbx_amd import diarize
    for argv, message in ((['--checkpoint', 'c.pth'] + REQUIRED, '--gpus is empty'), (['--gpus', '0'] + REQUIRED, '--checkpoint')):
        with pytest.raises(SystemExit):
            diarize.parse_args(argv)
        assert message in capsys.readouterr().err


def test_the_library_call_refuses_what_the_command_line_refuses():
    from vbx_amd import diarize
    with pytest.raises(ValueError, match='go together'):
        diarize.diarize_files(['a'], 'wav', 'lab', 'c.pth', 't.h5', 'plda', out_ark_fn='x.ark')
    with pytest.raises(ValueError, match='loopP'):
        diarize.diarize_files(['a'], 'wav', 'lab', 'c.pth', 't.h5', 'plda', loopP=2.0)
    with pytest.raises(ValueError, match='init must be'):
        diarize.diarize_files(['a'], 'wav', 'lab', 'c.pth', 't.h5', 'plda', init='VB')


# ---- segment times -------------------------------------------------------------------------------------------------
def test_segment_times_take_the_way_through_the_segments_file(tmp_path):
    """A few thousand random (lab start, lab end, window start, seg_len, sample rate): the doubles ``segment_times`` parses
    from window_plan's lines are, bit for bit, the ones ``read_xvector_timing_dict`` reads from a file of those lines --
    what vbhmm gets after predict wrote it -- and both are the printed numbers."""
    from vbx_amd import diarize, fbank
    from vbx_amd.kaldi_formats import read_xvector_timing_dict
    rng = np.random.default_rng(20)
    lines, want = [], {}
    for f in range(40):
        sr = (8000, 16000)[f % 2]
        seg_len, seg_jump = int(rng.integers(20, 200)), int(rng.integers(5, 60))
        segs, pos = [], int(rng.integers(0, 5 * sr))
        for segnum in range(int(rng.integers(1, 12))):
            n = int(rng.integers(int(0.011 * sr), 9 * sr))
            segs.append(fbank.Segment(segnum, pos, n, fbank.n_frames(n, sr), (pos, pos + n)))
            pos += n + int(rng.integers(1, 3 * sr))
        plan = fbank.window_plan(f'file{f}', segs, sr, seg_len, seg_jump)
        lines += [w.line for w in plan]
        want[f'file{f}'] = plan
    assert len(lines) > 3000
    path = tmp_path / 'x.seg'
    with open(path, 'w') as fh:
        fh.write(''.join(line + os.linesep for line in lines))
    from_file, direct = read_xvector_timing_dict(str(path)), diarize.segment_times(lines)
    assert list(from_file) == list(direct) == list(want)
    for name, plan in want.items():
        assert direct[name][0].tolist() == from_file[name][0].tolist() == [w.key for w in plan]
        assert direct[name][1].dtype == np.float64 and direct[name][1].shape == (len(plan), 2)
        assert np.array_equal(direct[name][1].view(np.int64), from_file[name][1].view(np.int64))
        printed = np.array([[float(v) for v in w.line.split()[2:]] for w in plan])
        assert np.array_equal(direct[name][1], printed)
    assert diarize.segment_times([]) == {}


# ---- the keep list -------------------------------------------------------------------------------------------------
def _windows(counts):
    keys, lines = [], []
    for fn, n in counts.items():
        for i in range(n):
            keys.append(f'{fn}_{i:04}-{0:08}-{144:08}')
            lines.append(f'{keys[-1]} {fn} {0.24 * i:.2f} {0.24 * i + 1.44:.2f}')
    return keys, lines


def test_keep_list_without_a_nan_keeps_everything():
    from vbx_amd import diarize
    files = ['a', 'b_x']                                                     # (an underscore in the name: the key splits at the last)
    keys, lines = _windows({'a': 3, 'b_x': 2})
    warned = []
    rows, recs, segs, vanished = diarize.plan_recordings(files, keys, lines, np.zeros(5, bool), warn=warned.append)
    assert rows is None and vanished == [] and warned == []
    assert [(r[0], r[1].tolist(), r[2]) for r in recs] == [('a', keys[:3], None), ('b_x', keys[3:], None)]
    assert list(segs) == files and segs['b_x'][0].tolist() == keys[3:] and segs['a'][1].shape == (3, 2)


def test_keep_list_drops_rows_recordings_and_everything():
    from vbx_amd import diarize
    files = ['a', 'empty', 'b', 'c']                                         # 'empty': a file no window came of
    keys, lines = _windows({'a': 3, 'b': 2, 'c': 4})
    flags = np.zeros(9, bool)
    flags[[1, 3, 4, 8]] = True                                               # the middle of a, all of b, the last of c
    warned = []
    rows, recs, segs, vanished = diarize.plan_recordings(files, keys, lines, flags, warn=warned.append)
    assert rows.dtype == np.int64 and rows.tolist() == [0, 2, 5, 6, 7]
    assert warned == [f'NaN found, not processing: {keys[i]}{os.linesep}' for i in (1, 3, 4, 8)]          # predict's text
    assert [r[0] for r in recs] == ['a', 'c'] and vanished == ['empty', 'b']
    assert recs[0][1].tolist() == [keys[0], keys[2]] and recs[1][1].tolist() == keys[5:8]
    assert list(segs) == ['a', 'c'] and segs['a'][0].tolist() == [keys[0], keys[2]]
    assert np.array_equal(segs['a'][1], [[0.0, 1.44], [0.48, 1.92]])
    # every row dropped; nothing there at all
    rows, recs, segs, vanished = diarize.plan_recordings(files, keys, lines, np.ones(9, bool), warn=warned.append)
    assert rows.tolist() == [] and recs == [] and segs == {} and vanished == files
    rows, recs, segs, vanished = diarize.plan_recordings(['empty'], [], [], np.zeros(0, bool))
    assert rows is None and recs == [] and segs == {} and vanished == ['empty']
    with pytest.raises(AssertionError):
        diarize.plan_recordings(files, keys, lines, np.zeros(8, bool))


# ---- the core of the driver ----------------------------------------------------------------------------------------
def test_the_core_gives_the_state_of_the_file_reading_driver(tmp_path, capsys):
    """``diarize`` = reading + ``diarize_recordings``: called on what the readers return, the core writes the golden RTTM
    files and returns the state ``diarize`` returns."""
    from vbx_amd import vbhmm
    from vbx_amd.kaldi_formats import read_vec_flt_ark_grouped, read_xvector_timing_dict
    paths = _write_inputs(tmp_path)
    args = vbhmm.build_parser().parse_args(_argv(paths))
    want, want_timing = vbhmm.diarize(args, stages=OracleStages())
    _check_rttm(paths)
    for d in (paths['out'], paths['out'] + '2nd'):
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
    capsys.readouterr()
    got, timing = vbhmm.diarize_recordings(read_vec_flt_ark_grouped(paths['ark']), read_xvector_timing_dict(paths['seg']),
                                           vbhmm.load_models(paths['transform'], paths['plda']), args, OracleStages())
    assert capsys.readouterr().out.split() == list(RECS)
    _check_rttm(paths)
    assert list(got) == list(want) == list(RECS)
    for rec in RECS:
        assert set(got[rec]) == set(want[rec]) == {'labels1st', 'labels2nd', 'thr', 'n_iters'}
        assert np.array_equal(got[rec]['labels1st'], want[rec]['labels1st'])
        assert np.array_equal(got[rec]['labels2nd'], want[rec]['labels2nd'])
        assert got[rec]['thr'] == want[rec]['thr'] and got[rec]['n_iters'] == want[rec]['n_iters']
    assert set(timing) == set(want_timing)
    assert (timing['recordings'], timing['xvectors'], timing['rank'], timing['world']) == (3, 1025, 0, 1)


def test_the_core_without_an_rttm_directory_returns_labels_only(tmp_path):
    from vbx_amd import vbhmm
    from vbx_amd.kaldi_formats import read_vec_flt_ark_grouped, read_xvector_timing_dict
    paths = _write_inputs(tmp_path)
    argv = _argv(paths)
    argv[1] = 'AHC'
    args = vbhmm.build_parser().parse_args(argv)
    want, _ = vbhmm.diarize(args, stages=OracleStages(), log=lambda *_: None)
    args.out_rttm_dir = None
    stages = OracleStages()
    got, _ = vbhmm.diarize_recordings(read_vec_flt_ark_grouped(paths['ark'])[1:], read_xvector_timing_dict(paths['seg']),
                                      vbhmm.load_models(paths['transform'], paths['plda']), args, stages, log=lambda *_: None)
    assert list(got) == list(RECS[1:]) and not stages.vb_calls
    for rec in RECS[1:]:
        assert np.array_equal(got[rec]['labels1st'], want[rec]['labels1st'])
    assert not os.path.exists('None') and not os.path.exists('None2nd')


def test_device_stages_refuse_projections_that_do_not_fit_the_recordings():
    """project_device checks what it adopts against the recordings before any stage reads it (no device needed: the check
    is on the host)."""
    from types import SimpleNamespace
    from vbx_amd import vbhmm
    stages = vbhmm.DeviceStages.__new__(vbhmm.DeviceStages)
    stages.ctx, stages.xv = SimpleNamespace(device=0), None
    models = dict(plda_psi=np.ones(8))
    ok = SimpleNamespace(n=7, fea_dim=4, ctx=SimpleNamespace(device=0))
    stages.project_device([3, 4], ok, models, 4)
    assert stages.xv is ok and stages.T == [3, 4] and stages.row0.tolist() == [0, 3, 7] and stages.Phi.tolist() == [1.0] * 4
    for bad in (SimpleNamespace(n=6, fea_dim=4, ctx=SimpleNamespace(device=0)),
                SimpleNamespace(n=7, fea_dim=5, ctx=SimpleNamespace(device=0)),
                SimpleNamespace(n=7, fea_dim=4, ctx=SimpleNamespace(device=1))):
        stages.xv = None
        with pytest.raises(ValueError, match='project_device'):
            stages.project_device([3, 4], bad, models, 4)
        assert stages.xv is None
    with pytest.raises(ValueError, match='without x-vectors'):
        stages.project_device([3], None, models, 4)
    stages.project_device([], None, models, 4)
    assert stages.xv is None and stages.T == []
