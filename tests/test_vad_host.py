"""The energy VAD without a GPU: the numpy path of vbx_amd/vad.py against the referee of tests/vad_ref.py
on every case the GPU tests run, the hand-derived expectations of those cases, the command line, the .lab text and its way
back through fbank.read_lab into fbank.segments, and the ABI."""
import os
import re

import numpy as np
import pytest

import vad_ref
from vad_ref import ulps
from vbx_amd import fbank, vad

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(vad_ref.cases())


def test_the_cases_cover_the_kernel_edges():
    from vbx_amd import _capi
    frames = {name: len(vad_ref.reference(name)['N']) for name in CASES}
    for k in ('16k', '8k'):
        assert [frames[f'T{t}-{k}'] for t in (255, 256, 257, 512)] == [_capi.VAD_TILE - 1, _capi.VAD_TILE, _capi.VAD_TILE + 1, 2 * _capi.VAD_TILE]
        L, H = vad_ref.GEOMETRY[int(k[:-1]) * 1000]
        assert [frames[f'n{n}-{k}'] for n in (0, L - 1, L, L + H - 1, L + H)] == [0, 0, 1, 1, 2]
        assert frames[f'long-{k}'] > _capi.VAD_RUN_PASS and frames[f'many_merges-{k}'] > _capi.VAD_RUN_PASS
        assert any(a < _capi.VAD_RUN_PASS < b for a, b in vad_ref.reference(f'long-{k}')['runs'])
        assert len(vad_ref.reference(f'many_runs-{k}')['runs']) > _capi.VAD_RUN_BLOCK
        raw_runs = vad_ref.maximal_runs(list(vad_ref.reference(f'many_merges-{k}')['raw']), 1)
        assert len(raw_runs) > _capi.VAD_RUN_BLOCK and len(vad_ref.reference(f'many_merges-{k}')['runs']) < len(raw_runs) // 2
        # the largest sums: every frame of the constant -32768 has N = 0 from two terms of L^2 2^30
        assert set(vad_ref.reference(f'floor-{k}')['N']) == {0}
        # the window of the first and the last frames is cut by the recording, one in between straddles a tile edge
        ref = vad_ref.reference(f'tile_edge-{k}')
        assert ref['raw'][_capi.VAD_TILE - 1] and ref['raw'][_capi.VAD_TILE] and ref['raw'][-1] and not ref['e'][-1] > ref['theta']
    assert 5 * 0.6 == 3.0                                            # prop_exact: three hot frames of five meet the product exactly


@pytest.mark.parametrize('name', CASES)
def test_referee_meets_the_expectations_written_by_hand(name):
    sr, x, params, expect = vad_ref.cases()[name]
    ref = vad_ref.reference(name)
    assert ref['margin'] >= 1e-9                                     # no energy near enough to the threshold for rounding to matter
    if expect is not None:
        assert [tuple(r) for r in ref['runs'].tolist()] == expect
    if 'below' in name:
        assert (ref['e'] < ref['theta']).all() and len(ref['e']) == 300
    if 'above' in name:
        assert (ref['e'] > ref['theta']).all() and len(ref['e']) == 300
    if params.get('context') == 0:                                   # the crafted gaps and runs are what their names say
        raw_runs = vad_ref.maximal_runs(list(ref['raw']), 1)
        gaps = [b[0] - a[1] for a, b in zip(raw_runs, raw_runs[1:])]
        lens = [b - a for a, b in raw_runs]
        want = {'gap29': (gaps, [29]), 'gap30': (gaps, [30]), 'speech19': (lens, [19]), 'speech20': (lens, [20]),
                'rescued': (lens, [7, 42, 7]), 'pad_merge': (gaps, [40])}.get(name.split('-')[0])
        if want:
            assert want[0] == want[1]


@pytest.mark.parametrize('name', CASES)
def test_numpy_path_equals_the_referee(name):
    sr, x, params, _ = vad_ref.cases()[name]
    ref = vad_ref.reference(name)
    runs, det = vad.energy_vad([x], sr, details=True, **params)
    assert len(runs) == len(det) == 1
    assert runs[0].dtype == np.int32 and runs[0].shape == ref['runs'].shape and np.array_equal(runs[0], ref['runs'])
    assert det[0]['N'].dtype == np.int64 and [int(v) for v in det[0]['N']] == ref['N']
    # one f64 log of identical inputs on both sides, numpy's and the C library's: each within an ulp of the true value
    assert ulps(det[0]['e'], ref['e']) <= 2
    assert abs(det[0]['theta'] - ref['theta']) <= 1e-11              # a mean of a few thousand such terms
    assert np.array_equal(det[0]['raw'], ref['raw'])
    assert np.array_equal(vad.energy_vad([x], sr, **params)[0], ref['runs'])


def test_batches_of_recordings_and_bad_arguments():
    names = ['gap30-16k', 'n0-16k', 'bursts41-16k']
    got = vad.energy_vad([vad_ref.cases()[n][1] for n in names], 16000)
    want = [vad.energy_vad([vad_ref.cases()[n][1]], 16000)[0] for n in names]
    assert len(got) == 3 and all(np.array_equal(g, w) for g, w in zip(got, want)) and got[1].shape == (0, 2)
    assert vad.energy_vad([], 16000) == [] and vad.energy_vad([], 16000, details=True) == ([], [])
    with pytest.raises(ValueError, match='integers'):
        vad.energy_vad([np.zeros(1000)], 16000)
    with pytest.raises(ValueError, match='8kHz and 16kHz'):
        vad.energy_vad([np.zeros(1000, dtype=np.int16)], 44100)
    for bad in (dict(context=-1), dict(min_silence=1.5), dict(pad=2 ** 31), dict(proportion=float('nan')), dict(mean_scale=float('inf'))):
        with pytest.raises(ValueError):
            vad.energy_vad([np.zeros(1000, dtype=np.int16)], 16000, **bad)
    assert vad.batches([5, 5, 5, 20, 1, 1], budget=10) == [[0, 1], [2], [3], [4, 5]] and vad.batches([]) == []


# ---- command line -----------------------------------------------------------------------------------------------------
def test_parser_defaults_and_required_flags(capsys):
    p = vad.build_parser()
    args = p.parse_args(['--in-file-list', 'l', '--in-wav-dir', 'w', '--out-lab-dir', 'd'])
    assert {k: getattr(args, k) for k in vad.DEFAULTS} == vad_ref.DEFAULTS == vad.DEFAULTS == \
        dict(energy_threshold=5.5, mean_scale=0.5, context=2, proportion=0.12, min_silence=30, min_speech=20, pad=0)
    assert args.device is None and args.out_file_list is None
    import inspect
    sig = inspect.signature(vad.energy_vad).parameters
    assert {k: sig[k].default for k in vad.DEFAULTS} == vad.DEFAULTS and sig['device'].default is None and sig['details'].default is False
    for missing in ('--in-file-list', '--in-wav-dir', '--out-lab-dir'):
        argv = [a for flag in ('--in-file-list', '--in-wav-dir', '--out-lab-dir') if flag != missing for a in (flag, 'x')]
        with pytest.raises(SystemExit):
            p.parse_args(argv)
        assert missing in capsys.readouterr().err
    args = p.parse_args(['--in-file-list', 'l', '--in-wav-dir', 'w', '--out-lab-dir', 'd', '--device', '1', '--min-silence', '7',
                         '--min-speech', '3', '--pad', '2', '--context', '4', '--proportion', '0.3', '--energy-threshold', '6',
                         '--mean-scale', '0.25', '--out-file-list', 'f'])
    assert (args.device, args.min_silence, args.min_speech, args.pad, args.context, args.proportion, args.energy_threshold,
            args.mean_scale, args.out_file_list) == (1, 7, 3, 2, 4, 0.3, 6.0, 0.25, 'f')


def test_command_line_on_the_host(tmp_path, capsys):
    names = {'a': 'bursts41-16k', 'b': 'zero-8k', 'c': 'gap30-8k'}
    os.makedirs(tmp_path / 'wav')
    for fn, case in names.items():
        sr, x, _, _ = vad_ref.cases()[case]
        fbank.write_wav(str(tmp_path / 'wav' / f'{fn}.wav'), x, sr)
    (tmp_path / 'list').write_text('a\nb\nc\n')
    assert vad.main(['--in-file-list', str(tmp_path / 'list'), '--in-wav-dir', str(tmp_path / 'wav'), '--out-lab-dir',
                     str(tmp_path / 'lab'), '--out-file-list', str(tmp_path / 'kept')]) == 0
    assert sorted(os.listdir(tmp_path / 'lab')) == ['a.lab', 'c.lab']
    assert (tmp_path / 'kept').read_text() == 'a\nc\n'
    err = capsys.readouterr().err
    assert 'b: no speech found' in err and 'a:' not in err
    for fn in ('a', 'c'):
        sr = vad_ref.cases()[names[fn]][0]
        ref = vad_ref.energy_vad(vad_ref.cases()[names[fn]][1], sr)                  # (gap30 with the default parameters)
        assert (tmp_path / 'lab' / f'{fn}.lab').read_text() == vad_ref.lab_text(ref['runs'], sr) != ''
    with pytest.raises(SystemExit):
        vad.main(['--in-file-list', str(tmp_path / 'list'), '--in-wav-dir', str(tmp_path / 'nowhere'), '--out-lab-dir', str(tmp_path / 'lab2')])
    assert not (tmp_path / 'lab2').exists()


# ---- .lab files ---------------------------------------------------------------------------------------------------------
def test_write_lab_text_and_the_way_back(tmp_path):
    runs = np.array([[0, 7], [123, 4567], [100000, 359999]], dtype=np.int32)
    assert vad.segments_seconds(runs, 16000) == vad.segments_seconds(runs, 8000) == [(0.0, 0.07), (1.23, 45.67), (1000.0, 3599.99)]
    for sr in (16000, 8000):
        path = str(tmp_path / f'x{sr}.lab')
        vad.write_lab(path, runs, sr)
        assert open(path).read() == '0.000 0.070 sp\n1.230 45.670 sp\n1000.000 3599.990 sp\n' == vad.lab_text(runs, sr)
        H = fbank.geometry(sr)['shift']
        back = fbank.read_lab(path, sr)
        assert back.shape == (3, 2) and np.abs(back - runs.astype(np.int64) * H).max() <= 1
        vad.write_lab(path, runs[:1], sr)                            # a single line still reads back as one row
        assert fbank.read_lab(path, sr).shape == (1, 2)
    with pytest.raises(ValueError, match='no segment'):
        vad.write_lab(str(tmp_path / 'none.lab'), np.zeros((0, 2), dtype=np.int32), 16000)
    assert not (tmp_path / 'none.lab').exists()


# frame indices whose printed time, times the rate and truncated as fbank.read_lab does, lands one sample below a * H
# (DESIGN section 19 quotes these counts): the rest come back exactly
ONE_BELOW = {16000: 2356, 8000: 2356}          # (the same indices: a factor of two is exact)


@pytest.mark.parametrize('sr', [16000, 8000])
def test_every_frame_index_survives_the_printed_time_within_one_sample(sr):
    H = fbank.geometry(sr)['shift']
    a = np.arange(400001)
    text = vad.lab_text(np.stack([a, a + 1], axis=1)[[0, 1, 12345, 400000]], sr).split('\n')
    assert text[:4] == ['0.000 0.010 sp', '0.010 0.020 sp', '123.450 123.460 sp', '4000.000 4000.010 sp']
    # what write_lab prints for frame a, read the way read_lab reads it: (float(text) * sr).astype(int)
    printed = np.array([float('%.3f' % (int(v) * H / sr)) for v in a])
    back = (printed * sr).astype(int)
    diff = back - a * H
    print(f'sr {sr}: {int((diff == -1).sum())} of {len(a)} frame indices come back one sample below, {int((diff == 0).sum())} exactly')
    assert diff.min() >= -1 and diff.max() <= 1
    assert int((diff == -1).sum()) == ONE_BELOW[sr] and int((diff == 1).sum()) == 0


def test_fbank_segments_accepts_the_result(tmp_path):
    for name in ('bursts42-16k', 'bursts42-8k'):
        sr, x, _, _ = vad_ref.cases()[name]
        runs = vad.energy_vad([x], sr)[0]
        path = str(tmp_path / f'{name}.lab')
        vad.write_lab(path, runs, sr)
        labs = fbank.read_lab(path, sr)
        segs = fbank.segments(labs, len(x), sr)
        H = fbank.geometry(sr)['shift']
        assert len(segs) == len(runs) > 5
        for s, (a, b) in zip(segs, runs):
            assert abs(s.start - a * H) <= 1 and abs(s.start + s.n - b * H) <= 1 and s.start + s.n <= len(x) and s.nframes > 0
        assert fbank.window_plan(name, segs, sr)                     # and the x-vector windows can be planned on them


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_listed_and_built_from_its_header():
    from vbx_amd import _capi, build
    header = open(os.path.join(REPO, 'include', 'vbx_hip.h')).read()
    assert re.search(r'\bint vbx_vad_energy\s*\(', header) and 'vbx_vad_energy' in _capi.ABI_SYMBOLS
    assert '#define VBX_ABI_VERSION 7' in header
    assert 'vbx_vad.hpp' in build.HEADERS and 'vbx_vad.hpp' not in build.ITERATION_SOURCES
    assert '#include "vbx_vad.hpp"' in open(os.path.join(build.CSRC, 'vbx_capi.hip')).read()
    src = open(os.path.join(build.CSRC, 'vbx_vad.hpp')).read()
    const = {k: int(v) for k, v in re.findall(r'constexpr int (kVad\w+) = (\d+);', src)}
    assert (_capi.VAD_TILE, _capi.VAD_RUN_PASS) == (const['kVadTile'], 256 * const['kVadRunFrames']) and _capi.VAD_RUN_BLOCK == _capi.LABELS_BLOCK
