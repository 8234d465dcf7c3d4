"""The energy VAD kernels (vbx_vad.hpp) against the referee of tests/vad_ref.py -- -m gpu.

N must be the referee's integers, e one f64 log away from it, and -- since every case keeps its energies at least 1e-9
from the threshold, which the test asserts on the referee first -- the decisions and the segments must be the referee's
exactly: rounding of a log (1e-14) and of a mean over a few thousand terms (1e-11) cannot move e - theta that far."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vad_ref
from vad_ref import ulps

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(vad_ref.cases())
# e: the largest distance measured between the device's log and the referee's (the C library's) on these cases is
# E_ULPS_MEASURED; twice that is asserted.  The bound is there to catch a wrong formula, not to police either libm.
E_ULPS_MEASURED = 1


def device(xs, sr, **params):
    from vbx_amd import vad
    return vad.energy_vad(xs, sr, device=0, details=True, **params)


def same(det, runs, ref):
    assert det['N'].dtype == np.int64 and [int(v) for v in det['N']] == ref['N']
    d = ulps(det['e'], ref['e'])
    assert d <= 2 * E_ULPS_MEASURED, d
    assert abs(det['theta'] - ref['theta']) <= 1e-11
    assert np.array_equal(det['raw'], ref['raw'])
    assert runs.dtype == np.int32 and runs.shape == ref['runs'].shape and np.array_equal(runs, ref['runs'])
    return d


@pytest.mark.parametrize('name', CASES)
def test_device_equals_the_referee(name):
    sr, x, params, expect = vad_ref.cases()[name]
    ref = vad_ref.reference(name)
    assert ref['margin'] >= 1e-9
    runs, det = device([x], sr, **params)
    print(f'{name}: T {len(ref["N"])}, {len(ref["runs"])} segments, e within {same(det[0], runs[0], ref)} ulps')
    if expect is not None:
        assert [tuple(r) for r in runs[0].tolist()] == expect


def test_largest_distance_of_e_in_ulps():
    """The figure DESIGN section 19 quotes, over all cases in two calls."""
    worst = 0
    for sr in (16000, 8000):
        names = [n for n in CASES if vad_ref.cases()[n][0] == sr and not vad_ref.cases()[n][2]]      # (e does not depend on the parameters)
        _, det = device([vad_ref.cases()[n][1] for n in names], sr)
        worst = max([worst] + [ulps(d['e'], vad_ref.reference(n)['e']) for n, d in zip(names, det)])
    print(f'largest |e_device - e_referee| = {worst} ulps')
    assert worst <= 2 * E_ULPS_MEASURED


@pytest.mark.parametrize('sr', [16000, 8000])
def test_recordings_at_every_sample_offset_inside_the_batch(sr):
    """A recording that starts at an odd sample, and at every other residue of the eight samples of a 16-byte chunk."""
    k = f'{sr // 1000}k'
    target, floor = f'T257-{k}', f'floor-{k}'
    x = vad_ref.cases()[target][1]
    assert len(x) % 8 == 0 and len(vad_ref.cases()[floor][1]) % 2 == 1
    batch, where, off, offsets = [], [], 0, set()
    for fill in [vad_ref.cases()[floor][1]] + [vad_ref.uniform(seed, 1) for seed in range(7)]:
        batch += [fill, x]
        off += len(fill)
        where.append(len(batch) - 1)
        offsets.add(off % 8)
        off += len(x)
    assert offsets == set(range(8)) and any(o & 1 for o in offsets)
    runs, det = device(batch, sr)
    for i in where:
        same(det[i], runs[i], vad_ref.reference(target))
    same(det[0], runs[0], vad_ref.reference(floor))
    assert all(len(det[i]['N']) == 0 and len(runs[i]) == 0 for i in range(2, len(batch), 2))


@pytest.mark.parametrize('sr', [16000, 8000])
def test_a_recording_gives_the_same_bits_anywhere_in_any_batch(sr):
    k = f'{sr // 1000}k'
    # ends voiced | begins voiced | no frame | an odd number of samples | more frames than one boundary pass | nothing at all
    names = [f'one_merge-{k}', f'starts_hot-{k}', f'n{vad_ref.GEOMETRY[sr][0] - 1}-{k}', f'floor-{k}', f'long-{k}', f'n0-{k}']
    xs = [vad_ref.cases()[n][1] for n in names]
    # (the defaults here, whatever the case was made for: the referee once more where they differ)
    refs = [vad_ref.energy_vad(x, sr) if vad_ref.cases()[n][2] else vad_ref.reference(n) for n, x in zip(names, xs)]
    assert refs[0]['raw'][-1] == 1 and refs[1]['raw'][0] == 1 and len(refs[2]['N']) == 0 and len(xs[3]) % 2 == 1
    assert all(r['margin'] >= 1e-9 for r in refs)
    alone = [device([x], sr) for x in xs]
    for ref, (runs, det) in zip(refs, alone):
        same(det[0], runs[0], ref)
    places = {i: set() for i in range(len(xs))}
    for shift in range(len(xs)):                                      # every rotation: each recording first, last and in between
        order = [(i + shift) % len(xs) for i in range(len(xs))]
        runs, det = device([xs[i] for i in order], sr)
        for pos, i in enumerate(order):
            places[i].add('first' if pos == 0 else 'last' if pos == len(xs) - 1 else 'middle')
            a_runs, a_det = alone[i][0][0], alone[i][1][0]
            assert np.array_equal(runs[pos], a_runs) and runs[pos].dtype == a_runs.dtype
            for key in ('N', 'e', 'raw'):
                assert det[pos][key].tobytes() == a_det[key].tobytes(), (names[i], pos, key)
            assert np.float64(det[pos]['theta']).tobytes() == np.float64(a_det['theta']).tobytes(), (names[i], pos)
    assert all(p == {'first', 'middle', 'last'} for p in places.values())


def test_results_without_details_and_refusals():
    from vbx_amd import _capi, vad
    x = vad_ref.cases()['gap30-16k'][1]
    runs = vad.energy_vad([x, x[:100], x], 16000, device=0, context=0, proportion=0.5)
    assert [r.tolist() for r in runs] == [[[8, 50], [80, 122]], [], [[8, 50], [80, 122]]]
    times = {}
    vad.energy_vad([x], 16000, device=0, times=times)
    assert set(times) == {'upload', 'kernels'} and times['upload'] > 0 and times['kernels'] > 0
    ctx = _capi.default_context(0)
    for rec, winlen, kw, msg in (([[0, len(x) + 1]], 400, {}, 'outside'), ([[-1, 10]], 400, {}, 'outside'), ([[0, len(x)]], 512, {}, 'not built'),
                                 ([[0, len(x)]], 400, dict(context=-1), r'\[0, 2\^30\]'), ([[0, len(x)]], 400, dict(proportion=float('nan')), 'finite')):
        p = dict(vad.DEFAULTS, **kw)
        with pytest.raises(_capi.VbxError, match=msg):
            _capi.vad_energy(ctx, x, np.array(rec, dtype=np.int64), winlen, 160, p['energy_threshold'], p['mean_scale'], p['context'],
                             p['proportion'], p['min_silence'], p['min_speech'], p['pad'])


def test_command_line_end_to_end(tmp_path):
    from vbx_amd import fbank
    names = {'talk': 'bursts43-16k', 'still': 'zero-16k', 'phone': 'bursts42-8k'}
    os.makedirs(tmp_path / 'wav')
    for fn, case in names.items():
        sr, x, _, _ = vad_ref.cases()[case]
        fbank.write_wav(str(tmp_path / 'wav' / f'{fn}.wav'), x, sr)
    (tmp_path / 'list').write_text(''.join(f'{fn}\n' for fn in names))
    res = subprocess.run([sys.executable, '-m', 'vbx_amd.vad', '--device', '0', '--in-file-list', str(tmp_path / 'list'), '--in-wav-dir',
                          str(tmp_path / 'wav'), '--out-lab-dir', str(tmp_path / 'lab'), '--out-file-list', str(tmp_path / 'kept')],
                         env=dict(os.environ, PYTHONPATH=REPO), cwd=REPO, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    assert 'still: no speech found' in res.stderr
    assert sorted(os.listdir(tmp_path / 'lab')) == ['phone.lab', 'talk.lab']
    assert (tmp_path / 'kept').read_text() == 'talk\nphone\n'
    for fn in ('talk', 'phone'):
        sr = vad_ref.cases()[names[fn]][0]
        text = vad_ref.lab_text(vad_ref.reference(names[fn])['runs'], sr)
        assert (tmp_path / 'lab' / f'{fn}.lab').read_text() == text and text.count('\n') > 5
        assert len(fbank.segments(fbank.read_lab(str(tmp_path / 'lab' / f'{fn}.lab'), sr), len(vad_ref.cases()[names[fn]][1]), sr)) == text.count('\n')


def test_wav_files_to_rttm_with_no_labels_but_the_ones_found(tmp_path):
    """``python -m vbx_amd.vad`` then ``python -m vbx_amd.diarize --in-lab-dir <its output>``: generated voices taking turns over
    near-silence, the models, and nothing else."""
    import diarize_util as du
    from vbx_amd import fbank
    recs = {'recA': du.synth_recording(1, 16000, 20, 2), 'recC': du.synth_recording(3, 8000, 15, 2)}
    rates = {'recA': 16000, 'recC': 8000}
    p = du.write_corpus(tmp_path, {fn: (x, rates[fn], lab) for fn, (x, lab, _) in recs.items()})
    p.update(du.write_models(tmp_path), ckpt=du.write_checkpoint(tmp_path), found=str(tmp_path / 'found'), kept=str(tmp_path / 'kept'),
             out=str(tmp_path / 'rttm'))
    env = dict(os.environ, PYTHONPATH=REPO)
    res = subprocess.run([sys.executable, '-m', 'vbx_amd.vad', '--device', '0', '--in-file-list', p['list'], '--in-wav-dir', p['wav'],
                          '--out-lab-dir', p['found'], '--out-file-list', p['kept']], env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    assert open(p['kept']).read() == 'recA\nrecC\n'
    for fn, (x, _, turns) in recs.items():
        labs = fbank.read_lab(os.path.join(p['found'], f'{fn}.lab'), rates[fn]) / rates[fn]
        for a, b, _ in turns:                                         # every turn, but for its fades, lies inside one segment found
            assert any(s <= a + 0.05 and b - 0.05 <= e for s, e in labs), (fn, a, b)
        assert labs[0, 0] > 0.1 and labs[-1, 1] < len(x) / rates[fn] - 0.1          # the near-silence at either end is left out
    res = subprocess.run([sys.executable, '-m', 'vbx_amd.diarize', '--gpus', '0', '--checkpoint', p['ckpt'], '--in-file-list', p['kept'],
                          '--in-lab-dir', p['found'], '--in-wav-dir', p['wav'], '--batch-size', '16', '--out-rttm-dir', p['out'],
                          '--xvec-transform', p['transform'], '--plda-file', p['plda'], '--init', 'AHC+VB', '--threshold', '0.0', '--lda-dim', '128',
                          '--Fa', '4.0', '--Fb', '1.0', '--loopP', '0.99'], env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    rttm = du.rttm_dir(p['out'])
    assert sorted(rttm) == ['recA.rttm', 'recC.rttm'] and all(du.rttm_speakers_and_lines(v)[1] >= 1 for v in rttm.values())
