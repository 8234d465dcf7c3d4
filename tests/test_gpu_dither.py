"""The dither drawn on the GPU (vbx_fbank.hpp:fbank_dither_kernel through FrontEnd.run_raw) against numpy's generator
(fbank.dither): the same bits in the signal, hence in the features, the windows and predict's output files.  Every
comparison is np.array_equal."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from vbx_amd import _capi, fbank

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 16000
SIZES = [1, 2, 311, 312, 313, 623, 624, 625, 937, 100003]      # 312 doubles are one twist; the last is 321 twists
SEEDS = [3, 0, 2 ** 32 - 1]
LEVELS = [8, 1]


def _samples(n, seed):
    """random int16 values that include both ends of the range (one of them where n = 1)"""
    x = np.random.default_rng(seed).integers(-32768, 32768, n).astype(np.int64)
    x[0] = -32768
    x[-1] = 32767 if n > 1 else x[-1]
    return x


def _whole(n, sr=SR):
    """the recording as one segment"""
    return [fbank.Segment(0, 0, n, fbank.n_frames(n, sr), (0, n))]


@pytest.fixture(scope='module')
def fe():
    return fbank.front_end(SR)


@pytest.mark.parametrize('level', LEVELS)
@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('n', SIZES)
def test_signal_of_one_recording(fe, n, seed, level):
    x = _samples(n, n)
    if n >= 400:
        recs = [(x, _whole(n))]
    else:                                                        # too short for a segment: a second recording holds one
        recs = [(x, []), (_samples(1000, 1), _whole(1000))]
    fe.run_raw(recs, seed=seed, level=level)
    off = 0
    for r, _ in recs:
        got = fe.signal(off, len(r))
        assert got.dtype == np.float64 and np.array_equal(got, fbank.dither(r, seed, level))
        off += len(r)


def test_signal_of_several_recordings(fe):
    xs = [_samples(n, 10 + n) for n in (313, 5000, 1)]
    fe.run_raw([(xs[0], []), (xs[1], _whole(5000)), (xs[2], [])])
    off = 0
    for x in xs:                                                 # each restarts from the seed, none leaks into the next
        assert np.array_equal(fe.signal(off, len(x)), fbank.dither(x))
        off += len(x)
    assert np.array_equal(fe.signal(0, off), np.concatenate([fbank.dither(x) for x in xs]))


def _speech(sr, seed=5):
    n = int(1.3 * sr)
    x = np.clip(np.round(np.random.default_rng(seed).standard_normal(n) * 2000), -32768, 32767).astype(np.int64)
    labs = (np.array([(0.05, 0.6), (0.7, 1.25)]) * sr).astype(int)
    return x, labs


@pytest.mark.parametrize('sr', [8000, 16000])
def test_features_and_windows_have_the_host_dithers_bits(sr):
    x, labs = _speech(sr)
    f = fbank.front_end(sr)
    sig, segs = fbank.prepare(x, labs, sr)
    assert len(segs) == 2
    f.run([(sig, segs)])
    host = {w: f.get(0, f.rows, w) for w in ('fea', 'logmel')}
    f.run_raw([(x, segs)])
    assert f.dither_time() > 0.0
    assert np.array_equal(f.signal(0, len(x)), sig)
    for w, ref in host.items():
        got = f.get(0, f.rows, w)
        assert got.shape == ref.shape and ref.shape[0] > 100 and np.array_equal(got, ref)
    for a, b in zip(fbank.features([(x, labs)], sr, dither_on='device')[0], fbank.features([(x, labs)], sr)[0]):
        assert np.array_equal(a, b)
    # (a tail of 24 frames per segment besides the full windows)
    plan_d, full_d, full_wd, tails_d = fbank.windows(x, labs, sr, 'r', seg_len=40, seg_jump=8, dither_on='device')
    plan_h, full_h, full_wh, tails_h = fbank.windows(x, labs, sr, 'r', seg_len=40, seg_jump=8, dither_on='host')
    assert plan_d == plan_h and full_d == full_h and len(full_h) > 0 and np.array_equal(full_wd, full_wh)
    assert tails_d.keys() == tails_h.keys() and len(tails_h) > 0
    for length in tails_h:
        assert tails_d[length][0] == tails_h[length][0] and np.array_equal(tails_d[length][1], tails_h[length][1])


def test_run_after_run_raw_is_runs_result(fe):
    x, labs = _speech(SR)
    sig, segs = fbank.prepare(x, labs, SR)
    fe.run([(sig, segs)])
    ref = fe.get(0, fe.rows)
    y = _samples(3 * len(x), 2)                                  # a longer raw run in between: the buffers grow
    fe.run_raw([(y, _whole(len(y)))], seed=1)
    assert fe.rows != len(ref)
    fe.run([(sig, segs)])
    assert fe.dither_time() == 0.0
    assert np.array_equal(fe.signal(0, len(x)), sig) and np.array_equal(fe.get(0, fe.rows), ref)


def test_device_dither_refuses_no_dither():
    x, labs = _speech(SR)
    with pytest.raises(ValueError):
        fbank.features([(x, labs)], SR, dither_signal=False, dither_on='device')
    with pytest.raises(ValueError):
        fbank.features([(x, labs)], SR, dither_on='gpu')


def test_run_raw_refuses_bad_tables(fe):
    x = fbank.raw_samples(_samples(2000, 3))
    seg = np.array([[0, 1000]], dtype=np.int64)
    ok = dict(seeds=[3, 3], levels=[8.0, 8.0], segs=seg)
    assert fe.dev.run_raw(x, [[0, 1000], [1000, 1000]], **ok) > 0
    with pytest.raises(_capi.VbxError, match='overlap'):
        fe.dev.run_raw(x, [[500, 1000], [0, 501]], **ok)
    with pytest.raises(_capi.VbxError, match='outside'):
        fe.dev.run_raw(x, [[0, 1000], [1000, 1001]], **ok)
    with pytest.raises(_capi.VbxError, match='outside'):
        fe.dev.run_raw(x, [[-1, 1000], [1000, 1000]], **ok)
    lib, h = fe.dev._lib, fe.dev._h
    rec = np.array([[0, 2000]], dtype=np.int64)
    seeds, levels, rows = np.array([3], dtype=np.uint32), np.array([8.0]), C.c_int64()
    p = _capi._ptr
    args = [p(x), 1, p(rec), p(seeds), p(levels), 1, p(seg)]
    assert lib.vbx_fbank_run_raw(h, 2000, *args, 150, 149, C.byref(rows)) == 0 and rows.value > 0
    for i in (0, 2, 3, 4, 6):                                    # every pointer in turn
        bad = list(args)
        bad[i] = None
        assert lib.vbx_fbank_run_raw(h, 2000, *bad, 150, 149, C.byref(rows)) != 0
        assert b'NULL' in lib.vbx_last_error(fe.ctx._h)
    bad = list(args)
    bad[1] = 0
    assert lib.vbx_fbank_run_raw(h, 2000, *bad, 150, 149, C.byref(rows)) != 0
    assert b'n_rec' in lib.vbx_last_error(fe.ctx._h)
    with pytest.raises(_capi.VbxError, match='past'):
        fe.dev.signal(1999, 2)
    assert fe.dev.signal(1999, 1).shape == (1,)


RECORDER = '''
import torch
class Recorder(torch.nn.Module):
    def forward(self, x):
        return torch.cat([x.mean(dim=2), x.std(dim=2)], dim=1)
torch.jit.script(Recorder()).save(__import__('sys').argv[1])
'''


def test_cli_writes_the_same_files(tmp_path):
    wav, lab = tmp_path / 'wav', tmp_path / 'lab'
    wav.mkdir()
    lab.mkdir()
    for name, sr in (('a16', 16000), ('b8', 8000)):
        n = 2 * sr
        x = np.clip(np.round(np.random.default_rng(sr).standard_normal(n) * 3000), -32768, 32767).astype(np.int64)
        x[:2] = (-32768, 32767)
        fbank.write_wav(str(wav / f'{name}.wav'), x, sr)
        (lab / f'{name}.lab').write_text('0.050 0.900 sp\n1.000 1.950 sp\n')
    (tmp_path / 'list.txt').write_text('a16\nb8\n')
    model = str(tmp_path / 'recorder.pt')
    (tmp_path / 'make_recorder.py').write_text(RECORDER)              # (TorchScript compiles from a source file)
    env = dict(os.environ, PYTHONPATH=REPO)
    subprocess.run([sys.executable, str(tmp_path / 'make_recorder.py'), model], check=True, env=env, timeout=300)
    out = {}
    for where in ('host', 'device'):
        ark, seg = str(tmp_path / f'{where}.ark'), str(tmp_path / f'{where}.seg')
        res = subprocess.run([sys.executable, '-m', 'vbx_amd.predict', '--gpus', '0', '--model-file', model, '--in-file-list',
                              str(tmp_path / 'list.txt'), '--in-lab-dir', str(lab), '--in-wav-dir', str(wav), '--out-ark-fn',
                              ark, '--out-seg-fn', seg, '--batch-size', '16', '--seg-len', '40', '--seg-jump', '8',
                              '--dither', where], env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-3000:]
        with open(ark, 'rb') as fa, open(seg, 'rb') as fs:
            out[where] = (fa.read(), fs.read())
    assert len(out['host'][0]) > 1000 and out['host'][1].count(b'\n') > 10
    assert out['host'] == out['device']
