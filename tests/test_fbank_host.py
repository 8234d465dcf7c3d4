"""Host side of the filterbank front end (vbx_amd.fbank) against tests/golden/fbank_cases.npz (made by the unmodified
predict.py, tests/golden/make_golden_fbank.py): readers, Mel matrix and window, the window plan and segments-file text,
and the folded f64 frame operator the device runs, applied here in numpy."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from vbx_amd import fbank

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'fbank_cases.npz'))
NAMES = [str(n) for n in G['names']]
RATE = dict(zip(NAMES, (int(r) for r in G['rates'])))


def _files(tmp_path, name):
    wav, lab = tmp_path / f'{name}.wav', tmp_path / f'{name}.lab'
    fbank.write_wav(str(wav), G['sig_' + name], RATE[name])
    lab.write_text(str(G['lab_' + name]))
    return str(wav), str(lab)


@pytest.mark.parametrize('name', NAMES)
def test_readers_match_the_reference_semantics(tmp_path, name):
    wav, lab = _files(tmp_path, name)
    x, sr = fbank.read_wav(wav)
    assert sr == RATE[name] and x.dtype == np.int64
    # (sf.read(...) * 2**15).astype(int) of 16-bit PCM: the int16 values
    assert np.array_equal(x, (G['sig_' + name].astype(np.float64) / 2 ** 15 * 2 ** 15).astype(int))
    labs = fbank.read_lab(lab, sr)
    assert labs.ndim == 2 and labs.shape[1] == 2
    assert np.array_equal(labs, np.atleast_2d((np.loadtxt(lab, usecols=(0, 1)) * sr).astype(int)))


def test_wav_reader_refuses_other_formats(tmp_path):
    p = str(tmp_path / 'x.wav')
    fbank.write_wav(p, np.zeros(100, dtype=np.int16), 44100)
    with pytest.raises(ValueError, match='Only 8kHz and 16kHz'):
        fbank.read_wav(p)
    with wave.open(p, 'wb') as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(b'\0' * 400)
    with pytest.raises(ValueError, match='mono 16-bit'):
        fbank.read_wav(p)


def test_one_line_lab(tmp_path):
    p = tmp_path / 'one.lab'
    p.write_text('0.50 1.25 sp\n')
    assert fbank.read_lab(str(p), 16000).tolist() == [[8000, 20000]]


@pytest.mark.parametrize('sr', [16000, 8000])
def test_mel_matrix_and_window(sr):
    g = fbank.geometry(sr)
    assert np.abs(fbank.mel_matrix(sr) - G[f'mel_{sr}']).max() <= 1e-15
    assert np.abs(fbank.povey_window(g['winlen']) - G[f'window_{sr}']).max() <= 1e-15


def test_dither_is_numpy_legacy_stream():
    x = np.arange(1000)
    np.random.seed(3)
    ref = x + 8 * (np.random.rand(1000) * 2 - 1)
    assert np.array_equal(fbank.dither(x), ref)


def _plan_text():
    text = ''
    for name in NAMES:
        sr = RATE[name]
        labs = np.atleast_2d((np.loadtxt(str(G['lab_' + name]).splitlines(), usecols=(0, 1)) * sr).astype(int))
        segs = fbank.segments(labs, len(G['sig_' + name]), sr)
        assert [s.nframes for s in segs] == G['rows_' + name].tolist()
        text += ''.join(w.line + os.linesep for w in fbank.window_plan(name, segs, sr))
    return text


def test_window_plan_and_segments_text_byte_for_byte():
    assert _plan_text() == str(G['segments'])


@pytest.mark.parametrize('name', NAMES)
def test_folded_operator_reproduces_the_reference(name):
    sr = RATE[name]
    labs = np.atleast_2d((np.loadtxt(str(G['lab_' + name]).splitlines(), usecols=(0, 1)) * sr).astype(int))
    sig = fbank.dither(G['sig_' + name].astype(int))
    segs = fbank.segments(labs, len(sig), sr)
    fea, row = G['fea_' + name], 0
    for j, s in enumerate(segs):
        lm = fbank.host_logmel(fbank.mirror_pad(sig[s.start:s.start + s.n], sr), sr)
        if j == 0:                                  # the fixture keeps the first rows of the first segment's log-Mel
            ref = G['logmel_' + name]
            assert np.abs(lm[:len(ref)] - ref).max() <= 1e-9
        cmn = fbank.host_cmn(lm).astype(np.float32)
        assert np.abs(cmn - fea[row:row + s.nframes]).max() <= 4e-6
        row += s.nframes
    assert row == len(fea)


def test_cli_refusals(tmp_path):
    base = ['--in-file-list', 'l', '--in-lab-dir', 'd', '--in-wav-dir', 'd', '--out-ark-fn', 'a', '--out-seg-fn', 's']
    for extra, msg in ((['--gpus', '', '--model-file', 'm'], '--gpus is empty'),
                       (['--gpus', '0', '--backend', 'onnx', '--weights', 'w'], 'onnx is not supported'),
                       (['--gpus', '0', '--model', 'ResNet101', '--weights', 'w'], '--model/--weights are not supported')):
        res = subprocess.run([sys.executable, '-m', 'vbx_amd.predict'] + base + extra, cwd=REPO, capture_output=True,
                             text=True, timeout=120)
        assert res.returncode != 0 and msg in res.stderr
