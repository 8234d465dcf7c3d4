"""The filterbank front end on the GPU (vbx_fbank.hpp) and python -m vbx_amd.predict against the unmodified predict.py
(tests/golden/fbank_cases.npz, tests/golden/make_golden_fbank.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from vbx_amd import fbank
from vbx_amd import kaldi_formats as kf

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(REPO, 'tests', 'golden', 'fbank_cases.npz'))
NAMES = [str(n) for n in G['names']]
RATE = dict(zip(NAMES, (int(r) for r in G['rates'])))


def _rec(name):
    sr = RATE[name]
    labs = np.atleast_2d((np.loadtxt(str(G['lab_' + name]).splitlines(), usecols=(0, 1)) * sr).astype(int))
    return G['sig_' + name].astype(np.int64), labs, sr


def _seg_fea(name):
    rows = G['rows_' + name]
    off = np.concatenate([[0], np.cumsum(rows)])
    return [G['fea_' + name][off[i]:off[i + 1]] for i in range(len(rows))]


@pytest.mark.parametrize('name', [n for n in NAMES if not n.startswith('tone')])
def test_features_match_the_reference(name):
    x, labs, sr = _rec(name)
    got = fbank.features([(x, labs)], sr)[0]
    ref = _seg_fea(name)
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert g.shape == r.shape and g.dtype == np.float32
        assert np.abs(g - r).max() <= 4e-6


@pytest.mark.parametrize('name', ['tone16', 'tone8'])
def test_loud_tone_needs_the_f64_transform(name):
    x, labs, sr = _rec(name)
    fe = fbank.front_end(sr)
    sig, segs = fbank.prepare(x, labs, sr)
    rows = fe.run([(sig, segs)])[0]
    lm = fe.get(rows[0], segs[0].nframes, which='logmel')
    ref = G['logmel_' + name]                                         # (the first rows of the segment)
    assert np.abs(lm[:len(ref)] - ref).max() <= 1e-6                  # (the power spectrum is kept in f32 for the Mel sum)
    assert np.abs(fe.get(rows[0], segs[0].nframes) - _seg_fea(name)[0]).max() <= 4e-6


@pytest.mark.parametrize('name', ['rec16', 'rec8'])
def test_windows_are_slices_of_the_features(name):
    x, labs, sr = _rec(name)
    plan, full, full_w, tails = fbank.windows(x, labs, sr, name)
    fea = fbank.features([(x, labs)], sr)[0]
    assert full_w.shape == (len(full), 64, 144)
    for j, i in enumerate(full):
        w = plan[i]
        assert np.array_equal(full_w[j], fea[w.seg][w.start:w.end].T)
    n_tail = 0
    for length, (idx, arr) in tails.items():
        for j, i in enumerate(idx):
            w = plan[i]
            assert np.array_equal(arr[j], fea[w.seg][w.start:w.end].T)
            n_tail += 1
    assert len(full) + n_tail == len(plan) and n_tail > 0


def test_multi_recording_call_equals_single_calls():
    recs = [_rec(n) for n in NAMES if RATE[n] == 16000]
    together = fbank.features([(x, labs) for x, labs, _ in recs], 16000)
    for (x, labs, sr), t in zip(recs, together):
        alone = fbank.features([(x, labs)], sr)[0]
        assert len(alone) == len(t) and all(np.array_equal(a, b) for a, b in zip(alone, t))


DEVICE_DST = '''
import sys
import numpy as np
import torch                                          # first: libvbx_hip.so then binds to PyTorch's HIP runtime
sys.path.insert(0, sys.argv[1])
from vbx_amd import fbank
g = np.load(sys.argv[2])
sr = 16000
labs = np.atleast_2d((np.loadtxt(str(g['lab_rec16']).splitlines(), usecols=(0, 1)) * sr).astype(int))
fe = fbank.front_end(sr)
sig, segs = fbank.prepare(g['sig_rec16'].astype(np.int64), labs, sr)
fe.run([(sig, segs)])
host = fe.get(0, fe.rows)
dev = fe.get(0, fe.rows, out='torch')
assert dev.device.type == 'cuda' and np.array_equal(dev.cpu().numpy(), host)
wh = fe.windows([0, 5, 100], 144)
wd = fe.windows([0, 5, 100], 144, out='torch')
assert wd.shape == (3, 64, 144) and np.array_equal(wd.cpu().numpy(), wh)
fe.run([(sig, segs)])
assert np.array_equal(fe.get(0, fe.rows), host)
print('device destination OK')
'''


def test_device_destination_and_repeat_runs_are_bit_identical():
    # a process of its own: torch has to be imported before the library binds to a HIP runtime
    res = subprocess.run([sys.executable, '-c', DEVICE_DST, REPO, os.path.join(REPO, 'tests', 'golden', 'fbank_cases.npz')],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'device destination OK' in res.stdout, res.stderr[-3000:]


def test_no_dither_runs():
    x, labs, sr = _rec('rec8')
    a = fbank.features([(x, labs)], sr, dither_signal=False)[0]
    b = fbank.features([(x, labs)], sr)[0]
    assert all(np.isfinite(s).all() for s in a)
    assert [s.shape for s in a] == [s.shape for s in b]
    assert any(not np.array_equal(s, t) for s, t in zip(a, b))


RECORDER = '''
import torch
class Recorder(torch.nn.Module):
    def forward(self, x):
        return torch.cat([x.mean(dim=2), x.std(dim=2)], dim=1)
torch.jit.script(Recorder()).save(__import__('sys').argv[1])
'''


def test_cli_reproduces_predict_py(tmp_path):
    wav, lab = tmp_path / 'wav', tmp_path / 'lab'
    wav.mkdir()
    lab.mkdir()
    for name in NAMES:
        fbank.write_wav(str(wav / f'{name}.wav'), G['sig_' + name], RATE[name])
        (lab / f'{name}.lab').write_text(str(G['lab_' + name]))
    (tmp_path / 'list.txt').write_text(''.join(n + '\n' for n in NAMES))
    model = str(tmp_path / 'recorder.pt')
    (tmp_path / 'make_recorder.py').write_text(RECORDER)              # (TorchScript compiles from a source file)
    env = dict(os.environ, PYTHONPATH=REPO)
    subprocess.run([sys.executable, str(tmp_path / 'make_recorder.py'), model], check=True, env=env, timeout=300)
    ark, seg = str(tmp_path / 'out.ark'), str(tmp_path / 'out.seg')
    res = subprocess.run([sys.executable, '-m', 'vbx_amd.predict', '--gpus', '0', '--model-file', model, '--in-file-list',
                          str(tmp_path / 'list.txt'), '--in-lab-dir', str(lab), '--in-wav-dir', str(wav), '--out-ark-fn', ark,
                          '--out-seg-fn', seg, '--batch-size', '16'], env=env, cwd=REPO, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    with open(seg) as f:
        assert f.read() == str(G['segments'])
    ref_path = str(tmp_path / 'ref.ark')
    G['ark'].tofile(ref_path)
    got, ref = list(kf.read_vec_flt_ark(ark)), list(kf.read_vec_flt_ark(ref_path))
    assert [k for k, _ in got] == [k for k, _ in ref]
    for (_, a), (_, b) in zip(got, ref):
        assert a.dtype == b.dtype == np.float32 and np.abs(a - b).max() <= 1e-5

