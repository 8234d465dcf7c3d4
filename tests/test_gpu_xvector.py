"""The x-vector network on the GPU (vbx_resnet.hpp, vbx_amd.xvector.ResNet101) against the unmodified predict.py +
models/resnet.py with a synthetic checkpoint (tests/golden/resnet_cases.npz, tests/golden/make_golden_resnet.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import resnet_shapes as rs
from vbx_amd import fbank, xvector
from vbx_amd import kaldi_formats as kf

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_PATH = os.path.join(REPO, 'tests', 'golden', 'resnet_cases.npz')
F_PATH = os.path.join(REPO, 'tests', 'golden', 'fbank_cases.npz')
R, F = np.load(R_PATH), np.load(F_PATH)
SEED, E = int(R['seed']), int(R['embed_dim'])
NAMES = [str(n) for n in F['names']]


def window(j):
    name = NAMES[R['win_rec'][j]]
    rows = F['rows_' + name]
    s, a, n = int(R['win_seg'][j]), int(R['win_start'][j]), int(R['win_len'][j])
    r0 = int(rows[:s].sum())
    return F['fea_' + name][r0 + a:r0 + a + n].T


@pytest.fixture(scope='module')
def net():
    return xvector.ResNet101.from_checkpoint(xvector.synthetic_state_dict(SEED, E))


@pytest.fixture(scope='module')
def full():
    """the fixture's full windows [n][64][144]"""
    return np.stack([window(j) for j in np.flatnonzero(R['win_len'] == 144)])


def test_fixture_windows_match_the_reference(net):
    got = np.empty((len(R['win_len']), E), dtype=np.float32)
    for n in sorted(set(R['win_len'].tolist())):
        idx = np.flatnonzero(R['win_len'] == n)
        got[idx] = net.embed(np.stack([window(j) for j in idx]))
    assert got.dtype == np.float32 and np.isfinite(got).all()
    for j in range(len(got)):
        scale = np.abs(R['emb_f64'][j]).max()
        assert np.abs(got[j] - R['emb_ref'][j]).max() <= 2e-5 * scale, j
        assert np.abs(got[j] - R['emb_f64'][j]).max() <= 1e-5 * scale, j


def test_batch_invariance(net, full):
    rng = np.random.default_rng(11)
    batch = np.concatenate([full, full[:, :, ::-1] + 0.1 * rng.standard_normal(full.shape)]).astype(np.float32)
    batch = batch[rng.integers(0, len(batch), 128)]
    w = full[3]
    alone = net.embed(w[None])[0]
    for pos in (0, 77, 127):
        b = batch.copy()
        b[pos] = w
        assert np.array_equal(net.embed(b)[pos], alone), pos
    # and a tail window alone vs among its own length
    tails = np.stack([window(j) for j in np.flatnonzero(R['win_len'] == 20)] * 5)
    assert np.array_equal(net.embed(tails)[3], net.embed(tails[3:4])[0])


def test_large_batch_past_2_gib(net, full):
    # 512 full windows: one layer1 activation is 512 x 64 x 144 x 128 x 4 B = 2.4 GB
    assert 512 * 64 * 144 * 128 * 4 > 2 ** 31
    rng = np.random.default_rng(12)
    batch = full[rng.integers(0, len(full), 512)] + 0.05 * rng.standard_normal((512, 64, 144))
    batch = batch.astype(np.float32)
    got = net.embed(batch)
    assert got.shape == (512, E) and np.isfinite(got).all()
    for i in (0, 1, 300, 511):
        assert np.array_equal(got[i], net.embed(batch[i:i + 1])[0]), i


def test_nan_stays_in_its_window(net, full):
    x = full[:4].copy()
    x[2, 17, 40] = np.nan
    got = net.embed(x)
    assert np.isnan(got[2]).all()
    assert np.isfinite(got[[0, 1, 3]]).all()
    assert np.array_equal(got[[0, 1, 3]], net.embed(full[[0, 1, 3]]))


@pytest.mark.parametrize('n,T', rs.NETWORK_RUNS)
def test_production_shapes(net, full, n, T):
    """Batches as predict forms them (the last, short batch of a file; tail windows grouped by length): together with the
    other runs of this file they reach every convolution instantiation and edge path the network can (resnet_shapes,
    tests/test_xvector_host.py).  Every window is bit-equal to its own run alone and within 1e-5 max|e| of the f64 referee."""
    rng = np.random.default_rng(1000 * n + T)
    x = full[rng.integers(0, len(full), n)][:, :, :T] + 0.1 * rng.standard_normal((n, 64, T))
    x = x.astype(np.float32)
    got = net.embed(x)
    assert got.shape == (n, E) and got.dtype == np.float32 and np.isfinite(got).all()
    sd = xvector.synthetic_state_dict(SEED, E)
    for i in range(n):
        assert np.array_equal(got[i], net.embed(x[i:i + 1])[0]), i
    for i0 in range(0, n, 8):
        ref = xvector.forward_reference(sd, x[i0:i0 + 8])
        for i, e in enumerate(ref, i0):
            err, scale = np.abs(got[i] - e).max(), np.abs(e).max()
            assert err <= 1e-5 * scale, (i, err / scale)


DEVICE_INPUTS = '''
import sys
import numpy as np
import torch                                          # first: libvbx_hip.so then binds to PyTorch's HIP runtime
sys.path.insert(0, sys.argv[1])
from vbx_amd import fbank, xvector
g = np.load(sys.argv[2])
r = np.load(sys.argv[3])
net = xvector.ResNet101.from_checkpoint(xvector.synthetic_state_dict(int(r['seed']), int(r['embed_dim'])))
sr = 16000
labs = np.atleast_2d((np.loadtxt(str(g['lab_rec16']).splitlines(), usecols=(0, 1)) * sr).astype(int))
fe = fbank.front_end(sr)
sig, segs = fbank.prepare(g['sig_rec16'].astype(np.int64), labs, sr)
rows = fe.run([(sig, segs)])[0]
for length, starts in ((144, [0, 24, 48, 130]), (26, [3, 7])):
    host = fe.windows(starts, length)
    a = net.embed(host)
    b = net.embed(torch.from_numpy(host).cuda())
    assert b.device.type == 'cuda' and b.dtype == torch.float32
    c = net.embed_windows(fe, starts, length)
    assert np.array_equal(b.cpu().numpy(), a) and np.array_equal(c, a), length
print('device inputs OK')
'''


def test_device_inputs_give_the_same_bits():
    res = subprocess.run([sys.executable, '-c', DEVICE_INPUTS, REPO, F_PATH, R_PATH], capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0 and 'device inputs OK' in res.stdout, res.stderr[-3000:]


def test_cli_with_a_checkpoint_reproduces_predict_py(tmp_path):
    import torch
    wav, lab = tmp_path / 'wav', tmp_path / 'lab'
    wav.mkdir()
    lab.mkdir()
    for name, sr in zip(NAMES, F['rates']):
        fbank.write_wav(str(wav / f'{name}.wav'), F['sig_' + name], int(sr))
        (lab / f'{name}.lab').write_text(str(F['lab_' + name]))
    (tmp_path / 'list.txt').write_text(''.join(n + '\n' for n in NAMES))
    ck = str(tmp_path / 'ckpt.pth')
    sd = xvector.synthetic_state_dict(SEED, E)
    torch.save({'state_dict': {k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
    ark, seg = str(tmp_path / 'out.ark'), str(tmp_path / 'out.seg')
    env = dict(os.environ, PYTHONPATH=REPO)
    res = subprocess.run([sys.executable, '-m', 'vbx_amd.predict', '--gpus', '0', '--checkpoint', ck, '--in-file-list',
                          str(tmp_path / 'list.txt'), '--in-lab-dir', str(lab), '--in-wav-dir', str(wav), '--out-ark-fn', ark,
                          '--out-seg-fn', seg, '--batch-size', '16'], env=env, cwd=REPO, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    with open(seg) as f:
        assert f.read() == str(R['segments'])
    ref_path = str(tmp_path / 'ref.ark')
    R['ark'].tofile(ref_path)
    got, ref = list(kf.read_vec_flt_ark(ark)), list(kf.read_vec_flt_ark(ref_path))
    assert [k for k, _ in got] == [k for k, _ in ref]
    for (_, a), (_, b) in zip(got, ref):
        assert a.dtype == b.dtype == np.float32 and np.abs(a - b).max() <= 5e-5 * np.abs(b).max()
