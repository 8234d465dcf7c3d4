"""The x-vector network in its split mode (ResNet101(sd, gemm='split'): vbx_resnet_split.hpp) on the GPU, held to what
tests/test_gpu_xvector.py holds the exact mode to, with the same fixture (tests/golden/resnet_cases.npz)."""
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
R = np.load(os.path.join(REPO, 'tests', 'golden', 'resnet_cases.npz'))
F = np.load(os.path.join(REPO, 'tests', 'golden', 'fbank_cases.npz'))
SEED, E = int(R['seed']), int(R['embed_dim'])
NAMES = [str(n) for n in F['names']]


def window(j):
    name = NAMES[R['win_rec'][j]]
    rows = F['rows_' + name]
    s, a, n = int(R['win_seg'][j]), int(R['win_start'][j]), int(R['win_len'][j])
    r0 = int(rows[:s].sum())
    return F['fea_' + name][r0 + a:r0 + a + n].T


@pytest.fixture(scope='module')
def sd():
    return xvector.synthetic_state_dict(SEED, E)


@pytest.fixture(scope='module')
def net(sd):
    return xvector.ResNet101.from_checkpoint(sd, gemm='split')


@pytest.fixture(scope='module')
def exact(sd):
    return xvector.ResNet101(sd)


@pytest.fixture(scope='module')
def full():
    """the fixture's full windows [n][64][144]"""
    return np.stack([window(j) for j in np.flatnonzero(R['win_len'] == 144)])


def test_fixture_windows_match_the_reference(net):
    """The exact mode's tolerances.  Measured on an MI355X: 6.8e-6 of the reference's embeddings, 6.6e-6 of the f64 referee
    (the exact mode on the same device: 8.3e-6 and 7.9e-6)."""
    got = np.empty((len(R['win_len']), E), dtype=np.float32)
    for n in sorted(set(R['win_len'].tolist())):
        idx = np.flatnonzero(R['win_len'] == n)
        got[idx] = net.embed(np.stack([window(j) for j in idx]))
    assert net.gemm_in_effect() == 'split'
    assert got.dtype == np.float32 and np.isfinite(got).all()
    worst_ref = worst_f64 = 0.0
    for j in range(len(got)):
        scale = np.abs(R['emb_f64'][j]).max()
        worst_ref = max(worst_ref, np.abs(got[j] - R['emb_ref'][j]).max() / scale)
        worst_f64 = max(worst_f64, np.abs(got[j] - R['emb_f64'][j]).max() / scale)
    print('split mode, 41 fixture windows: max |e - e_ref| / max|e| = %.2e, max |e - e_f64| / max|e| = %.2e' % (worst_ref, worst_f64))
    for j in range(len(got)):
        scale = np.abs(R['emb_f64'][j]).max()
        assert np.abs(got[j] - R['emb_ref'][j]).max() <= 2e-5 * scale, j
        assert np.abs(got[j] - R['emb_f64'][j]).max() <= 1e-5 * scale, j


def test_the_default_is_the_exact_mode_and_keeps_its_bits(sd, exact, net, full):
    named = xvector.ResNet101(sd, gemm='exact')
    a, b = exact.embed(full[:5]), named.embed(full[:5])
    assert exact.gemm_in_effect() == 'exact' and named.gemm_in_effect() == 'exact'
    assert np.array_equal(a, b)
    c = net.embed(full[:5])
    assert net.gemm_in_effect() == 'split'
    assert not np.array_equal(a, c)                           # (another arithmetic: the split mode does run)
    assert np.abs(a - c).max() <= 2e-5 * np.abs(a).max()      # each is within 1e-5 of the f64 referee
    # switching an existing network: back and forth gives each mode's own bits again
    named.dev.set_gemm('split')
    assert np.array_equal(named.embed(full[:5]), c) and named.gemm_in_effect() == 'split'
    named.dev.set_gemm('exact')
    assert np.array_equal(named.embed(full[:5]), a) and named.gemm_in_effect() == 'exact'
    with pytest.raises(ValueError):
        xvector.ResNet101(sd, gemm='f16')


def test_batch_invariance(net, full):
    rng = np.random.default_rng(11)
    batch = np.concatenate([full, full[:, :, ::-1] + 0.1 * rng.standard_normal(full.shape)]).astype(np.float32)
    batch = batch[rng.integers(0, len(batch), 128)]
    batch[::3] *= np.float32(2.0 ** 12)                       # neighbours of another scale: a batch-wide scale would show
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
def test_production_shapes(net, exact, full, n, T):
    """The batches of test_gpu_xvector.py::test_production_shapes: every window bit-equal to its own run alone, and within
    2e-5 max|e| of the exact mode on the same device (each mode is within 1e-5 of the f64 referee)."""
    rng = np.random.default_rng(1000 * n + T)
    x = full[rng.integers(0, len(full), n)][:, :, :T] + 0.1 * rng.standard_normal((n, 64, T))
    x = x.astype(np.float32)
    got = net.embed(x)
    assert got.shape == (n, E) and got.dtype == np.float32 and np.isfinite(got).all()
    for i in sorted({0, 1, n // 2, n - 1}):
        assert np.array_equal(got[i], net.embed(x[i:i + 1])[0]), i
    want = exact.embed(x)
    for i in range(n):
        assert np.abs(got[i] - want[i]).max() <= 2e-5 * np.abs(want[i]).max(), i


def test_cli_with_gemm_split_reproduces_predict_py(tmp_path, sd):
    import torch
    wav, lab = tmp_path / 'wav', tmp_path / 'lab'
    wav.mkdir()
    lab.mkdir()
    for name, sr in zip(NAMES, F['rates']):
        fbank.write_wav(str(wav / f'{name}.wav'), F['sig_' + name], int(sr))
        (lab / f'{name}.lab').write_text(str(F['lab_' + name]))
    (tmp_path / 'list.txt').write_text(''.join(n + '\n' for n in NAMES))
    ck = str(tmp_path / 'ckpt.pth')
    torch.save({'state_dict': {k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
    ark, seg = str(tmp_path / 'out.ark'), str(tmp_path / 'out.seg')
    env = dict(os.environ, PYTHONPATH=REPO)
    res = subprocess.run([sys.executable, '-m', 'vbx_amd.predict', '--gpus', '0', '--checkpoint', ck, '--gemm', 'split',
                          '--in-file-list', str(tmp_path / 'list.txt'), '--in-lab-dir', str(lab), '--in-wav-dir', str(wav),
                          '--out-ark-fn', ark, '--out-seg-fn', seg, '--batch-size', '16'], env=env, cwd=REPO, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    with open(seg) as f:
        assert f.read() == str(R['segments'])
    ref_path = str(tmp_path / 'ref.ark')
    R['ark'].tofile(ref_path)
    got, ref = list(kf.read_vec_flt_ark(ark)), list(kf.read_vec_flt_ark(ref_path))
    assert [k for k, _ in got] == [k for k, _ in ref]
    for (_, a), (_, b) in zip(got, ref):
        assert a.dtype == b.dtype == np.float32 and np.abs(a - b).max() <= 5e-5 * np.abs(b).max()
