"""The host side of the device dither (vbx_fbank.hpp:fbank_dither_kernel): the seeding, the sample check, the command
line, and the data-parallel schedule of the MT19937 twist the kernel follows -- all against numpy's own generator."""
import numpy as np
import pytest

from vbx_amd import fbank, predict

N, M = 624, 397


@pytest.mark.parametrize('seed', [0, 3, 2 ** 32 - 1])
def test_seed_state_is_numpys(seed):
    got = fbank.mt19937_seed_state(seed)
    ref = np.random.RandomState(seed).get_state()
    assert got.dtype == np.uint32 and got.shape == (N,)
    assert np.array_equal(got, ref[1]) and ref[2] == N          # (position 624: the first draw twists)


@pytest.mark.parametrize('seed', [-1, 2 ** 32])
def test_seed_state_refuses_what_numpy_refuses(seed):
    with pytest.raises(ValueError):
        np.random.RandomState(seed)
    with pytest.raises(ValueError):
        fbank.mt19937_seed_state(seed)


def test_raw_samples_takes_what_read_wav_returns(tmp_path):
    x = np.array([0, -32768, 32767, 5, -7], dtype=np.int16)
    path = str(tmp_path / 'x.wav')
    fbank.write_wav(path, x, 16000)
    samples, _ = fbank.read_wav(path)
    assert samples.dtype == np.int64
    got = fbank.raw_samples(samples)
    assert got.dtype == np.int16 and np.array_equal(got, x)


@pytest.mark.parametrize('bad', [32768, -32769])
def test_raw_samples_names_the_first_sample_out_of_range(bad):
    x = np.zeros(10, dtype=np.int64)
    x[4] = bad
    x[7] = bad
    with pytest.raises(ValueError, match=rf'sample 4 is {bad}\b'):
        fbank.raw_samples(x)


def test_raw_samples_refuses_floats():
    with pytest.raises(ValueError, match='integers'):
        fbank.raw_samples(np.zeros(4, dtype=np.float64))


BASE = ['--gpus', '0', '--model-file', 'm.pt', '--in-file-list', 'l', '--in-lab-dir', 'lab', '--in-wav-dir', 'wav',
        '--out-ark-fn', 'a', '--out-seg-fn', 's']


def test_cli_takes_dither_device():
    assert predict.parse_args(BASE).dither == 'host'
    assert predict.parse_args(BASE + ['--dither', 'device']).dither == 'device'
    assert predict.parse_args(BASE + ['--dither', 'host', '--no-dither']).no_dither


def test_cli_refuses_dither_device_without_dither(capsys):
    with pytest.raises(SystemExit):
        predict.parse_args(BASE + ['--dither', 'device', '--no-dither'])
    assert '--no-dither' in capsys.readouterr().err


def _f(u, v, w):
    y = (u & np.uint32(0x80000000)) | (v & np.uint32(0x7fffffff))
    return w ^ (y >> np.uint32(1)) ^ np.where(y & np.uint32(1), np.uint32(0x9908b0df), np.uint32(0))


def _twist(old):
    """The kernel's schedule: three data-parallel phases (the last word goes with the third)."""
    new = np.empty_like(old)
    new[0:227] = _f(old[0:227], old[1:228], old[397:624])
    new[227:454] = _f(old[227:454], old[228:455], new[0:227])
    new[454:623] = _f(old[454:623], old[455:624], new[227:396])
    new[623] = _f(old[623:624], new[0:1], new[396:397])[0]
    return new


def _temper(y):
    y = y ^ (y >> np.uint32(11))
    y = y ^ ((y << np.uint32(7)) & np.uint32(0x9d2c5680))
    y = y ^ ((y << np.uint32(15)) & np.uint32(0xefc60000))
    return y ^ (y >> np.uint32(18))


@pytest.mark.parametrize('seed', [3, 0, 2 ** 32 - 1])
def test_phased_twist_is_numpys_stream(seed):
    twists = 3
    mt = fbank.mt19937_seed_state(seed)
    out = []
    for _ in range(twists):
        mt = _twist(mt)
        w = _temper(mt)
        a, b = (w[0::2] >> np.uint32(5)).astype(np.float64), (w[1::2] >> np.uint32(6)).astype(np.float64)
        out.append((a * 67108864.0 + b) / 9007199254740992.0)
    rs = np.random.RandomState(seed)
    assert np.array_equal(np.concatenate(out), rs.rand(twists * (N // 2)))
    assert np.array_equal(mt, rs.get_state()[1])


def test_dither_rounds_once():
    # 2 r - 1 is exact and 8 (2 r - 1) too, so x + 8 (2 r - 1) rounds only in the add: fused or not, the same bits
    r = np.random.RandomState(3).rand(4096)
    d = r * 2 - 1
    assert np.array_equal(((d + 1) / 2), r)
    x = np.random.default_rng(0).integers(-32768, 32768, 4096)
    assert np.array_equal(fbank.dither(x), x + 8 * d)
