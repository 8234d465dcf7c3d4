"""vbx_amd.audio on the host: the filter table, the numpy path against the referee of tests/audio_ref.py
bit for bit, expectations derived by hand (which check the referee too), scipy's resample_poly as an independent
implementation, the WAV parser, the command line and the ABI."""
import math
import os
import re
import warnings

import numpy as np
import pytest

import audio_ref as ar

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ['u8', 's16', 's24', 's32', 'f32']
RESAMPLING = [p for p in ar.PAIRS if p[0] != p[1]]


def host(data, fmt, C, sr_in, sr_out):
    from vbx_amd import audio
    y = audio.to_mono16([data], fmt, C, sr_in, sr_out)[0]
    assert y.dtype == np.int16
    return [int(v) for v in y]


def s16(values):
    return ar.encode(values, 's16')


# ---- the filter table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', ar.PAIRS)
def test_every_phase_sums_to_one_and_the_table_is_the_rounded_prototype(pair):
    from vbx_amd import audio
    f = audio.resample_filter(*pair)
    g = math.gcd(*pair)
    assert (f.L, f.M, f.P) == (pair[1] // g, pair[0] // g, 32 * max(pair) // g) and f.hq.dtype == np.int64 and f.hq.shape == (2 * f.P + 1,)
    ref = ar.filter_table(*pair)
    assert [int(v) for v in f.hq] == ref['hq']
    off = np.abs(f.hq - ref['h'] * 2.0 ** 24) > 0.5
    for p in range(f.L):
        assert int(f.hq[p::f.L].sum()) == 1 << 24
        assert int(np.abs(f.hq[p::f.L]).sum()) < 1 << 26
        assert int(off[p::f.L].sum()) <= 1
    table = f.phase_table()
    assert table.dtype == np.int32 and table.shape == (f.L, f.taps) and f.taps == 2 * f.P // f.L + 1
    for p in range(0, f.L, max(f.L // 7, 1)):
        row = [int(v) for v in f.hq[p::f.L]]
        assert [int(v) for v in table[p]] == row + [0] * (f.taps - len(row))


def test_the_equal_rate_table_is_the_unit_impulse():
    from vbx_amd import audio
    for sr in (8000, 16000):
        f = audio.resample_filter(sr, sr)
        assert (f.L, f.M, f.P) == (1, 1, 32)
        assert int(f.hq[f.P]) == 1 << 24 and int(np.abs(f.hq).sum()) == 1 << 24


@pytest.mark.parametrize('pair', RESAMPLING)
def test_ripple_and_stop_band_of_the_integer_table(pair):
    """From the integer table by an FFT of 2^20 points at the L-times upsampled rate, where the lower Nyquist frequency is
    1 / (2 R) of the rate and the gain at 0 Hz is L (every phase sums to one)."""
    from vbx_amd import audio
    f = audio.resample_filter(*pair)
    N = 1 << 20
    gain = np.abs(np.fft.rfft(f.hq / 2.0 ** 24, N)) / f.L
    x = np.arange(N // 2 + 1) / N * 2 * max(f.L, f.M)          # frequency in units of the lower Nyquist frequency
    ripple = float(np.abs(20 * np.log10(gain[x <= 0.9])).max())
    stop = float(20 * np.log10(gain[x >= 1.1].max()))
    print(f'{pair}: ripple {ripple:.5f} dB, stop band {stop:.1f} dB, taps {f.taps}')
    assert ripple <= 0.001 and stop <= -95.0


def test_rate_pairs_refused():
    from vbx_amd import audio
    with pytest.raises(ValueError, match=r'16000 / 44101'):
        audio.resample_filter(44101, 16000)
    with pytest.raises(ValueError, match='Only 8kHz and 16kHz'):
        audio.resample_filter(48000, 44100)
    for sr in (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000):
        for out in (8000, 16000):
            audio.resample_filter(sr, out)


# ---- the numpy path is the referee -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', ar.PAIRS)
def test_numpy_path_equals_the_referee(pair):
    k = 0
    for fmt in FORMATS:
        for C in (1, 2, 3):
            k += 1
            n = 90 + 17 * k
            data = ar.random_bytes(100 * k + ar.PAIRS.index(pair), fmt, C, n, sigma=0.35)
            ref = ar.reference(data, fmt, C, *pair)
            assert len(ref) == -(-n * pair[1] // pair[0]) and max(abs(v) for v in ref) > 1000
            assert host(data, fmt, C, *pair) == ref, (fmt, C, n)


@pytest.mark.parametrize('pair', ar.PAIRS)
def test_no_frame_and_one_frame(pair):
    for fmt in FORMATS:
        assert host(b'', fmt, 2, *pair) == [] == ar.reference(b'', fmt, 2, *pair)
        one = ar.encode([0.75, -0.25] if fmt == 'f32' else [200, 17] if fmt == 'u8' else [ar.FULL_SCALE[fmt][1] // 2, -5], fmt)
        ref = ar.reference(one, fmt, 2, *pair)
        assert len(ref) == -(-pair[1] // pair[0]) and host(one, fmt, 2, *pair) == ref


def test_recordings_of_a_batch_and_trailing_bytes():
    from vbx_amd import audio
    a, b = ar.random_bytes(1, 's24', 2, 120), ar.random_bytes(2, 's24', 2, 45)
    got = audio.to_mono16([a, b'', np.frombuffer(b + b'\x01\x02', dtype=np.uint8)], 's24', 2, 44100, 16000)       # (a broken last frame is left out)
    assert [[int(v) for v in y] for y in got] == [ar.reference(a, 's24', 2, 44100, 16000), [], ar.reference(b, 's24', 2, 44100, 16000)]
    with pytest.raises(ValueError, match='format'):
        audio.to_mono16([a], 's20', 2, 44100, 16000)
    with pytest.raises(ValueError, match='channels'):
        audio.to_mono16([a], 's24', 9, 44100, 16000)


# ---- expectations derived by hand ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', ar.PAIRS)
def test_a_constant_comes_out_as_itself_away_from_the_ends(pair):
    """Every phase sums to 2^24: acc = c 2^8 2^24 wherever the whole window lies inside, and floor(c + 1/2) = c."""
    f = ar.filter_table(*pair)
    edge = -(-f['P'] // f['M']) + 1
    n = (2 * f['P'] // f['L'] + 1) + 40 * f['M'] // f['L'] + 40
    for c in (-12345, 1, 32767):
        y = host(s16([c] * n), 's16', 1, *pair)
        assert y == ar.reference(s16([c] * n), 's16', 1, *pair) and len(y) > 2 * edge + 5
        assert y[edge:len(y) - edge] == [c] * (len(y) - 2 * edge)


@pytest.mark.parametrize('pair', ar.PAIRS + [(11025, 8000)])
def test_an_impulse_reads_the_table_back(pair):
    """Height A (an s16 sample: q = A 2^8) at frame j0: y[m] = floor((2 A hq[P + m M - j0 L] + 2^24) / 2^25)."""
    from vbx_amd import audio
    f = audio.resample_filter(*pair)
    hq = [int(v) for v in f.hq]
    n, j0, A = 2 * f.P // f.L + 50, f.P // f.L + 13, 30011
    x = [0] * n
    x[j0] = A
    y = host(s16(x), 's16', 1, *pair)
    want = []
    for m in range(-(-n * f.L // f.M)):
        i = f.P + m * f.M - j0 * f.L
        want.append(((2 * A * hq[i] if 0 <= i <= 2 * f.P else 0) + (1 << 24)) >> 25)
    assert y == want and max(want) > 0.3 * A * min(f.L / f.M, 1.0)
    assert y == ar.reference(s16(x), 's16', 1, *pair)


@pytest.mark.parametrize('pair', [(48000, 16000), (44100, 8000), (8000, 16000)])
def test_equal_channels_are_mono_and_opposite_channels_are_zero(pair):
    rng = np.random.default_rng(5)
    x = [int(v) for v in rng.integers(-32767, 32768, 300)]
    mono = host(s16(x), 's16', 1, *pair)
    assert host(s16([v for a in x for v in (a, a)]), 's16', 2, *pair) == mono and max(mono) > 5000
    assert host(s16([v for a in x for v in (a, a, a)]), 's16', 3, *pair) == mono
    assert host(s16([v for a in x for v in (a, -a)]), 's16', 2, *pair) == [0] * len(mono)


@pytest.mark.parametrize('pair', [(48000, 16000), (8000, 16000), (44100, 16000)])
def test_full_scale_square_wave_saturates_and_never_wraps(pair):
    """Full scale alternating every 50 frames: the filter's overshoot at every edge passes the int16 range."""
    f = ar.filter_table(*pair)
    x = [32767 if (j // 50) % 2 == 0 else -32768 for j in range(600)]
    raw = ar.resample(ar.decode(s16(x), 's16', 1), 1, f, clamp=False)
    assert max(raw) > 32767 + 1000 and min(raw) < -32768 - 1000
    y = host(s16(x), 's16', 1, *pair)
    assert y == [min(max(v, -32768), 32767) for v in raw] == ar.reference(s16(x), 's16', 1, *pair)
    assert y.count(32767) > 10 and y.count(-32768) > 10
    stereo = [v for a in x for v in (a, a)]                                   # (|X| at its largest: 2^24 a channel)
    assert host(s16(stereo), 's16', 2, *pair) == y


def test_s32_shifts_with_floor():
    """v = -129 * 256 + 1: floor gives q = -129 and y = floor(-129 / 256 + 1 / 2) = -1; truncation would give q = -128, y = 0."""
    from vbx_amd import audio
    values = [-129 * 256 + 1, -1, -255, -256, -257, 255, 256 * 256 * 77 + 255, -(1 << 31), (1 << 31) - 1]
    data = ar.encode(values, 's32')
    want = [-129, -1, -1, -1, -2, 0, 256 * 77, -(1 << 23), (1 << 23) - 1]
    assert [int(v) for v in audio.decode(data, 's32', 1)] == want == ar.decode(data, 's32', 1)
    assert host(data, 's32', 1, 16000, 16000) == [-1, 0, 0, 0, 0, 0, 77, -32768, 32767]


def test_f32_maps_as_defined():
    from vbx_amd import audio
    q = 2.0 ** -23
    values = [float('nan'), float('inf'), float('-inf'), 1.5, -1.5, 1.0, -1.0, 0.5, 2.5 * q, 3.5 * q, -2.5 * q, 0.5 * q, 1.5 * q, -0.0, 1e-42, 3e38]
    data = ar.encode(values, 'f32')
    top, bot = (1 << 23) - 1, -(1 << 23)
    want = [0, top, bot, top, bot, top, bot, 1 << 22, 2, 4, -2, 0, 2, 0, 0, top]
    assert [int(v) for v in audio.decode(data, 'f32', 1)] == want == ar.decode(data, 'f32', 1)
    assert host(data, 'f32', 1, 8000, 8000)[:8] == [0, 32767, -32768, 32767, -32768, 32767, -32768, 16384]
    assert [int(v) for v in audio.decode(ar.encode([0, 128, 255], 'u8') + ar.encode([-2, 3], 's16'), 'u8', 1)][:3] == [-128 << 16, 0, 127 << 16]
    assert [int(v) for v in audio.decode(ar.encode([-2, 3, -(1 << 23)], 's24'), 's24', 3)] == [1 - (1 << 23)]


# ---- against an independent implementation -----------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', RESAMPLING)
def test_scipy_resample_poly_rounds_to_the_referee(pair):
    signal = pytest.importorskip('scipy.signal')
    f = ar.filter_table(*pair)
    x = np.clip(np.rint(np.random.default_rng(0).standard_normal(3000) * 6000), -32768, 32767).astype(np.int64)
    X = [int(v) << 8 for v in x]
    ref = ar.resample(X, 1, f)
    z = signal.resample_poly(np.array(X, dtype=np.float64) / 256, f['L'], f['M'], window=np.array(f['hq'], dtype=np.float64) / 2.0 ** 24 / f['L'],
                             padtype='constant')
    frac = z + 0.5 - np.floor(z + 0.5)
    margin = float(np.minimum(frac, 1 - frac).min())
    print(f'{pair}: smallest distance from a rounding tie {margin:.2e}')
    assert margin >= 1e-6
    assert len(z) == len(ref) and [int(v) for v in np.floor(z + 0.5)] == ref


# ---- the parser ------------------------------------------------------------------------------------------------------------
def write(tmp_path, name, blob):
    path = str(tmp_path / name)
    with open(path, 'wb') as fh:
        fh.write(blob)
    return path


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('extensible', [False, True])
def test_every_accepted_format_is_read(tmp_path, fmt, extensible):
    from vbx_amd import audio
    data = ar.random_bytes(3, fmt, 3, 41)                      # (41 frames of 3 u8 samples: an odd data chunk with its pad byte)
    before = [(b'LIST', b'INFOISFT\x05\0\0\0abcd\0\0'), (b'odd ', b'\x01\x02\x03')] if extensible or fmt == 's24' else []
    path = write(tmp_path, 'a.wav', ar.wav_bytes(data, fmt, 3, 44100, extensible=extensible, before=before))
    got, name, ch, sr, frames = audio.read_audio(path)
    assert (got.tobytes(), name, ch, sr, frames) == (data, fmt, 3, 44100, 41) and got.dtype == np.uint8
    y, rate = audio.load_mono16(path, 8000)
    assert rate == 8000 and [int(v) for v in y] == ar.reference(data, fmt, 3, 44100, 8000)


def test_refusals_name_what_was_found(tmp_path):
    from vbx_amd import audio
    d = ar.random_bytes(1, 's16', 1, 10)
    for blob, msg in ((ar.wav_bytes(d, 's16', 1, 8000, tag=2), r'0x0002 \(ADPCM\)'), (ar.wav_bytes(d, 's16', 1, 8000, tag=7), r'0x0007 \(mu-law\)'),
                      (ar.wav_bytes(d, 's16', 1, 8000, tag=0x55), r'0x0055'), (ar.wav_bytes(d, 'f32', 1, 8000, bits=64, align=8), '64-bit IEEE float'),
                      (ar.wav_bytes(d, 's16', 1, 8000, bits=12), '12-bit PCM'), (ar.wav_bytes(d * 9, 's16', 9, 8000), '9 channels'),
                      (ar.wav_bytes(d, 's24', 1, 8000, align=4), 'frames of 4 bytes'), (ar.wav_bytes(d, 's16', 1, 8000, extensible=True, tag=6), 'sub-format 0600'),
                      (b'RIFX' + ar.wav_bytes(d, 's16', 1, 8000)[4:], 'not a RIFF/WAVE file'), (ar.wav_bytes(d, 's16', 1, 8000)[:36], 'no data chunk'),
                      (b'RIFF\x04\0\0\0WAVE', 'no fmt chunk')):
        with pytest.raises(ValueError, match=msg):
            audio.read_audio(write(tmp_path, 'bad.wav', blob))


def test_a_data_chunk_is_cut_to_whole_frames_in_the_file(tmp_path):
    from vbx_amd import audio
    data = ar.random_bytes(4, 's24', 2, 30)
    for blob, frames in ((ar.wav_bytes(data, 's24', 2, 48000, data_size=1 << 20), 30), (ar.wav_bytes(data[:-2], 's24', 2, 48000, data_size=len(data)), 29),
                         (ar.wav_bytes(data[:-1], 's24', 2, 48000), 29), (ar.wav_bytes(data, 's24', 2, 48000, data_size=0xFFFFFFFF), 30)):
        with pytest.warns(UserWarning, match=f'cut to {frames} whole frames'):
            got, _, _, _, n = audio.read_audio(write(tmp_path, 'cut.wav', blob))
        assert n == frames and got.tobytes() == data[:6 * frames]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert audio.read_audio(write(tmp_path, 'whole.wav', ar.wav_bytes(data, 's24', 2, 48000)))[4] == 30


@pytest.mark.parametrize('sr', [8000, 16000])
def test_a_mono_s16_file_at_the_target_rate_is_read_wavs_samples(tmp_path, sr):
    from vbx_amd import audio, fbank
    x = np.random.default_rng(sr).integers(-32768, 32768, 777).astype(np.int16)
    x[:2] = (-32768, 32767)
    path = str(tmp_path / 'm.wav')
    fbank.write_wav(path, x, sr)
    y, rate = audio.load_mono16(path, sr)
    want, want_sr = fbank.read_wav(path, raw=True)
    assert rate == want_sr == sr and y.dtype == want.dtype and np.array_equal(y, want) and np.array_equal(y, x)


# ---- the commands ------------------------------------------------------------------------------------------------------------
def corpus(tmp_path):
    """Three files of three kinds; -> {name: (data, fmt, C, sr)}"""
    files = {'studio': (ar.random_bytes(7, 's24', 2, 4800), 's24', 2, 48000), 'cd': (ar.random_bytes(8, 'f32', 1, 2000), 'f32', 1, 44100),
             'cd2': (ar.random_bytes(9, 'f32', 1, 500), 'f32', 1, 44100), 'phone': (ar.random_bytes(10, 's16', 1, 900), 's16', 1, 8000)}
    os.makedirs(tmp_path / 'wav')
    for name, (data, fmt, C, sr) in files.items():
        write(tmp_path / 'wav', f'{name}.wav', ar.wav_bytes(data, fmt, C, sr, extensible=fmt == 's24'))
    (tmp_path / 'list').write_text(''.join(f'{name}\n' for name in files))
    return files


@pytest.mark.parametrize('rate', [16000, 8000])
def test_command_writes_files_that_read_wav_reads(tmp_path, rate):
    from vbx_amd import audio, fbank
    files = corpus(tmp_path)
    assert audio.main(['--in-file-list', str(tmp_path / 'list'), '--in-wav-dir', str(tmp_path / 'wav'), '--out-wav-dir', str(tmp_path / 'out'),
                       '--rate', str(rate)]) == 0
    assert sorted(os.listdir(tmp_path / 'out')) == sorted(f'{name}.wav' for name in files)
    for name, (data, fmt, C, sr) in files.items():
        y, got_rate = fbank.read_wav(str(tmp_path / 'out' / f'{name}.wav'))
        assert got_rate == rate and [int(v) for v in y] == ar.reference(data, fmt, C, sr, rate)


def test_command_refuses_what_the_parser_refuses(tmp_path, capsys):
    from vbx_amd import audio
    os.makedirs(tmp_path / 'wav')
    write(tmp_path / 'wav', 'law.wav', ar.wav_bytes(b'\0' * 8, 'u8', 1, 8000, tag=7))
    (tmp_path / 'list').write_text('law\n')
    with pytest.raises(SystemExit):
        audio.main(['--in-file-list', str(tmp_path / 'list'), '--in-wav-dir', str(tmp_path / 'wav'), '--out-wav-dir', str(tmp_path / 'out')])
    assert 'mu-law' in capsys.readouterr().err and not os.path.exists(tmp_path / 'out')


def test_vad_takes_any_wav_with_the_option_and_refuses_it_without(tmp_path, capsys):
    """``vad --resample-to`` gives the .lab files that plain ``vad`` gives on the converted files; without the option the
    file is refused as before."""
    from vbx_amd import audio, vad
    rng = np.random.default_rng(11)
    level = np.repeat([5.0, 4000.0, 5.0, 6000.0, 5.0], 48000 // 2)
    x = np.clip(np.rint(rng.standard_normal(level.size) * level), -32768, 32767).astype(np.int64)
    stereo = ar.encode([int(v) for a in x for v in (a, a // 2)], 's16')
    os.makedirs(tmp_path / 'wav')
    write(tmp_path / 'wav', 'talk.wav', ar.wav_bytes(stereo, 's16', 2, 48000))
    (tmp_path / 'list').write_text('talk\n')
    common = ['--in-file-list', str(tmp_path / 'list'), '--min-speech', '5', '--min-silence', '5']
    assert vad.main(common + ['--in-wav-dir', str(tmp_path / 'wav'), '--out-lab-dir', str(tmp_path / 'lab_a'), '--resample-to', '16000']) == 0
    assert audio.main(['--in-file-list', str(tmp_path / 'list'), '--in-wav-dir', str(tmp_path / 'wav'), '--out-wav-dir', str(tmp_path / 'mono')]) == 0
    assert vad.main(common + ['--in-wav-dir', str(tmp_path / 'mono'), '--out-lab-dir', str(tmp_path / 'lab_b')]) == 0
    text = (tmp_path / 'lab_a' / 'talk.lab').read_text()
    assert text == (tmp_path / 'lab_b' / 'talk.lab').read_text() and text.count('\n') == 2
    with pytest.raises(SystemExit):
        vad.main(common + ['--in-wav-dir', str(tmp_path / 'wav'), '--out-lab-dir', str(tmp_path / 'lab_c')])
    assert 'only mono 16-bit PCM is supported' in capsys.readouterr().err


def test_predict_and_diarize_have_the_option_and_default_to_none():
    from vbx_amd import diarize, predict
    base = ['--gpus', '0', '--checkpoint', 'c', '--in-file-list', 'l', '--in-lab-dir', 'lab', '--in-wav-dir', 'wav']
    pre = base + ['--out-ark-fn', 'a', '--out-seg-fn', 's']
    dia = base + ['--init', 'AHC', '--out-rttm-dir', 'r', '--xvec-transform', 't', '--plda-file', 'p', '--threshold', '0', '--lda-dim', '128', '--Fa', '1',
                  '--Fb', '1', '--loopP', '0.5']
    for mod, argv in ((predict, pre), (diarize, dia)):
        assert mod.parse_args(argv).resample_to is None
        assert mod.parse_args(argv + ['--resample-to', '8000']).resample_to == 8000
        with pytest.raises(SystemExit):
            mod.parse_args(argv + ['--resample-to', '44100'])


def test_abi_gains_the_symbol_and_keeps_its_version():
    from vbx_amd import _capi, build
    header = open(os.path.join(REPO, 'include', 'vbx_hip.h')).read()
    assert re.search(r'\bint vbx_resample_pcm\s*\(', header) and 'vbx_resample_pcm' in _capi.ABI_SYMBOLS
    assert re.search(r'#define VBX_ABI_VERSION 7\b', header)
    assert 'vbx_resample.hpp' in build.HEADERS and 'vbx_resample.hpp' not in build.ITERATION_SOURCES
    assert '#include "vbx_resample.hpp"' in open(os.path.join(build.CSRC, 'vbx_capi.hip')).read()
