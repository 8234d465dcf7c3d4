"""The resampling kernel (vbx_resample.hpp) against the referee of tests/audio_ref.py -- -m gpu.

The definition is integer arithmetic, so the device's samples must be the referee's as integers: no tolerance anywhere.
Shapes are the smallest at which the kernel can go wrong: every sample format and frame size, recordings at every byte offset
of a 16-byte chunk, lengths round the tile of 256 outputs, a table in LDS (L <= 3) and one read through L2."""
import os
import subprocess
import sys

import numpy as np
import pytest

import audio_ref as ar

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ['u8', 's16', 's24', 's32', 'f32']
# L / M / taps: 1 / 3 / 193 single phase | 2 / 1 / 65 upsampling | 160 / 441 / 177 every phase inside one tile |
# 320 / 441 / 89 L larger than a tile's phase span | 1 / 1 / 65 equal rates
PAIRS = [(48000, 16000), (8000, 16000), (44100, 16000), (11025, 8000), (16000, 16000)]


def device(recordings, fmt, C, pair, **kw):
    from vbx_amd import audio
    got = audio.to_mono16(recordings, fmt, C, *pair, device=0, **kw)
    assert len(got) == len(recordings) and all(y.dtype == np.int16 for y in got)
    return [[int(v) for v in y] for y in got]


def n_out(n, f):
    return -(-n * f['L'] // f['M'])


def frames_for(outputs, f):
    """The fewest frames that give at least ``outputs`` samples (exactly that many whenever L <= M)."""
    n = outputs * f['M'] // f['L']
    while n_out(n, f) < outputs:
        n += 1
    return n


def test_the_pairs_are_what_they_are_here_for():
    from vbx_amd import _capi, audio
    shape = {p: (audio.resample_filter(*p).L, audio.resample_filter(*p).M, audio.resample_filter(*p).taps) for p in PAIRS}
    assert [shape[p] for p in PAIRS] == [(1, 3, 193), (2, 1, 65), (160, 441, 177), (320, 441, 89), (1, 1, 65)]
    in_lds = [L * taps <= _capi.RESAMPLE_TABLE_LDS for L, _, taps in shape.values()]
    assert in_lds == [True, True, False, False, True] and _capi.RESAMPLE_TILE == 256
    assert shape[PAIRS[3]][0] > _capi.RESAMPLE_TILE > shape[PAIRS[2]][0]


@pytest.mark.parametrize('pair', PAIRS)
def test_every_format_and_channel_count(pair):
    k = 0
    for fmt in FORMATS:
        for C in (1, 2, 3):
            k += 1
            batch = [ar.random_bytes(31 * k + s, fmt, C, n, sigma=0.35) for s, n in enumerate((70 + 9 * k, 1, 41 + k))]
            refs = [ar.reference(b, fmt, C, *pair) for b in batch]
            assert max(abs(v) for v in refs[0]) > 1000
            assert device(batch, fmt, C, pair) == refs, (fmt, C)


@pytest.mark.parametrize('pair', PAIRS)
def test_lengths_round_the_tile_and_the_ends(pair):
    """No frame, one, two; the longest recording every output of which sees an end inside its window; and the lengths that
    give a tile less one, a tile, a tile and one, two tiles and three outputs (upsampling by two: the even count at or above)."""
    from vbx_amd import _capi
    f, tile = ar.filter_table(*pair), _capi.RESAMPLE_TILE
    sees_an_end = lambda n: all(m * f['M'] - f['P'] < 0 or m * f['M'] + f['P'] > (n - 1) * f['L'] for m in range(n_out(n, f)))
    edge = max(n for n in range(1, 4 * f['P'] // f['L'] + 8) if sees_an_end(n))
    assert edge >= f['P'] // f['L'] and not sees_an_end(edge + f['M'] // f['L'] + 1)
    lengths = [0, 1, 2, edge] + [frames_for(t, f) for t in (tile - 1, tile, tile + 1, 2 * tile + 3)]
    outs = [n_out(n, f) for n in lengths]
    assert outs[4:] == ([tile - 1, tile, tile + 1, 2 * tile + 3] if f['L'] <= f['M'] else [tile, tile, tile + 2, 2 * tile + 4])
    fmt, C = [('s16', 1), ('f32', 2), ('s24', 1), ('u8', 2), ('s32', 3)][PAIRS.index(pair)]
    batch = [ar.random_bytes(7 + i, fmt, C, n, sigma=0.3) for i, n in enumerate(lengths)]
    got = device(batch, fmt, C, pair)
    assert [len(y) for y in got] == outs
    for n, y, b in zip(lengths, got, batch):
        assert y == ar.reference(b, fmt, C, *pair), n
        assert device([b], fmt, C, pair) == [y], n


@pytest.mark.parametrize('fmt,C,pair,n', [('u8', 1, (8000, 16000), 48), ('s24', 3, (44100, 16000), 64), ('s16', 1, (48000, 16000), 24)])
def test_recordings_at_every_byte_offset_inside_the_batch(fmt, C, pair, n):
    """Frames of 1, 9 and 2 bytes: copies of one recording, a filler of one frame before each, start at every residue of 16
    (of 16 in steps of two for the 2-byte frames)."""
    fb = ar.WIDTH[fmt] * C
    assert n * fb % 16 == 0
    target = ar.random_bytes(3, fmt, C, n, sigma=0.4)
    fillers = [ar.random_bytes(50 + i, fmt, C, 1, sigma=0.4) for i in range(16)]
    batch, offsets, off = [], set(), 0
    for filler in fillers:
        batch += [filler, target]
        off += fb
        offsets.add(off % 16)
        off += n * fb
    assert offsets == set(range(0, 16, 2 if fb == 2 else 1))
    got = device(batch, fmt, C, pair)
    ref = ar.reference(target, fmt, C, *pair)
    assert max(abs(v) for v in ref) > 1000
    for i, filler in enumerate(fillers):
        assert got[2 * i + 1] == ref, i
        assert got[2 * i] == ar.reference(filler, fmt, C, *pair), i


@pytest.mark.parametrize('pair', [(44100, 16000), (48000, 16000), (8000, 16000)])
def test_a_recording_gives_the_same_bits_anywhere_in_any_batch(pair):
    """Alone, then first, in the middle and last; next to a recording of no frame; between a neighbour that ends at full scale
    and one that begins at full scale: nothing leaks across."""
    fmt, C = 's16', 2
    hi, lo = ar.encode([32767] * (2 * 90), fmt), ar.encode([-32768] * (2 * 90), fmt)
    recs = [ar.random_bytes(1, fmt, C, 150, sigma=0.3), b'', hi, ar.random_bytes(2, fmt, C, 333, sigma=0.3), lo]
    refs = [ar.reference(b, fmt, C, *pair) for b in recs]
    alone = [device([b], fmt, C, pair)[0] for b in recs]
    assert alone == refs and refs[1] == [] and 32767 in refs[2] and -32768 in refs[4]
    places = {i: set() for i in range(len(recs))}
    for shift in range(len(recs)):
        order = [(i + shift) % len(recs) for i in range(len(recs))]
        got = device([recs[i] for i in order], fmt, C, pair)
        for pos, i in enumerate(order):
            places[i].add('first' if pos == 0 else 'last' if pos == len(recs) - 1 else 'middle')
            assert got[pos] == alone[i], (shift, pos)
    assert all(p == {'first', 'middle', 'last'} for p in places.values())
    # the random recording with the full-scale ones on both sides, in both orders
    assert device([hi, recs[3], lo], fmt, C, pair)[1] == refs[3] == device([lo, recs[3], hi], fmt, C, pair)[1]


@pytest.mark.parametrize('pair', [(48000, 16000), (8000, 16000), (44100, 16000)])
def test_saturation_and_impulse(pair):
    """The two cases of tests/test_audio_host.py on the device: a full-scale square wave whose overshoot passes the int16 range
    (mono, and stereo where |X| is at its largest), and an impulse that reads the table back."""
    from vbx_amd import audio
    f = ar.filter_table(*pair)
    x = [32767 if (j // 50) % 2 == 0 else -32768 for j in range(600)]
    raw = ar.resample(ar.decode(ar.encode(x, 's16'), 's16', 1), 1, f, clamp=False)
    assert max(raw) > 32767 + 1000 and min(raw) < -32768 - 1000
    want = [min(max(v, -32768), 32767) for v in raw]
    assert device([ar.encode(x, 's16')], 's16', 1, pair) == [want]
    assert device([ar.encode([v for a in x for v in (a, a)], 's16')], 's16', 2, pair) == [want]
    full = ar.encode([v for a in x for v in [1.0 if a > 0 else -1.0] * 8], 'f32')              # eight channels at the f32 clamps
    assert device([full], 'f32', 8, pair) == [ar.reference(full, 'f32', 8, *pair)]
    hq = [int(v) for v in audio.resample_filter(*pair).hq]
    L, M, P = f['L'], f['M'], f['P']
    n, j0, A = 2 * P // L + 50, P // L + 13, 30011
    imp = [0] * n
    imp[j0] = A
    want = []
    for m in range(n_out(n, f)):
        i = P + m * M - j0 * L
        want.append(((2 * A * hq[i] if 0 <= i <= 2 * P else 0) + (1 << 24)) >> 25)
    assert device([ar.encode(imp, 's16')], 's16', 1, pair) == [want] and max(want) > 0.3 * A * min(L / M, 1.0)


def test_f32_special_values_and_s32_floor_on_the_device():
    q = 2.0 ** -23
    values = [float('nan'), float('inf'), float('-inf'), 1.5, -1.5, 1.0, -1.0, 0.5, 2.5 * q, 3.5 * q, -2.5 * q, 0.5 * q, 1.5 * q, -0.0, 1e-42, 3e38]
    data = ar.encode(values, 'f32')
    assert device([data], 'f32', 1, (16000, 16000)) == [ar.reference(data, 'f32', 1, 16000, 16000)]
    assert device([data], 'f32', 1, (16000, 16000))[0][:8] == [0, 32767, -32768, 32767, -32768, 32767, -32768, 16384]
    # 256 channels' worth of rounding would be needed to see one quantum: sum 8 channels of 2.5 q (half-even: 2 each) and of 3.5 q (4 each)
    eight = ar.encode([2.5 * q] * 8 + [3.5 * q] * 8 + [float('nan')] * 8, 'f32')
    assert device([eight], 'f32', 8, (8000, 8000)) == [ar.reference(eight, 'f32', 8, 8000, 8000)]
    s32 = ar.encode([-129 * 256 + 1, -1, -255, -256, -257, 255, 256 * 256 * 77 + 255, -(1 << 31), (1 << 31) - 1], 's32')
    assert device([s32], 's32', 1, (16000, 16000)) == [[-1, 0, 0, 0, 0, 0, 77, -32768, 32767]]


def test_times_and_refusals():
    from vbx_amd import _capi, audio
    data = ar.random_bytes(1, 's16', 2, 500)
    times = {}
    y = audio.to_mono16([data], 's16', 2, 48000, 16000, device=0, times=times)[0]
    assert np.array_equal(y, audio.to_mono16([data], 's16', 2, 48000, 16000)[0])
    assert set(times) == {'upload', 'kernels'} and times['upload'] > 0 and times['kernels'] > 0
    assert audio.to_mono16([], 's16', 2, 48000, 16000, device=0) == []
    ctx = _capi.default_context(0)
    f = audio.resample_filter(48000, 16000)
    raw = np.frombuffer(data, dtype=np.uint8)
    ok = dict(rec=[[0, 500]], fmt=1, channels=2, L=f.L, M=f.M, table=f.phase_table())
    for kw, msg in ((dict(rec=[[0, 501]]), 'outside'), (dict(rec=[[-4, 10]]), 'outside'), (dict(rec=[[4, 500]]), 'outside'), (dict(fmt=5), 'format = 5'),
                    (dict(channels=9), 'channels = 9'), (dict(M=4), 'taps = 193'), (dict(L=0, table=np.zeros((0, 193), np.int32)), 'L = 0')):
        a = dict(ok, **kw)
        with pytest.raises(_capi.VbxError, match=msg):
            _capi.resample_pcm(ctx, raw, np.array(a['rec'], dtype=np.int64), a['fmt'], a['channels'], a['L'], a['M'], a['table'])
    with pytest.raises(_capi.VbxError, match='at most 8192 are staged'):          # 240 kHz -> 8 kHz: M / L = 30
        audio.to_mono16([data], 's16', 2, 240000, 8000, device=0)


def test_diarize_with_the_option_equals_diarize_on_the_converted_files(tmp_path):
    """Generated recordings rendered as 48 kHz stereo s16, in fresh child processes: ``diarize --resample-to 16000`` writes the
    RTTM bytes that plain ``diarize`` writes on the files ``python -m vbx_amd.audio`` made of them; without the option the
    stereo files are refused with the message they always were."""
    import diarize_util as du
    recs = {'recA': du.synth_recording(1, 48000, 12, 2), 'recB': du.synth_recording(3, 48000, 9, 2)}
    os.makedirs(tmp_path / 'wav')
    os.makedirs(tmp_path / 'lab')
    for fn, (x, lab, _) in recs.items():
        stereo = np.stack([x, x // 2 + 3], axis=1).astype('<i2').tobytes()
        (tmp_path / 'wav' / f'{fn}.wav').write_bytes(ar.wav_bytes(stereo, 's16', 2, 48000))
        (tmp_path / 'lab' / f'{fn}.lab').write_text(lab)
    (tmp_path / 'list').write_text(''.join(f'{fn}\n' for fn in recs))
    p = dict(du.write_models(tmp_path), ckpt=du.write_checkpoint(tmp_path))
    env = dict(os.environ, PYTHONPATH=REPO)
    run = lambda argv: subprocess.run([sys.executable, '-m'] + argv, env=env, cwd=REPO, capture_output=True, text=True, timeout=300)
    res = run(['vbx_amd.audio', '--device', '0', '--rate', '16000', '--in-file-list', str(tmp_path / 'list'), '--in-wav-dir', str(tmp_path / 'wav'),
               '--out-wav-dir', str(tmp_path / 'mono')])
    assert res.returncode == 0, res.stderr[-3000:]

    def diarize(wav, out, *more):
        return run(['vbx_amd.diarize', '--gpus', '0', '--checkpoint', p['ckpt'], '--in-file-list', str(tmp_path / 'list'), '--in-lab-dir',
                    str(tmp_path / 'lab'), '--in-wav-dir', str(tmp_path / wav), '--batch-size', '16', '--out-rttm-dir', str(tmp_path / out),
                    '--xvec-transform', p['transform'], '--plda-file', p['plda'], '--init', 'AHC+VB', '--threshold', '0.0', '--lda-dim', '128',
                    '--Fa', '4.0', '--Fb', '1.0', '--loopP', '0.99', *more])
    res = diarize('mono', 'rttm_mono')
    assert res.returncode == 0, res.stderr[-3000:]
    res = diarize('wav', 'rttm_direct', '--resample-to', '16000')
    assert res.returncode == 0, res.stderr[-3000:]
    direct, mono = du.rttm_dir(str(tmp_path / 'rttm_direct')), du.rttm_dir(str(tmp_path / 'rttm_mono'))
    assert sorted(direct) == ['recA.rttm', 'recB.rttm'] and direct == mono
    assert all(du.rttm_speakers_and_lines(v)[1] >= 1 for v in direct.values())
    res = diarize('wav', 'rttm_refused')
    assert res.returncode != 0 and '2 channel(s) of 16-bit samples; only mono 16-bit PCM is supported' in res.stderr
    assert du.rttm_dir(str(tmp_path / 'rttm_refused')) == {}
