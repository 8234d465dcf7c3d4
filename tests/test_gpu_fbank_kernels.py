"""The filterbank front end's kernels one by one (vbx_fbank.hpp: fbank_frame_kernel, fbank_cmn_kernel, fbank_gather_kernel,
fbank_gather_ragged_kernel) and the run tables of vbx_host_fbank.hpp, on the cases, the reference and the comparison
functions of tests/fbank_ref.py -- the ones tests/test_fbank_ref_host.py shows to see a mirror, a hop, a fill, a window or a
transpose that is off by one.

Every case of a rate is a slice of one 9.5 s signal; a rate's whole table (the mirror edges, 2 .. 470 frames at the smallest
and the largest sample count each, a loud tone, digital silence; one case twice, in a shuffled order) is ONE run of 4 896
frames, repeated for each of the seven (lc, rc) settings.

Measured on an MI355X (the tests print the figures; -s shows them):
    largest |log-Mel - ref_logmel|             5.805e-8 at 16 kHz, 5.907e-8 at 8 kHz; the tolerance, fbank_ref.LOGMEL_TOL, is
                                               four times the larger one: 2.363e-7 (the project's bound was 1e-6)
    CMN outputs that are not the bits of       74 of 2 193 408 at 16 kHz (3.4e-5), 66 of 2 193 408 at 8 kHz (3.0e-5); the
    float32(ref_cmn(device log-Mel))           cap is 1 %.  9 and 6 of them are a float32 neighbour of the reference; the
                                               other 65 and 60 are all at (lc, rc) = (0, 0), see below
    largest |feature - reference|              9.54e-7 at both rates (tolerance 4e-6)

The CMN check leaves one thing to fbank_ref.cmn_slack, and says why there: an output within 1e-12 of the float64 reference
is not asked to be one of the reference's float32 neighbours.  At (lc, rc) = (0, 0) the reference is exactly 0 and the
kernel's slid window sum is x[t-1] + (x[t] - x[t-1]), which now and then is not x[t] to the last bit: those 65 and 60
outputs are at most 1.8e-15.  As a count of float32 steps from 0 that is astronomical, as a feature it is 0.  At every other
setting every output is the reference's float32 value or a neighbour of it, with no slack at all.
"""
import functools

import numpy as np
import pytest

import fbank_ref as R
from vbx_amd import _capi, fbank

pytestmark = pytest.mark.gpu

DEFAULT = (fbank.CMN_LC, fbank.CMN_RC)
TWICE = 'N65max'                                  # the case the table holds twice


def _new_device(sr):
    g = fbank.geometry(sr)
    return _capi.FbankDevice(fbank.front_end(sr).ctx, g['winlen'], g['shift'], g['nfft'], fbank.povey_window(g['winlen']),
                             fbank.mel_matrix(sr), fbank.PREEMPH)


@functools.lru_cache(maxsize=None)
def _device(sr):
    return _new_device(sr)


@functools.lru_cache(maxsize=None)
def _table(sr):
    """[(case, first sample, samples, first row)] of the rate's one run: every case in a seeded shuffle, TWICE twice."""
    cases = list(R.cases(sr))
    cases.append(next(c for c in cases if c[0] == TWICE))
    order = list(np.random.default_rng(31 + sr).permutation(len(cases)))
    # the gathers at rows 0 and rows - len must not look at rows of zeros (the silence, and every segment of one frame,
    # whose mean is the frame): long segments go to both ends, the silence to the middle
    for name, to in (('N364min', 0), ('N470min', len(order) - 1), ('silence', len(order) // 2)):
        at = order.index(next(k for k, c in enumerate(cases) if c[0] == name))
        order[at], order[to] = order[to], order[at]
    out, row = [], 0
    for k in order:
        name, a, n = cases[k]
        out.append((name, a, n, row))
        row += fbank.n_frames(n, sr)
    return tuple(out), row


def _run(dev, sr, table, lc, rc):
    rows = dev.run(R.recording(sr), np.array([(a, n) for _, a, n, _ in table], dtype=np.int64), lc, rc)
    return rows


@functools.lru_cache(maxsize=None)
def _big(sr, setting):
    """(log-Mel rows, feature rows) of the rate's one run at one (lc, rc), copied out once and read-only."""
    table, rows = _table(sr)
    dev = _device(sr)
    assert _run(dev, sr, table, *setting) == rows == dev.rows
    lm, fea = dev.get('logmel', 0, rows), dev.get('fea', 0, rows)
    assert lm.dtype == np.float64 and fea.dtype == np.float32 and lm.shape == fea.shape == (rows, 64)
    lm.setflags(write=False)
    fea.setflags(write=False)
    return lm, fea


def _rows_of(sr, arr):
    """[(case, its rows of arr)] in table order."""
    return [(name, arr[row:row + fbank.n_frames(n, sr)]) for name, _, n, row in _table(sr)[0]]


# ---- the frame kernel alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('sr', R.RATES)
def test_logmel_rows_against_the_reference(sr):
    ref = R.reference(sr)
    lm = _big(sr, DEFAULT)[0]
    worst, bad = 0.0, []
    for name, got in _rows_of(sr, lm):
        assert got.shape == ref[name][0].shape, name
        err = float(np.abs(got - ref[name][0]).max())
        worst = max(worst, err)
        if R.logmel_excess(got, ref[name][0]) > 1.0:
            bad.append((name, err))
    print(f'{sr} Hz: largest |log-Mel - reference| = {worst:.3e} (tolerance {R.LOGMEL_TOL:.3e})')
    assert not bad, bad
    silence = dict(_rows_of(sr, lm))['silence']
    assert silence.shape == (40, 64) and not silence.any() and not np.signbit(silence).any()
    for setting in R.CMN_SETTINGS:                                 # (the frame kernel does not know the window)
        assert R.same_bits(_big(sr, setting)[0], lm), setting


# ---- the CMN kernel alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sr', R.RATES)
def test_cmn_of_the_device_logmel_rows(sr):
    differ = total = 0
    bad = []
    for setting in R.CMN_SETTINGS:
        lm, fea = _big(sr, setting)
        for (name, x), (_, got) in zip(_rows_of(sr, lm), _rows_of(sr, fea)):
            steps, d, _, n = R.cmn_steps(got, R.ref_cmn(x, *setting), R.cmn_slack(x, *setting))
            differ, total = differ + d, total + n
            if steps > 1.0:
                bad.append((name, setting, steps))
            if name == 'silence':
                assert not got.any(), setting
    print(f'{sr} Hz: {differ} of {total} CMN outputs are not the bits of the reference '
          f'({differ / total:.2e}; cap {R.CMN_SHARE})')
    assert not bad, bad
    assert differ <= R.CMN_SHARE * total


# ---- end to end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sr', R.RATES)
def test_features_against_the_reference(sr):
    ref = R.reference(sr)
    worst, bad = 0.0, []
    for setting in R.CMN_SETTINGS:
        for name, got in _rows_of(sr, _big(sr, setting)[1]):
            excess = R.fea_excess(got, R.ref_cmn(ref[name][0], *setting))
            worst = max(worst, excess)
            if excess > 1.0:
                bad.append((name, setting, excess * R.FEA_TOL))
    print(f'{sr} Hz: largest |feature - reference| = {worst * R.FEA_TOL:.3e} (tolerance {R.FEA_TOL})')
    assert not bad, bad


# ---- the run tables ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sr', R.RATES)
def test_a_segment_among_others_equals_the_segment_alone(sr):
    table, rows = _table(sr)
    names = [t[0] for t in table]
    assert names.count(TWICE) == 2 and min(t[1] for t in table) == 0 and max(t[1] + t[2] for t in table) == R.n_signal(sr)
    spans = sorted((a, a + n) for _, a, n, _ in table)
    assert sum(1 for (_, b0), (a1, _) in zip(spans, spans[1:]) if a1 < b0) >= 2
    dev = _device(sr)
    for setting in (DEFAULT, (5, 3)):
        lm, fea = _big(sr, setting)
        bad = []
        for name, a, n, row in table:
            nf = dev.run(R.recording(sr), np.array([(a, n)], dtype=np.int64), *setting)
            assert nf == fbank.n_frames(n, sr), name
            same = R.same_bits(dev.get('logmel', 0, nf), lm[row:row + nf]) and R.same_bits(dev.get('fea', 0, nf), fea[row:row + nf])
            if not same:
                bad.append(name)
        assert not bad, (setting, bad)


@pytest.mark.parametrize('sr', R.RATES)
def test_run_raw_tables_with_two_recordings(sr):
    _, shift, _, _ = R.dims(sr)
    fe = fbank.front_end(sr)
    recs, rng = [], np.random.default_rng(9 + sr)
    for k, frames in enumerate(((65, 2, 129, 64, 17, 129), (128, 16, 63, 300, 63))):
        n_rec = (310 if k else 200) * shift
        x = R.samples(n_rec, sr, seed=500 + k)[0]
        segs = []
        for j, N in enumerate(frames):
            n = shift * N - shift // 2 + int(rng.integers(0, shift))
            a = 0 if j == 0 else (n_rec - n if j == 1 else int(rng.integers(0, n_rec - n + 1)))
            if j == len(frames) - 1:
                a, n = segs[2].start, segs[2].n                     # one segment twice
            segs.append(fbank.Segment(j, a, n, fbank.n_frames(n, sr), (a, a + n)))
        recs.append((x, segs))
    seg_rows = fe.run_raw(recs)
    lm, fea = fe.get(0, fe.rows, which='logmel'), fe.get(0, fe.rows)
    bad = []
    for k, (x, segs) in enumerate(recs):
        sig = fbank.dither(x)
        for s, row in zip(segs, seg_rows[k]):
            assert R.logmel_excess(lm[row:row + s.nframes], R.ref_logmel(sig[s.start:s.start + s.n], sr)[0]) <= 1.0, (k, s.segnum)
            alone = [(y, [s] if i == k else []) for i, (y, _) in enumerate(recs)]
            assert fe.run_raw(alone)[k] == [0] and fe.rows == s.nframes
            if not (R.same_bits(fe.get(0, s.nframes, which='logmel'), lm[row:row + s.nframes])
                    and R.same_bits(fe.get(0, s.nframes), fea[row:row + s.nframes])):
                bad.append((k, s.segnum))
    assert not bad, bad
    # and the dithered signal is the host's, so the rows are those of run() on it
    sig = [fbank.dither(x) for x, _ in recs]
    fe.run(list(zip(sig, (segs for _, segs in recs))))
    assert R.same_bits(fe.get(0, fe.rows, which='logmel'), lm) and R.same_bits(fe.get(0, fe.rows), fea)


# ---- capacity reuse ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sr', R.RATES)
def test_small_run_after_a_large_one(sr):
    table, rows = _table(sr)
    dev = _device(sr)
    assert _run(dev, sr, table, *DEFAULT) == rows
    name, a, n = next(c for c in R.cases(sr) if c[0] == 'N2max')
    seg = np.array([(a, n)], dtype=np.int64)
    assert dev.run(R.recording(sr), seg, 5, 3) == 2 == dev.rows
    fresh = _new_device(sr)
    assert fresh.run(R.recording(sr), seg, 5, 3) == 2
    for which in ('logmel', 'fea'):
        assert R.same_bits(dev.get(which, 0, 2), fresh.get(which, 0, 2)), which
    assert R.same_bits(dev.windows([0], 2), fresh.windows([0], 2))
    fresh.close()
    for call in (lambda: dev.get('fea', 0, 3), lambda: dev.get('logmel', 2, 1), lambda: dev.get('fea', rows - 1, 1),
                 lambda: dev.windows([0], 3), lambda: dev.windows([1], 2), lambda: dev.windows_ragged([0, rows - 5], [2, 5])):
        with pytest.raises(_capi.VbxError):
            call()
    assert R.logmel_excess(dev.get('logmel', 0, 2), R.reference(sr)[name][0]) <= 1.0


# ---- the gather kernels --------------------------------------------------------------------------------------------
def _loaded(sr):
    """The device holding the rate's one run at the default window, and its feature rows."""
    table, rows = _table(sr)
    dev = _device(sr)
    assert _run(dev, sr, table, *DEFAULT) == rows
    fea = dev.get('fea', 0, rows)
    assert R.same_bits(fea, _big(sr, DEFAULT)[1])
    return dev, fea, [t[3] for t in table[1:]]


@pytest.mark.parametrize('sr', R.RATES)
def test_windows_are_transposed_slices_of_the_feature_rows(sr):
    dev, fea, cuts = _loaded(sr)
    rows = len(fea)
    for length in R.GATHER_LENGTHS:
        across = [c - (length + 1) // 2 for c in cuts if length > 1 and 0 <= c - (length + 1) // 2 <= rows - length][::8]
        assert len(across) >= 3 or length == 1                      # (windows over the cut between two segments)
        starts = [0, rows - length] + across
        got = dev.windows(starts, length)
        assert got.shape == (len(starts), 64, length) and got.dtype == np.float32
        bad = [s for s, w in zip(starts, got) if not R.same_bits(w, R.gather_ref(fea, s, length))]
        assert not bad, (length, bad)


@pytest.mark.parametrize('sr', R.RATES)
def test_ragged_windows_and_their_offsets(sr):
    dev, fea, cuts = _loaded(sr)
    rows = len(fea)
    for length in R.GATHER_LENGTHS:                                 # one window
        s = rows - length
        got = dev.windows_ragged([s], [length])
        assert got.shape == (64 * length,) and R.same_bits(got.reshape(64, length), R.gather_ref(fea, s, length)), length
    rng = np.random.default_rng(41 + sr)
    lens = np.array(R.GATHER_LENGTHS * 26, dtype=np.int32)          # 312 windows, every length 26 times, mixed
    rng.shuffle(lens)
    starts = np.array([int(rng.integers(0, rows - n + 1)) for n in lens], dtype=np.int64)
    starts[:len(R.GATHER_LENGTHS)] = 0
    starts[-len(R.GATHER_LENGTHS):] = rows - lens[-len(R.GATHER_LENGTHS):]
    got = dev.windows_ragged(starts, lens)
    off = 64 * np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
    assert got.shape == (off[-1],)
    bad = [(w, int(s), int(n)) for w, (s, n) in enumerate(zip(starts, lens))
           if not R.same_bits(got[off[w]:off[w + 1]].reshape(64, n), R.gather_ref(fea, s, n))]
    assert not bad, bad[:10]


# ---- refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sr', R.RATES)
def test_refusals_leave_the_object_usable(sr):
    pre = R.dims(sr)[0]
    dev, x, total = _device(sr), R.recording(sr), R.n_signal(sr)
    segs = np.array([c[1:] for c in R.cases(sr)[:12]], dtype=np.int64)
    rows = dev.run(x, segs, 5, 3)
    before = dev.get('logmel', 0, rows), dev.get('fea', 0, rows), dev.windows([0, rows - 65], 65)
    good = (1000, 2000)
    for bad_segs, lc in (([good, (500, pre)], 5), ([(500, pre + 1), good], 5), ([good, (-1, 2000)], 5),
                         ([good, (total - 1999, 2000)], 5), ([good], -1)):
        with pytest.raises(_capi.VbxError):
            dev.run(x, np.array(bad_segs, dtype=np.int64), lc, 3)
    with pytest.raises(_capi.VbxError):
        dev.run(x, np.array([good], dtype=np.int64), 5, -1)
    for call in (lambda: dev.get('fea', rows - 1, 2), lambda: dev.get('logmel', 0, rows + 1), lambda: dev.windows([0], 0),
                 lambda: dev.windows_ragged([0, 0], [5, 0])):
        with pytest.raises(_capi.VbxError):
            call()
    assert dev.run(x, segs, 5, 3) == rows
    after = dev.get('logmel', 0, rows), dev.get('fea', 0, rows), dev.windows([0, rows - 65], 65)
    assert all(R.same_bits(a, b) for a, b in zip(before, after))
    assert dev.run(x, np.array([(total - 2000, 2000)], dtype=np.int64), 5, 3) == fbank.n_frames(2000, sr)   # the last sample itself
