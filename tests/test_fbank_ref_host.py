"""tests/fbank_ref.py on the CPU: its reference reproduces the fixture of the unmodified predict.py, its inputs meet the
conditions the GPU tests rely on, and its comparison functions see every fault of the front end's kernels that a reading of
vbx_fbank.hpp suggests -- each wrong model below misses the tolerance of tests/test_gpu_fbank_kernels.py by a factor of at
least 100 on a named case of the shared tables."""
import os

import numpy as np
import pytest

import fbank_ref as R
from vbx_amd import fbank

G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'fbank_cases.npz'))
NAMES = [str(n) for n in G['names']]
RATE = dict(zip(NAMES, (int(r) for r in G['rates'])))


# ---- the reference against the fixture -----------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_reference_reproduces_the_fixture(name):
    sr = RATE[name]
    labs = np.atleast_2d((np.loadtxt(str(G['lab_' + name]).splitlines(), usecols=(0, 1)) * sr).astype(int))
    sig = fbank.dither(G['sig_' + name].astype(int))
    segs = fbank.segments(labs, len(sig), sr)
    fea, row = G['fea_' + name], 0
    for j, s in enumerate(segs):
        lm, _ = R.ref_logmel(sig[s.start:s.start + s.n], sr)
        assert len(lm) == s.nframes
        if j == 0:
            ref = G['logmel_' + name]
            assert np.abs(lm[:len(ref)] - ref).max() <= 1e-9
        got = R.ref_cmn(lm, fbank.CMN_LC, fbank.CMN_RC).astype(np.float32)
        assert np.abs(got.astype(np.float64) - fea[row:row + s.nframes]).max() <= 1e-12
        row += s.nframes
    assert row == len(fea)


# ---- the inputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sr', R.RATES)
def test_case_table(sr):
    pre, shift, winlen, _ = R.dims(sr)
    cases = R.cases(sr)
    by_name = {c[0]: c[1:] for c in cases}
    assert len(by_name) == len(cases) == 6 + 2 * len(R.FRAME_COUNTS) + 2
    mirror = [R.smallest(sr), pre + 20, shift + 1, winlen // 2 - 1, winlen // 2, winlen // 2 + 1]
    assert [by_name[k][1] for k in R.case_ids(sr)[:6]] == mirror
    ref = R.reference(sr)
    for N in R.FRAME_COUNTS:
        for which, n in (('min', shift * N - shift // 2), ('max', shift * N - shift // 2 + shift - 1)):
            assert by_name[f'N{N}{which}'][1] == n
            assert fbank.n_frames(n, sr) == N == len(ref[f'N{N}{which}'][0])
        assert fbank.n_frames(shift * N - shift // 2 - 1, sr) == N - 1 and fbank.n_frames(shift * N + shift // 2, sr) == N + 1
    for name, a, n in cases:
        assert fbank.n_frames(n, sr) == len(ref[name][0]) >= 1
        assert 0 <= a and a + n <= R.n_signal(sr)
    assert fbank.n_frames(R.smallest(sr), sr) == 1 and fbank.n_frames(R.smallest(sr) - 1, sr) == 0
    assert R.smallest(sr) == {16000: 140, 8000: 70}[sr] > pre + 1
    assert len(ref['tone'][0]) == 65 and max(len(v[0]) for v in ref.values()) == 470
    assert R.n_signal(sr) < 10 * sr
    assert min(a for _, a, _ in cases) == 0 and max(a + n for _, a, n in cases) == R.n_signal(sr)
    spans = sorted((a, a + n) for _, a, n in cases)
    assert sum(1 for (a0, b0), (a1, b1) in zip(spans, spans[1:]) if a1 < b0) >= 2      # overlapping pairs


@pytest.mark.parametrize('sr', R.RATES)
def test_no_case_sits_on_the_floor_of_the_log(sr):
    ref = R.reference(sr)
    low = {name: float(acc.min()) for name, (_, acc) in ref.items() if name != 'silence'}
    worst = min(low, key=low.get)
    print(f'{sr} Hz: smallest Mel sum {low[worst]:.3g} ({worst})')
    assert low[worst] >= 2.0
    lm, acc = ref['silence']
    assert not lm.any() and not acc.any()
    for lc, rc in R.CMN_SETTINGS:
        assert not R.ref_cmn(lm, lc, rc).any()


def test_loud_tone_is_the_case_an_f32_transform_misses():
    # the same steps with the transform in float32: the loud bins' rounding error lands in the quiet bands
    for sr in R.RATES:
        _, _, winlen, nfft = R.dims(sr)
        fr = R.cut(R.pad(R.segment(sr, 'tone'), sr), sr)
        z = fr - fr.mean(axis=1, keepdims=True)
        y = np.concatenate([z[:, :1] * (1 - R.PREEMPH), z[:, 1:] - R.PREEMPH * z[:, :-1]], axis=1) * fbank.povey_window(winlen)
        y32 = np.zeros((len(y), nfft), dtype=np.float32)
        y32[:, :winlen] = y
        q = (np.arange(nfft // 2 + 1)[:, None] * np.arange(nfft)[None, :]) % nfft
        ang = (2 * np.pi * q / nfft)
        re, im = y32 @ np.cos(ang).astype(np.float32).T, y32 @ np.sin(ang).astype(np.float32).T
        acc = (re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2) @ fbank.mel_matrix(sr)
        err = R.logmel_excess(np.log(np.maximum(1.0, acc)), R.reference(sr)['tone'][0])
        print(f'{sr} Hz: an f32 transform is {err:.0f} x the log-Mel tolerance off on the tone')
        assert err >= 100


# ---- the two CMN formulations --------------------------------------------------------------------------------------
def _running_cmn(x, lc, rc, drop_at_block=False):
    """The kernel's own formulation: the window sum of a 16-frame run is summed directly at the run's first frame, then
    slid by one frame at a time.  drop_at_block: the sum is not restarted at a 64-frame boundary, and that frame's slide
    is lost (a wrong model)."""
    N = len(x)
    win = min(N, lc + rc + 1)
    out = np.empty_like(x)
    total, ws_prev = None, -1
    for t in range(N):
        ws = max(min(t - lc, N - win), 0)
        if t % 16 == 0 and not (drop_at_block and t % 64 == 0 and t > 0):
            total = x[ws:ws + win].sum(0)
        elif t % 16 != 0 and ws != ws_prev:
            total = total + (x[ws + win - 1] - x[ws_prev])             # (the kernel's sum += a - b)
        ws_prev = ws
        out[t] = x[t] - total / win
    return out


@pytest.mark.parametrize('sr', R.RATES)
def test_cmn_formulations_agree_within_the_cap(sr):
    ref = R.reference(sr)
    # host_cmn takes differences of cumulative sums over the whole segment, N terms of up to N X each way; at a window of
    # one frame, where the reference is exactly 0, c[t + 1] - c[t] is x[t] only up to that rounding, so there its outputs
    # "differ" from 0 by 1e-13: its cap is on the outputs that differ by more than the rounding slack
    for label, other, terms, strict in (('host_cmn', fbank.host_cmn, lambda N: 2 * N * N, False),
                                        ('running sums', _running_cmn, lambda N: None, True)):
        differ = beyond = total = 0
        worst = 0.0
        for name, (lm, _) in ref.items():
            for lc, rc in R.CMN_SETTINGS:
                w, d, b, n = R.cmn_steps(other(lm, lc, rc).astype(np.float32), R.ref_cmn(lm, lc, rc),
                                         R.cmn_slack(lm, lc, rc, terms(len(lm))))
                differ, beyond, total, worst = differ + d, beyond + b, total + n, max(worst, w)
        print(f'{sr} Hz, {label}: {differ} of {total} float32 outputs differ from ref_cmn ({differ / total:.2e}), {beyond} '
              f'by more than float64 rounding, at most {worst:g} step')
        assert (differ if strict else beyond) <= R.CMN_SHARE * total and worst <= 1.0


# ---- negative controls ---------------------------------------------------------------------------------------------
def _worst(sr, model, names=None):
    """(factor over LOGMEL_TOL, case) of a wrong log-Mel model on the case it misses most; the count of frames is the
    host's, as on the device."""
    ref = R.reference(sr)
    out = (0.0, None)
    for name in (names or R.case_ids(sr)):
        if name == 'silence':
            continue
        out = max(out, (R.logmel_excess(model(R.segment(sr, name), sr), ref[name][0]), name), key=lambda v: v[0])
    return out


def _lead_off_by_one(seg, sr):
    pre = R.dims(sr)[0]
    padded = R.pad(seg, sr)
    padded[:pre] = seg[1:pre + 1][::-1]                             # the mirror leaves sample 0 out
    return R.frames_to_logmel(R.cut(padded, sr), sr)[0]


def _trail_cap_short(seg, sr):
    pre, _, winlen, _ = R.dims(sr)
    padded = np.concatenate([seg[:pre][::-1], seg, seg[::-1][:min(winlen // 2 - 1, len(seg))]])
    return R.frames_to_logmel(R.cut(padded, sr), sr)[0]


def _hop(d):
    def model(seg, sr):
        _, shift, winlen, _ = R.dims(sr)
        padded = R.pad(seg, sr)
        nf = (len(padded) - winlen) // shift + 1
        padded = np.concatenate([padded, np.zeros(nf + winlen)])
        return R.frames_to_logmel(np.stack([padded[f * (shift + d):f * (shift + d) + winlen] for f in range(nf)]), sr)[0]
    return model


def _tile_staging(garbage, fill_from=0):
    """The frame kernel's staging: a tile of 64 frames reads (64 - 1) shift + winlen positions of the padded segment, and
    positions from padlen + fill_from on hold `garbage`; all 64 rows are transformed, the segment's own are kept."""
    def model(seg, sr):
        _, shift, winlen, _ = R.dims(sr)
        padded = R.pad(seg, sr)
        nf = (len(padded) - winlen) // shift + 1
        rows = []
        for f0 in range(0, nf, 64):
            span = np.full(63 * shift + winlen, garbage, dtype=np.float64)
            have = padded[f0 * shift:min(len(padded) + fill_from, f0 * shift + len(span))]
            span[:len(have)] = have
            tile = np.stack([span[f * shift:f * shift + winlen] for f in range(64)])
            rows.append(R.frames_to_logmel(tile, sr)[0][:min(64, nf - f0)])
        return np.concatenate(rows)
    return model


LOGMEL_CONTROLS = [('leading mirror off by one sample', _lead_off_by_one),
                   ('trailing mirror capped at winlen/2 - 1', _trail_cap_short),
                   ('frames cut at shift + 1', _hop(1)), ('frames cut at shift - 1', _hop(-1)),
                   ('fill past padlen begins one sample early', _tile_staging(0.0, -1))]


@pytest.mark.parametrize('sr', R.RATES)
@pytest.mark.parametrize('label,model', LOGMEL_CONTROLS, ids=[c[0] for c in LOGMEL_CONTROLS])
def test_logmel_faults_are_seen(sr, label, model):
    factor, name = _worst(sr, model)
    print(f'{sr} Hz, {label}: {factor:.3g} x the log-Mel tolerance on {name}')
    assert factor >= 100
    # and the features see it as well, through the CMN and the float32 cast
    lm = R.reference(sr)[name][0]
    wrong = model(R.segment(sr, name), sr)
    if wrong.shape == lm.shape:
        e2e = max(R.fea_excess(R.ref_cmn(wrong, lc, rc).astype(np.float32), R.ref_cmn(lm, lc, rc)) for lc, rc in R.CMN_SETTINGS)
        print(f'    {e2e:.3g} x the feature tolerance')
        assert e2e >= 100


@pytest.mark.parametrize('sr', R.RATES)
def test_where_the_edge_faults_show(sr):
    # the leading mirror: already on the smallest segment; the trailing cap: wherever the last frame ends on the last padded
    # sample, which is every smallest sample count of a frame count (a frame is lost) and none of the largest
    assert _worst(sr, _lead_off_by_one, ['mirror-smallest'])[0] >= 100
    assert _worst(sr, _trail_cap_short, ['N2min'])[0] == np.inf
    assert _worst(sr, _trail_cap_short, ['N2max'])[0] == 0.0
    # a tile of 64 frames whose fill begins early: the last frame of a segment that ends on the last padded sample
    assert _worst(sr, _tile_staging(0.0, -1), ['N65min'])[0] >= 100


@pytest.mark.parametrize('sr', R.RATES)
def test_what_lies_past_padlen_reaches_no_output(sr):
    """The zero fill of vbx_fbank.hpp past padlen, replaced by garbage: every frame of the segment ends at or before
    padlen and the rows of a matrix product do not mix, so only rows nobody reads change.  Not one bit of a log-Mel row
    depends on the fill: there is no output in which a test could see it, on the host or on the device.  (What the guard
    `p < padlen` does protect is the load itself: without it the mirror index runs below the segment's first sample.)"""
    model = _tile_staging(1e30)
    for name in R.case_ids(sr):
        assert R.same_bits(model(R.segment(sr, name), sr), _tile_staging(0.0)(R.segment(sr, name), sr)), name
    factor, name = _worst(sr, _tile_staging(0.0))                   # (the tiled model itself: the reference up to BLAS order)
    assert factor <= 1e-3


def _cmn_wrong(kind):
    def model(x, lc, rc):
        N = len(x)
        if kind == 'rc + 1':
            return R.ref_cmn(x, lc, rc + 1)
        if kind == 'lc - 1':
            return R.ref_cmn(x, max(lc - 1, 0), rc) if lc else None
        if kind == 'sum not restarted at a block boundary':
            return _running_cmn(x, lc, rc, drop_at_block=True)
        assert kind == 'window start clamped to N - win + 1'
        win = min(N, lc + rc + 1)
        xp = np.vstack([x, np.zeros((1, x.shape[1]))])              # (the row behind the segment)
        return np.stack([x[t] - xp[max(min(t - lc, N - win + 1), 0):][:win].mean(0) for t in range(N)])
    return model


CMN_CONTROLS = ['rc + 1', 'lc - 1', 'sum not restarted at a block boundary', 'window start clamped to N - win + 1']


def _cmn_worst(sr, kind, settings, max_frames):
    out = (0.0, None, None)
    for name, (lm, _) in R.reference(sr).items():
        if name == 'silence' or len(lm) > max_frames:
            continue
        for lc, rc in settings:
            wrong = _cmn_wrong(kind)(lm, lc, rc)
            if wrong is not None:
                steps = R.cmn_steps(wrong.astype(np.float32), R.ref_cmn(lm, lc, rc), R.cmn_slack(lm, lc, rc))[0]
                out = max(out, (steps, name, (lc, rc)), key=lambda v: v[0])
    return out


@pytest.mark.parametrize('sr', R.RATES)
@pytest.mark.parametrize('kind', CMN_CONTROLS)
def test_cmn_faults_are_seen_on_short_segments_under_short_windows(sr, kind):
    steps, name, setting = _cmn_worst(sr, kind, R.SHORT_WINDOWS, 65)
    print(f'{sr} Hz, CMN with {kind}: {steps:.3g} float32 steps (tolerance: 1) on {name} at (lc, rc) = {setting}')
    assert steps >= 100 and len(R.reference(sr)[name][0]) <= 65


@pytest.mark.parametrize('sr', R.RATES)
def test_the_default_window_sees_cmn_faults_from_300_frames_only(sr):
    default = [(fbank.CMN_LC, fbank.CMN_RC)]
    for kind in ('rc + 1', 'lc - 1'):
        assert _cmn_worst(sr, kind, default, 299)[0] == 0.0         # not one bit below 300 frames
        assert _cmn_worst(sr, kind, default, 470)[0] >= 100
    # the window start's upper clamp is reached at t = lc + 1: never in a segment of up to 129 frames
    assert _cmn_worst(sr, 'window start clamped to N - win + 1', default, 129)[0] == 0.0
    assert _cmn_worst(sr, 'window start clamped to N - win + 1', default, 299)[0] >= 100
    assert _cmn_worst(sr, 'sum not restarted at a block boundary', default, 299)[0] == 0.0


def _gather_model(fea, start, length, swapped):
    """fbank_gather_kernel in numpy, element by element as its threads walk; swapped: from the second pass on an element
    index is split by 128 instead of by the pass's own count of frames."""
    out = np.zeros(64 * length, dtype=fea.dtype)
    for c0 in range(0, length, 128):
        nc = min(128, length - c0)
        tile = fea[start + c0:start + c0 + nc]
        e = np.arange(nc * 64)
        div = 128 if swapped and c0 else nc
        c, t = e // div, e % div
        keep = (t < nc) & (c < 64)
        out[c[keep] * length + c0 + t[keep]] = tile[t[keep], c[keep]]
    return out.reshape(64, length)


def test_gather_fault_is_seen_where_the_second_pass_is_partial():
    fea = np.random.default_rng(5).standard_normal((700, 64)).astype(np.float32)
    for length in R.GATHER_LENGTHS:
        for start in (0, 700 - length, 301):
            assert R.same_bits(_gather_model(fea, start, length, False), R.gather_ref(fea, start, length))
        wrong = _gather_model(fea, 0, length, True)
        seen = not R.same_bits(wrong, R.gather_ref(fea, 0, length))
        assert seen == (length > 128 and length % 128 != 0), length
        if seen:
            factor = R.fea_excess(wrong, R.gather_ref(fea, 0, length).astype(np.float64))
            print(f'gather with 128 for the count of a later pass, len {length}: {factor:.3g} x the feature tolerance')
            assert factor >= 100
