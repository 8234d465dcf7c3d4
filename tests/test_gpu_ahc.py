"""GPU parity of the AHC score stage (vbhmm.py:135-138): cos_similarity and twoGMMcalib_lin through the
C ABI against the reference's golden outputs and the CPU oracle.  float64 end to end; the tolerances are
the rounding of sums taken in a different order."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ahc_cases.npz')


@pytest.fixture(scope='module')
def ahc_cases():
    npz = np.load(GOLDEN)
    out = {}
    for key in npz.files:
        case, field = key.split('/', 1)
        out.setdefault(case, {})[field] = npz[key]
    return out


def test_cos_similarity_and_calibration_match_the_reference(ahc_cases):
    from vbx_amd.diarization_lib import cos_similarity, twoGMMcalib_lin
    for name, c in ahc_cases.items():
        x = c['x'].copy()
        scr = cos_similarity(x)
        assert np.array_equal(x, c['x']), 'input mutated'
        assert scr.dtype == np.float64 and scr.shape == (len(x), len(x))
        np.testing.assert_allclose(scr.ravel()[c['scr_sample_idx']], c['scr_sample'], rtol=0, atol=5e-15, err_msg=name)
        stats = np.array([scr.sum(), (scr ** 2).sum(), scr.min(), scr.max(), np.trace(scr)])
        np.testing.assert_allclose(stats, c['scr_stats'], rtol=1e-12, err_msg=name)
        assert np.abs(scr - scr.T).max() <= 1e-15
        thr, llr = twoGMMcalib_lin(scr.ravel())
        assert isinstance(thr, np.float64) and llr.shape == (scr.size,)
        np.testing.assert_allclose(thr, c['thr'], rtol=1e-10, err_msg=name)
        np.testing.assert_allclose(llr[c['scr_sample_idx']], c['llr_sample'], rtol=1e-9, atol=1e-9, err_msg=name)
        llr_stats = np.array([llr.sum(), (llr ** 2).sum(), llr.min(), llr.max()])
        np.testing.assert_allclose(llr_stats, c['llr_stats'], rtol=1e-9, err_msg=name)
        thr5, _ = twoGMMcalib_lin(scr.ravel().copy(), niters=5)
        np.testing.assert_allclose(thr5, c['thr5'], rtol=1e-10, err_msg=name)


def test_score_matrix_is_an_ordinary_array_and_in_place_edits_reach_the_calibration():
    """The reference returns a plain writable matrix (diarization_lib.py:213) and callers edit it in place; whatever
    they hand to twoGMMcalib_lin afterwards is what gets calibrated."""
    from vbx_amd import diarization_lib as dl
    from oracle import ahc_oracle
    x = np.random.default_rng(0).standard_normal((200, 32))
    scr = dl.cos_similarity(x)
    assert scr.flags.writeable and scr.flags.owndata and scr.flags.c_contiguous
    ref = ahc_oracle.cos_similarity(x)
    np.fill_diagonal(scr, 0.25)                                      # in-place edits of every kind ...
    np.fill_diagonal(ref, 0.25)
    scr *= -1
    ref *= -1
    scr[scr > 0.3] = 0.3
    ref[ref > 0.3] = 0.3
    thr, llr = dl.twoGMMcalib_lin(scr.ravel())                       # ... are what the calibration sees
    thr_o, llr_o = ahc_oracle.twoGMMcalib_lin(ref.ravel())
    np.testing.assert_allclose(thr, thr_o, rtol=1e-9)
    np.testing.assert_allclose(llr, llr_o, rtol=1e-8, atol=1e-8)
    with pytest.raises(ValueError):
        dl.twoGMMcalib_lin(scr)                                      # 2-D: the reference's s[:, np.newaxis] would fail too


@pytest.mark.parametrize('T,D', [(1, 8), (63, 5), (65, 128), (1000, 257)])
def test_shapes_and_edges_against_the_oracle(T, D):
    from vbx_amd.diarization_lib import cos_similarity, twoGMMcalib_lin
    from oracle import ahc_oracle
    x = np.random.default_rng(T + D).standard_normal((T, D)) * 3
    scr = cos_similarity(x)
    np.testing.assert_allclose(scr, ahc_oracle.cos_similarity(x), rtol=0, atol=5e-15)
    if T >= 63:
        thr, llr = twoGMMcalib_lin(scr.ravel(), niters=7)
        thr_o, llr_o = ahc_oracle.twoGMMcalib_lin(ahc_oracle.cos_similarity(x).ravel(), niters=7)
        np.testing.assert_allclose(thr, thr_o, rtol=1e-9)
        np.testing.assert_allclose(llr, llr_o, rtol=1e-8, atol=1e-8)


def test_headline_size_score_stage_properties():
    """T = 10 000 (the headline recording length): 1e8 scores, 800 MB resident.  Oracle-free properties:
    unit diagonal, symmetry, range, and the calibration's fixed point (one more pass does not move it)."""
    from vbx_amd.diarization_lib import cos_similarity, twoGMMcalib_lin
    rng = np.random.default_rng(1)
    centres = rng.standard_normal((6, 128))
    x = centres[rng.integers(0, 6, 10000)] + 0.8 * rng.standard_normal((10000, 128))
    scr = cos_similarity(x)
    np.testing.assert_allclose(np.diag(scr), 1.0, atol=1e-14)
    assert scr.min() >= -1.0001 and scr.max() <= 1.0001                   # diarization_lib.py:211-212
    i, j = rng.integers(0, 10000, 500), rng.integers(0, 10000, 500)
    np.testing.assert_allclose(scr[i, j], scr[j, i], rtol=0, atol=1e-15)
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    np.testing.assert_allclose(scr[i, j], np.einsum('kd,kd->k', xn[i], xn[j]), rtol=0, atol=5e-15)
    thr40, _ = twoGMMcalib_lin(scr.ravel(), niters=40)
    thr41, _ = twoGMMcalib_lin(scr.ravel(), niters=41)
    assert abs(thr40 - thr41) < 1e-6 and -1 < thr40 < 1


@pytest.mark.parametrize('T', [1, 2, 3, 64, 65, 257, 1025])
def test_condensed_negated_matrix_is_squareform_of_the_device_matrix(T):
    """vbx_scores_get_condensed(scale = -1) == scipy.spatial.distance.squareform(-scr_mx, checks=False) of the very
    matrix the device holds (vbhmm.py:139): bit for bit, sign of zero included; a vector that is not T x T is refused."""
    from scipy.spatial.distance import squareform
    from vbx_amd import _capi
    ctx = _capi.default_context(None)
    x = np.random.default_rng(T).standard_normal((T, 24))
    x[0] = 0.0                                                   # a zero row: similarities exactly 0 -> -0.0 after negation
    scores = _capi.Scores.cos_similarity(ctx, x)
    try:
        full = scores.get().reshape(T, T)
        cond = scores.get_condensed(T, -1.0)
        want = squareform(-full, checks=False) if T > 1 else np.empty(0)
        assert cond.shape == want.shape and np.array_equal(cond, want)
        assert np.array_equal(np.signbit(cond), np.signbit(want))
        assert np.array_equal(scores.get_condensed(T, 1.0), -want if T > 1 else want)
        if T > 2:
            with pytest.raises(_capi.VbxError):
                scores.get_condensed(T - 1, -1.0)
    finally:
        scores.close()


# ---- the calibration kernels at their edges: score VECTORS of any length, skewed and overlapping mixtures ----------------
# lengths: one or two workgroups (3, 255, 256, 257); nb = min(2048, ceil(n / 256)) saturating at kGmmPartials
CALIB_LENGTHS = (3, 255, 256, 257, 2048 * 256 - 1, 2048 * 256, 2048 * 256 + 1)
# (weight of the upper component, lower mean, upper mean, sd): symmetric; few same-speaker pairs, like a real score matrix;
# heavily overlapping
CALIB_MIXTURES = ((0.5, -1.0, 1.0, 0.3), (0.02, 0.0, 0.8, 0.1), (0.3, 0.1, 0.2, 0.2))
CALIB_NITERS = (1, 20)


def calib_scores(n, mix):
    w1, m0, m1, sd = CALIB_MIXTURES[mix]
    rng = np.random.default_rng(100 * mix + n % 1000)
    return np.where(rng.random(n) < w1, m1, m0) + sd * rng.standard_normal(n)


def calib_longdouble(s, niters):
    """oracle/ahc_oracle.twoGMMcalib_lin restated in np.longdouble, same statement order, the softmax done by hand;
    {k: (threshold, llr)} after each number of iterations k in niters"""
    s = np.asarray(s, dtype=np.longdouble)
    one, half = np.longdouble(1), np.longdouble(0.5)
    weights = np.array([half, half])
    means = np.mean(s) + np.std(s) * np.array([-one, one])
    var = np.var(s)
    out = {}
    for it in range(1, max(niters) + 1):
        lls = np.log(weights) - half * np.log(var) - half * (s[:, np.newaxis] - means) ** 2 / var
        e = np.exp(lls - lls.max(axis=1, keepdims=True))
        gammas = e / e.sum(axis=1, keepdims=True)
        cnts = np.sum(gammas, axis=0)
        weights = cnts / cnts.sum()
        means = s.dot(gammas) / cnts
        var = ((s ** 2).dot(gammas) / cnts - means ** 2).dot(weights)
        threshold = -half * (np.log(weights ** 2 / var) - means ** 2 / var).dot([one, -one]) / (means / var).dot([one, -one])
        if it in niters:
            out[it] = (threshold, lls[:, means.argmax()] - lls[:, means.argmin()])
    return out


def device_calib(s, niters, want_llr=True):
    from vbx_amd import _capi
    sc = _capi.Scores.upload(_capi.default_context(), s)
    try:
        return sc.two_gmm_calib(niters, want_llr)
    finally:
        sc.close()


@pytest.mark.parametrize('mix', range(len(CALIB_MIXTURES)))
@pytest.mark.parametrize('n', CALIB_LENGTHS)
def test_calibration_of_score_vectors_against_longdouble(n, mix):
    """gmm_* on vectors through Scores.upload, 1 and 20 passes, against the np.longdouble restatement of the oracle:
    threshold within 1e-9 std(s) (the project's 1e-9 on the scale of the scores: the symmetric mixture's threshold sits
    near 0, where a relative bound means nothing), LLRs at rtol = atol = 1e-8.  The float64 oracle is held to 1e-11 std(s)
    and 1e-10 in the same test, so a failure points at the device.  want_llr=False gives the same threshold bits."""
    from oracle import ahc_oracle
    s = calib_scores(n, mix)
    ref = calib_longdouble(s, CALIB_NITERS)
    sd = np.std(s)
    for niters in CALIB_NITERS:
        thr_ld, llr_ld = ref[niters]
        thr_o, llr_o = ahc_oracle.twoGMMcalib_lin(s, niters=niters)
        thr, llr = device_calib(s, niters)
        err = [abs(float(t - thr_ld)) / sd for t in (thr, thr_o)] + [float(np.max(np.abs(l - llr_ld))) for l in (llr, llr_o)]
        print(f'n={n} mix={mix} niters={niters}: threshold error / std(s) device {err[0]:.2g} oracle {err[1]:.2g}; '
              f'largest LLR error device {err[2]:.2g} oracle {err[3]:.2g} (largest |LLR| {float(np.abs(llr_ld).max()):.3g})')
        assert np.isfinite(float(thr_ld)) and np.all(np.isfinite(llr_ld.astype(np.float64)))
        assert err[1] <= 1e-11
        np.testing.assert_allclose(llr_o, llr_ld.astype(np.float64), rtol=1e-10, atol=1e-10)
        assert err[0] <= 1e-9, (thr, float(thr_ld))
        np.testing.assert_allclose(llr, llr_ld.astype(np.float64), rtol=1e-8, atol=1e-8)
        thr_only, none = device_calib(s, niters, want_llr=False)
        assert none is None and np.array_equal([thr_only], [thr])


@pytest.mark.parametrize('case', ['two', 'constant'])
def test_calibration_of_degenerate_vectors_is_nan_where_the_reference_is(case):
    """Two scores, and 1000 equal ones (0.25: every sum is exact, the variance exactly 0): the reference divides by a
    vanishing variance and returns NaN.  That is arithmetic, not a fault -- gmm_* has no data-dependent loop or index -- so
    the device returns NaN where the np.longdouble reference does, a close threshold where it does not, and no error."""
    s = calib_scores(2, 0) if case == 'two' else np.full(1000, 0.25)
    with np.errstate(all='ignore'):
        ref = calib_longdouble(s, CALIB_NITERS)
        for niters in CALIB_NITERS:
            thr_ld, llr_ld = ref[niters]
            thr, llr = device_calib(s, niters)
            print(f'{case} niters={niters}: threshold device {thr} reference {float(thr_ld)}')
            assert np.isnan(thr) == np.isnan(float(thr_ld))
            assert np.array_equal(np.isnan(llr), np.isnan(llr_ld.astype(np.float64)))
            if not np.isnan(thr):
                assert abs(thr - float(thr_ld)) <= 1e-9 * np.std(s)
                np.testing.assert_allclose(llr, llr_ld.astype(np.float64), rtol=1e-8, atol=1e-8)
            thr_only, _ = device_calib(s, niters, want_llr=False)
            assert np.array_equal([thr_only], [thr], equal_nan=True)
        assert np.isnan(float(ref[20][0]))
