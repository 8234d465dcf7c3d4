"""The reference and the bounds of tests/frontend_ref.py, checked on the host: a correct float64 evaluation lies well
inside them, three subtly wrong ones far outside, at every shape tests/test_gpu_frontend.py runs on the device; and the
numpy statement of the device arg-sort on the tie patterns the device test uses."""
import numpy as np
import pytest

import frontend_ref as fr

IDS = [fr.shape_id(s) for s in fr.SHAPES]


@pytest.fixture(scope='module')
def refs():
    """shape -> (inputs, long-double intermediates, xproj tolerance): computed once, read only."""
    out = {}
    for shape in fr.SHAPES:
        c = fr.make_case(shape)
        ref = fr.project_ref(**c)
        out[shape] = (c, ref, fr.xproj_bound(*ref[:3], c['lda'], c['mean2']))
    return out


def _model(c, mutant=None):
    """The float64 evaluation of the projections, optionally with one of three mistakes a kernel could make."""
    x, lda = np.asarray(c['x'], dtype=np.float64), c['lda']
    d = x - c['mean1']
    y1 = d / np.sqrt((d * d).sum(axis=1))[:, np.newaxis]
    if mutant == 'y1_float32':                              # the centred rows kept in float32
        y1 = y1.astype(np.float32).astype(np.float64)
    if mutant == 'last_k_quad':                             # the last group of four k of the first product left out
        keep = fr.round_up(x.shape[1], 4) - 4
        z = y1[:, :keep].dot(lda[:keep]) - c['mean2']
    else:
        z = y1.dot(lda) - c['mean2']
    if mutant == 'mean2_last_column':                       # the last column's mean not subtracted
        z[:, -1] += c['mean2'][-1]
    xproj = z / np.sqrt((z * z).sum(axis=1))[:, np.newaxis]
    fea = (xproj - c['plda_mu']).dot(c['plda_tr'].T)[:, :c['fea_dim']]
    return xproj, fea


def test_long_double_is_finer_than_float64():
    """The reference needs a type with more than 53 bits (x86: 64); where long double IS float64 it proves nothing."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize('shape', fr.SHAPES, ids=IDS)
def test_float64_evaluation_lies_within_a_tenth_of_the_bounds(shape, refs):
    c, ref, tol = refs[shape]
    n, din, dl, fea_dim, dtype = shape
    assert c['x'].dtype == dtype and ref[2].shape == tol.shape == (n, dl) and ref[3].shape == (n, fea_dim)
    y1_64, z_64, xproj_64, fea_64 = fr.project_ref(**c, dtype=np.float64)
    assert xproj_64.dtype == np.float64
    r_x = fr.ratio(xproj_64, ref[2], tol)
    fea_ref, fea_tol = fr.fea_bound(xproj_64, c['plda_mu'], c['plda_tr'], fea_dim)
    r_f = fr.ratio(fea_64, fea_ref, fea_tol)
    print(f'{fr.shape_id(shape)}: float64 / bound: xproj {r_x:.4f}, fea {r_f:.4f}; bounds up to {float(tol.max()):.2e}, {float(fea_tol.max()):.2e}')
    assert r_x <= 0.1 and r_f <= 0.1
    assert 0 < tol.min() and tol.max() < 1e-11 and 0 < fea_tol.min() and fea_tol.max() < 1e-11      # not vacuous
    # the model of this file is the same formula
    xproj_m, fea_m = _model(c)
    assert fr.ratio(xproj_m, ref[2], tol) <= 0.1 and fr.ratio(fea_m, fea_ref, fea_tol) <= 0.1


@pytest.mark.parametrize('mutant', ['last_k_quad', 'y1_float32', 'mean2_last_column'])
@pytest.mark.parametrize('shape', fr.SHAPES, ids=IDS)
def test_a_subtly_wrong_projection_is_far_outside_the_bound(shape, mutant, refs):
    c, ref, tol = refs[shape]
    xproj_m, _ = _model(c, mutant)
    r = fr.ratio(xproj_m, ref[2], tol)
    print(f'{fr.shape_id(shape)} {mutant}: {r:.3e} x the bound')
    assert r >= 1e3


def test_a_wrong_second_product_is_far_outside_its_bound(refs):
    """fea_bound isolates the second product: the plda mean left out, or a transform not transposed, is seen whatever
    xproj was."""
    for shape in fr.SHAPES:
        c, ref, _ = refs[shape]
        xproj = np.asarray(ref[2], dtype=np.float64)
        fea_ref, fea_tol = fr.fea_bound(xproj, c['plda_mu'], c['plda_tr'], c['fea_dim'])
        no_mean = xproj.dot(c['plda_tr'].T)[:, :c['fea_dim']]
        not_transposed = (xproj - c['plda_mu']).dot(c['plda_tr'])[:, :c['fea_dim']]
        assert fr.ratio(no_mean, fea_ref, fea_tol) >= 1e3 and fr.ratio(not_transposed, fea_ref, fea_tol) >= 1e3


@pytest.mark.parametrize('S', [1, 2, 3, 16, 17, 64, 65, 300])
def test_top2_reference_on_the_tie_patterns(S):
    """The numpy reference of the device arg-sort -- a stable argsort of -q in the storage type -- against a plain scan
    written out by hand, on the patterns the device test uploads."""
    g = fr.top2_patterns(257, S)
    assert g.shape == (257, S) and g.min() > 0
    for storage in (np.float64, np.float32):
        first, second = fr.top2_ref(g, storage)
        gs = g.astype(storage)
        assert (second is None) == (S == 1)
        for t in range(len(g)):
            best = max(gs[t])
            i1 = min(s for s in range(S) if gs[t, s] == best)
            assert first[t] == i1
            if S > 1:
                rest = [s for s in range(S) if s != i1]
                runner = max(gs[t, s] for s in rest)
                assert second[t] == min(s for s in rest if gs[t, s] == runner)
    if S > 1:
        # a pair that float64 orders and float32 ties: row 9 is [1/3, 1/3 + 1e-12, 1/4 ...]
        assert g[9, 1] > g[9, 0] and np.float32(g[9, 1]) == np.float32(g[9, 0])
        f64, f32 = fr.top2_ref(g[9:10], np.float64), fr.top2_ref(g[9:10], np.float32)
        assert (f64[0][0], f64[1][0]) == (1, 0) and (f32[0][0], f32[1][0]) == (0, 1)
    if S >= 3:
        rows = {k: g[k] for k in range(12)}
        assert np.sum(rows[3] == rows[3].max()) == 2 and np.sum(rows[4] == rows[4].max()) == 3
        assert np.all(rows[5] == rows[5][0])
        assert np.sum(rows[6] == rows[6].max()) == 1 and np.sum(rows[6] == np.sort(rows[6])[-2]) == 2
        assert np.all(np.diff(rows[7]) > 0) and np.all(np.diff(rows[8]) < 0)


def test_qinit_reference_is_the_softmax_of_the_smoothed_one_hot_rows():
    from scipy.special import softmax
    rng = np.random.default_rng(2)
    for S in (1, 5, 16, 17):
        for smoothing in (7.0, 0.0):
            lab = rng.integers(0, S, 40)
            g, hi, lo = fr.qinit_ref(lab, S, smoothing)
            onehot = np.zeros((40, S))
            onehot[range(40), lab] = 1.0
            want = softmax(smoothing * onehot, axis=1)
            assert np.all(np.abs(g - want) <= 2 * np.spacing(want))
            if S > 1:
                # (lo as the product e^-s hi and as the quotient e^-s / (1 + (S - 1) e^-s) are the same float64 here)
                z = np.exp(-smoothing)
                assert lo == z / (1.0 + (S - 1) * z)
