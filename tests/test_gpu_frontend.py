"""The driver's device stages (vbx_frontend.hpp and the resident form of the AHC score stage) at every padding and tile
edge, against the long-double reference and the derived bounds of tests/frontend_ref.py:

  projections          xv_center_norm_kernel, xv_gemm_kernel behind vbx_xvectors_project / vbx_xvectors_get
  resident scores      vbx_cos_similarity_resident + two_gmm_calib(want_llr=False), the only form the driver uses
  qinit, arg-sort      qinit_kernel behind set_recording_resident, top2_kernel behind labels(), before any run

No tolerance here is fitted to what the device gives: they are frontend_ref's bounds (float64 numpy sits at a few
percent of them, tests/test_frontend_ref_host.py), bit-for-bit equalities, or the tolerances the suite already uses for
the same quantities (test_gpu_ahc.py, test_driver.py, test_gpu_parity.py)."""
import ctypes as C

import numpy as np
import pytest

import frontend_ref as fr

pytestmark = pytest.mark.gpu
IDS = [fr.shape_id(s) for s in fr.SHAPES]
PRECISIONS = ['fp64', 'fp32', 'fp32-split']


@pytest.fixture(scope='module')
def ctx():
    from vbx_amd import _capi
    return _capi.default_context(0)


def _storage(precision):
    return np.float64 if precision == 'fp64' else np.float32


def _project(ctx, c):
    from vbx_amd import _capi
    return _capi.XVectors(ctx, c['x'], c['mean1'], c['lda'], c['mean2'], c['plda_mu'], c['plda_tr'], c['fea_dim'])


@pytest.fixture(scope='module')
def projected(ctx):
    """shape -> (inputs, resident x-vectors, xproj and fea as the device holds them): projected once, read only."""
    cache = {}

    def get(shape):
        if shape not in cache:
            c = fr.make_case(shape)
            xv = _project(ctx, c)
            cache[shape] = (c, xv, xv.get('xproj'), xv.get('fea'))
        return cache[shape]
    yield get
    for _, xv, _, _ in cache.values():
        xv.close()


def _check_rows(c, xproj, fea, rows=None, tag=''):
    """xproj within xproj_bound of the long-double reference, fea within fea_bound of the long-double product of the
    device's own xproj; -> the two largest |error| / bound."""
    x = c['x'] if rows is None else c['x'][rows]
    ref = fr.project_ref(x, c['mean1'], c['lda'], c['mean2'], c['plda_mu'], c['plda_tr'], c['fea_dim'])
    tol = fr.xproj_bound(*ref[:3], c['lda'], c['mean2'])
    got_x, got_f = (xproj, fea) if rows is None else (xproj[rows], fea[rows])
    assert np.all(np.isfinite(got_x)) and np.all(np.isfinite(got_f))
    r_x = fr.ratio(got_x, ref[2], tol)
    fea_ref, fea_tol = fr.fea_bound(got_x, c['plda_mu'], c['plda_tr'], c['fea_dim'])
    r_f = fr.ratio(got_f, fea_ref, fea_tol)
    print(f'{tag}: |error| / bound: xproj {r_x:.4f}, fea {r_f:.4f}')
    assert r_x <= 1.0, (tag, 'xproj', r_x)
    assert r_f <= 1.0, (tag, 'fea', r_f)
    return r_x, r_f


# ---- projections ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', fr.SHAPES, ids=IDS)
def test_projections_lie_within_the_derived_bounds(shape, projected):
    n, din, dl, fea_dim, dtype = shape
    c, xv, xproj, fea = projected(shape)
    assert c['x'].dtype == dtype
    assert xproj.shape == (n, dl) and fea.shape == (n, fea_dim) and xproj.dtype == fea.dtype == np.float64
    _check_rows(c, xproj, fea, tag=fr.shape_id(shape))


@pytest.mark.parametrize('shape', fr.SHAPES, ids=IDS)
def test_row_ranges_read_the_same_bits_as_the_full_read(shape, projected):
    n, din, dl, fea_dim, dtype = shape
    c, xv, xproj, fea = projected(shape)
    ranges = {(0, n), (n - 1, 1), (n // 2, 0), (n, 0), (n // 3, n - n // 3), (min(1, n - 1), max(n - 2, 0)), (n // 2, (n + 3) // 4)}
    for which, full in (('xproj', xproj), ('fea', fea)):
        for row0, nrows in sorted(ranges):
            part = xv.get(which, row0, nrows)
            assert part.shape == (nrows, full.shape[1])
            assert np.array_equal(part.view(np.int64), full[row0:row0 + nrows].view(np.int64)), (which, row0, nrows)


@pytest.mark.parametrize('shape', fr.SHAPES, ids=IDS)
def test_a_power_of_two_scale_of_the_input_changes_no_bit(shape, ctx):
    """x * 2^k with mean1 = 0: the scaling is exact and the first normalisation removes it exactly."""
    c = dict(fr.make_case(shape))
    c['mean1'] = np.zeros_like(c['mean1'])
    out = []
    for k in (0, 20, -20):
        ck = dict(c, x=c['x'] * c['x'].dtype.type(2.0 ** k))
        assert ck['x'].dtype == c['x'].dtype and np.all(np.isfinite(ck['x'])) and np.all(ck['x'] != 0)
        assert np.array_equal(ck['x'].astype(np.float64), c['x'].astype(np.float64) * 2.0 ** k)          # (exact)
        xv = _project(ctx, ck)
        out.append((xv.get('xproj'), xv.get('fea')))
        xv.close()
    _check_rows(c, *out[0], tag=fr.shape_id(shape) + ' mean1=0')
    for xproj, fea in out[1:]:
        assert np.array_equal(xproj.view(np.int64), out[0][0].view(np.int64))
        assert np.array_equal(fea.view(np.int64), out[0][1].view(np.int64))


@pytest.mark.parametrize('bad', [17, 3])
def test_a_row_equal_to_the_mean_is_nan_and_spoils_no_other_row(bad, ctx):
    """x[bad] == mean1: the norm is 0 and numpy's l2_norm gives a NaN row (0 / 0).  Row 17 = n - 1 is the row the clamp of
    xv_gemm_kernel feeds to every ghost row of the last 16-row tile, which row 16 shares; row 3 sits in the middle of one."""
    from vbx_amd.vbhmm import l2_norm
    shape = (18, 63, 30, 17, np.float64)
    c = fr.make_case(shape, seed=77)
    c['x'][bad] = c['mean1']
    with np.errstate(invalid='ignore'):
        want = l2_norm(l2_norm(c['x'] - c['mean1']).dot(c['lda']) - c['mean2'])
    assert np.all(np.isnan(want[bad])) and np.all(np.isfinite(np.delete(want, bad, axis=0)))
    xv = _project(ctx, c)
    xproj, fea = xv.get('xproj'), xv.get('fea')
    xv.close()
    assert xproj.shape == (18, 30) and fea.shape == (18, 17)
    assert np.all(np.isnan(xproj[bad])) and np.all(np.isnan(fea[bad]))
    rows = np.array([t for t in range(18) if t != bad])
    _check_rows(c, xproj, fea, rows=rows, tag=f'degenerate row {bad}')


def test_bad_arguments_are_refused(ctx, projected):
    from vbx_amd import _capi
    shape = fr.SHAPES[2]
    n, din, dl, fea_dim, _ = shape
    c, xv, xproj, fea = projected(shape)
    lib = ctx._lib
    x, m1, lda, m2, mu, tr = (np.ascontiguousarray(c[k], dtype=np.float64) for k in ('x', 'mean1', 'lda', 'mean2', 'plda_mu', 'plda_tr'))

    def project(n_, fea_dim_):
        h = C.c_void_p()
        rc = lib.vbx_xvectors_project(ctx._h, n_, din, dl, fea_dim_, _capi._ptr(x), _capi.VBX_F64, _capi._ptr(m1), _capi._ptr(lda),
                                      _capi._ptr(m2), _capi._ptr(mu), _capi._ptr(tr), C.byref(h))
        assert not h.value
        ctx.check(rc, 'vbx_xvectors_project')

    for n_, fea_dim_ in ((n, 0), (n, dl + 1), (0, fea_dim), (n, -1), (-1, fea_dim)):
        with pytest.raises(_capi.VbxError, match='bad argument'):
            project(n_, fea_dim_)
    for which in ('xproj', 'fea'):
        for row0, nrows in ((0, n + 1), (n, 1), (n + 1, 0), (n - 1, 2)):
            with pytest.raises(_capi.VbxError):
                xv.get(which, row0, nrows)
        out = np.empty((1, dl))
        assert lib.vbx_xvectors_get(xv._h, 0 if which == 'xproj' else 1, -1, 1, _capi._ptr(out)) != 0
    for row0, T in ((0, 0), (0, n + 1), (n, 1), (-1, 2)):
        with pytest.raises(_capi.VbxError, match='bad argument'):
            _capi.Scores.cos_similarity_resident(ctx, xv, row0, T)
    # (the handle is as usable as before)
    assert np.array_equal(xv.get('xproj', 1, 3).view(np.int64), xproj[1:4].view(np.int64))


# ---- resident cosine scores and the calibration --------------------------------------------------------------------
@pytest.mark.parametrize('shape', [s for s in fr.SHAPES if s[2] in (7, 30, 129, 128)],
                         ids=[fr.shape_id(s) for s in fr.SHAPES if s[2] in (7, 30, 129, 128)])
def test_scores_of_resident_rows_are_the_scores_of_the_uploaded_rows(shape, ctx, projected):
    """Two "recordings" per projected set, from row 0 and from row n // 3 to the end.  The resident rows carry
    round_up(Dl, 4) - Dl columns of +0.0: lanes that add +0.0 to a partial sum of cos_norm_kernel, and Dp is the same either
    way, so the matrices are equal bit for bit."""
    from vbx_amd import _capi
    from oracle import ahc_oracle
    n, din, dl, fea_dim, _ = shape
    c, xv, xproj, fea = projected(shape)
    for row0 in sorted({0, n // 3}):
        T = n - row0
        rows = xv.get('xproj', row0, T)
        res = _capi.Scores.cos_similarity_resident(ctx, xv, row0, T)
        up = _capi.Scores.cos_similarity(ctx, rows)
        try:
            assert len(res) == len(up) == T * T
            m_res, m_up = res.get(), up.get()
            same = np.array_equal(m_res.view(np.int64), m_up.view(np.int64))
            print(f'{fr.shape_id(shape)} row0={row0} T={T}: resident == uploaded bit for bit: {same}')
            assert same
            np.testing.assert_allclose(m_res.reshape(T, T), ahc_oracle.cos_similarity(rows), rtol=0, atol=5e-15)
            if T >= 63:
                thr, llr = res.two_gmm_calib(20, want_llr=False)
                assert llr is None and isinstance(thr, float)
                assert np.array_equal(res.get().view(np.int64), m_res.view(np.int64))          # the scores are left alone
                thr_llr, llr_all = res.two_gmm_calib(20, want_llr=True)
                assert thr == thr_llr and llr_all.shape == (T * T,)
                thr_o, _ = ahc_oracle.twoGMMcalib_lin(ahc_oracle.cos_similarity(rows).ravel(), niters=20)
                np.testing.assert_allclose(thr, thr_o, rtol=1e-9)
                assert np.array_equal(res.get().view(np.int64), m_res.view(np.int64))
        finally:
            res.close()
            up.close()
    # one x-vector: its similarity with itself
    for row0 in sorted({0, n // 2, n - 1}):
        one = _capi.Scores.cos_similarity_resident(ctx, xv, row0, 1)
        try:
            np.testing.assert_allclose(one.get().reshape(1, 1), [[1.0]], rtol=0, atol=1e-15)
        finally:
            one.close()


# ---- the arg-sort --------------------------------------------------------------------------------------------------
# D = 8 from 16 speakers on: the responsibilities outgrow the staging block and are padded on the host (pack_matrix);
# D = 128: padded on the device (pad_gamma_kernel)
TOP2_CASES = [(1, 128), (2, 128), (3, 128), (16, 8), (16, 128), (17, 8), (17, 128), (64, 8), (64, 128), (65, 8), (65, 128), (300, 8)]


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('S,D', TOP2_CASES)
def test_top2_of_crafted_responsibilities_follows_the_stable_argsort(S, D, precision, ctx):
    """set_recording with a crafted gamma0, then labels() with no run in between: top2_kernel reads the padded rows the setter
    wrote.  Ties go to the lower index, in the batch's storage type: a pair float64 orders and float32 ties is a tie in fp32."""
    from vbx_amd import _capi
    T = 257
    g = fr.top2_patterns(T, S, seed=S)
    rng = np.random.default_rng(S * 1000 + D)
    X, Phi, pi0 = rng.standard_normal((T, D)), rng.uniform(0.5, 3.0, D), np.ones(S) / S
    batch = _capi.Batch(ctx, [T], [S], D, precision=precision, max_iters=1)
    try:
        for gdtype in (np.float64, np.float32):
            g0 = g.astype(gdtype)
            batch.set_recording(0, X, Phi, pi0, g0, 0.9, 0.3, 17.0)
            first, second = batch.labels(0)
            # (float32 responsibilities are exact in either storage type; float64 ones are rounded by an fp32 batch)
            want1, want2 = fr.top2_ref(g0, _storage(precision))
            assert first.shape == (T,) and np.array_equal(first, want1), (gdtype, np.flatnonzero(first != want1)[:5])
            if S == 1:
                assert second is None and want2 is None
            else:
                assert second.shape == (T,) and np.array_equal(second, want2), (gdtype, np.flatnonzero(second != want2)[:5])
            if S > 1:                                         # row 9 = [1/3, 1/3 + 1e-12, 1/4 ...]: ordered only where every bit is kept
                ordered = precision == 'fp64' and gdtype == np.float64
                assert (first[9], second[9]) == ((1, 0) if ordered else (0, 1))
            got = batch.result(0, want_model=False)['gamma']
            assert np.array_equal(got, g0.astype(_storage(precision)).astype(np.float64))
    finally:
        batch.close()


# ---- initial responsibilities from the AHC labels ------------------------------------------------------------------
QINIT_ROW0 = {40: 43, 257: 13}


@pytest.fixture(scope='module')
def qinit_sets(ctx):
    """fea_dim -> (resident x-vectors of 300 rows, Phi)."""
    out = {}
    for fea_dim in (17, 30):
        c = fr.make_case((300, 20, 30, fea_dim, np.float64), seed=500 + fea_dim)
        out[fea_dim] = (_project(ctx, c), np.random.default_rng(fea_dim).uniform(0.5, 3.0, fea_dim))
    yield out
    for xv, _ in out.values():
        xv.close()


def _labels(T, S, seed):
    """random labels, one value of 0 .. S - 1 never used (S > 1)"""
    rng = np.random.default_rng(seed)
    if S == 1:
        return np.zeros(T, dtype=np.int64), None
    unused = int(rng.integers(0, S))
    lab = rng.choice([s for s in range(S) if s != unused], size=T)
    return lab, unused


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('S', [1, 5, 16, 17])
@pytest.mark.parametrize('fea_dim,T', [(17, 40), (17, 257), (30, 40), (30, 257)])
def test_initial_responsibilities_are_the_two_values_of_the_softmax(fea_dim, T, S, precision, ctx, qinit_sets):
    """set_recording_resident, then labels() and result() before any run (the library answers both).
    With init_smoothing = 0 every entry is 1 / S and the arg-sort, by its tie rule, reports speakers 0 and 1 for every frame
    rather than the AHC labels; for a positive smoothing it reports the AHC label and the lowest other index."""
    from scipy.special import softmax
    from vbx_amd import _capi
    xv, Phi = qinit_sets[fea_dim]
    lab, unused = _labels(T, S, seed=fea_dim * T + S)
    assert unused is None or unused not in lab
    batch = _capi.Batch(ctx, [T], [S], fea_dim, precision=precision, max_iters=1)
    try:
        for smoothing in (7.0, 0.0):
            batch.set_recording_resident(0, xv, QINIT_ROW0[T], lab, smoothing, Phi, 0.9, 0.3, 17.0)
            first, second = batch.labels(0)
            res = batch.result(0, want_model=False)
            want, hi, lo = fr.qinit_ref(lab, S, smoothing)
            want = want.astype(_storage(precision)).astype(np.float64)
            assert res['gamma'].shape == (T, S) and np.array_equal(res['gamma'], want), (smoothing, np.abs(res['gamma'] - want).max())
            assert res['n_iters'] == 0 and np.array_equal(res['pi'], np.full(S, 1.0 / S))
            if precision == 'fp64':
                sm = softmax(smoothing * (np.arange(S)[None, :] == lab[:, None]), axis=1)
                assert np.all(np.abs(res['gamma'] - sm) <= 2 * np.spacing(sm))
            want1, want2 = fr.top2_ref(want, np.float64)
            if smoothing > 0:
                assert hi > lo or S == 1
                assert np.array_equal(want1, lab) and (S == 1 or np.array_equal(want2, np.where(lab == 0, 1, 0)))
            else:
                assert np.all(want1 == 0) and (S == 1 or np.all(want2 == 1))
            assert np.array_equal(first, want1)
            assert (second is None and S == 1) or np.array_equal(second, want2)
    finally:
        batch.close()


@pytest.mark.parametrize('S', [1, 5, 16, 17])
@pytest.mark.parametrize('fea_dim,T', [(17, 40), (17, 257), (30, 40), (30, 257)])
def test_one_iteration_from_resident_rows_and_labels(fea_dim, T, S, ctx, qinit_sets):
    """One EM iteration from the device-built responsibilities on the resident rows == one from the same rows and the same
    responsibilities uploaded (atol 1e-12, as test_resident_setter_and_clone_owner_in_a_stream_group) == the oracle (gamma
    atol 1e-9, ELBO rtol 1e-11, as test_device_stages_against_what_the_reference_driver_computed)."""
    from vbx_amd import _capi
    from oracle import vbx_oracle
    xv, Phi = qinit_sets[fea_dim]
    row0 = QINIT_ROW0[T]
    lab, _ = _labels(T, S, seed=fea_dim * T + S)
    fea = xv.get('fea', row0, T)
    for smoothing in (7.0, 0.0):
        q0, _, _ = fr.qinit_ref(lab, S, smoothing)
        res = {}
        for how in ('resident', 'uploaded'):
            batch = _capi.Batch(ctx, [T], [S], fea_dim, precision='fp64', max_iters=1)
            try:
                if how == 'resident':
                    batch.set_recording_resident(0, xv, row0, lab, smoothing, Phi, 0.9, 0.3, 17.0)
                else:
                    batch.set_recording(0, fea, Phi, np.ones(S) / S, q0, 0.9, 0.3, 17.0)
                batch.run(1, -np.inf)
                res[how] = batch.result(0, want_model=False)
            finally:
                batch.close()
        for key in ('gamma', 'pi', 'Li'):
            np.testing.assert_allclose(res['resident'][key], res['uploaded'][key], rtol=0, atol=1e-12, err_msg=key)
        g, p, L = vbx_oracle.VBx(fea, Phi, pi=S, gamma=q0, maxIters=1, epsilon=-1e300, loopProb=0.9, Fa=0.3, Fb=17.0)
        assert res['resident']['n_iters'] == 1
        np.testing.assert_allclose(res['resident']['gamma'], g, rtol=0, atol=1e-9)
        np.testing.assert_allclose(res['resident']['Li'], [L[0][0]], rtol=1e-11)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_labels_outside_the_speakers_are_refused_and_the_batch_stays_usable(precision, ctx, qinit_sets):
    from vbx_amd import _capi
    xv, Phi = qinit_sets[17]
    T, S = 40, 5
    lab, _ = _labels(T, S, seed=4)
    batch = _capi.Batch(ctx, [T], [S], 17, precision=precision, max_iters=1)
    try:
        for where, value in ((0, -1), (T - 1, S), (T // 2, S + 11), (3, -2 ** 31)):
            bad = lab.copy()
            bad[where] = value
            with pytest.raises(_capi.VbxError, match='outside'):
                batch.set_recording_resident(0, xv, 0, bad, 7.0, Phi, 0.9, 0.3, 17.0)
        with pytest.raises(_capi.VbxError, match='not in the resident'):
            batch.set_recording_resident(0, xv, xv.n - T + 1, lab, 7.0, Phi, 0.9, 0.3, 17.0)
        batch.set_recording_resident(0, xv, 0, lab, 7.0, Phi, 0.9, 0.3, 17.0)
        first, second = batch.labels(0)
        assert np.array_equal(first, lab) and np.array_equal(second, np.where(lab == 0, 1, 0))
        batch.run(1, -np.inf)
        res = batch.result(0, want_model=False)
        assert res['n_iters'] == 1 and np.all(np.isfinite(res['gamma'])) and np.isfinite(res['Li'][0])
        np.testing.assert_allclose(res['gamma'].sum(axis=1), 1.0, rtol=0, atol=1e-5)
    finally:
        batch.close()
