"""The one-step referee of tests/onestep_ref.py, checked on the CPU: its longdouble step is the reference's iteration (VBx_x in
both forms), no case of the table is vacuous or ill-conditioned, the bound rejects planted faults that today's end-to-end
tolerance lets through, and the plans the table expects cover every instance of the two chunk kernels."""
import numpy as np
import pytest

import onestep_ref as R
from oracle import vbx_oracle_x as ox

RECS = sorted({rec for case in R.CASES for rec in case.recs})
SHORT = [rec for rec in RECS if rec.T < 5000]
# the inputs the faults are planted in: the soft cases of a few tiles at every padded width
FAULT_RECS = [R.Rec(1100, 10), R.Rec(1100, 30), R.Rec(777, 10, 128, 0.05, 0.95), R.Rec(1300, 50, 128, 0.05, 0.95),
              R.Rec(4200, 20)]
FP64_TOL_TODAY = 2e-8         # gamma / pi of the fused fp64 kernels in the end-to-end tests


def _id(rec):
    return 'T{}-S{}-D{}-k{}-lp{}-Fa{}-Fb{}'.format(*rec)


@pytest.mark.parametrize('form', ['linear', 'log'])
@pytest.mark.parametrize('rec', SHORT, ids=_id)
def test_the_longdouble_step_is_the_reference_iteration(rec, form):
    """Measured: gamma <= 2.3e-12, ELBO <= 3.2e-12 absolute; held to 1e-10 (T = 1 and T = 2 are among the cases)."""
    X, Phi, g0, pi0 = R.inputs(rec)
    truth = R.first_step(rec)[0]
    g, pi, Li, alpha, invL = ox.VBx_x(X, Phi, loopProb=rec.lp, Fa=rec.Fa, Fb=rec.Fb, pi=pi0, gamma=g0, maxIters=1,
                                      epsilon=-1e300, form=form, return_model=True)
    d = {'gamma': np.abs(g - truth.gamma).max(), 'pi': np.abs(pi - truth.pi).max(), 'Li': abs(Li[0][0] - truth.Li),
         'alpha': np.abs(alpha - truth.alpha).max(), 'invL': np.abs(invL - truth.invL).max()}
    print(_id(rec), form, {k: f'{float(v):.1e}' for k, v in d.items()})
    assert all(float(v) <= 1e-10 for v in d.values()), d


def test_one_and_two_frames_are_cases():
    assert {1, 2} <= {rec.T for rec in SHORT}


@pytest.mark.parametrize('rec', RECS, ids=_id)
def test_no_case_is_vacuous_or_ill_conditioned(rec):
    """A condition on the table, not a measurement: a hardened state has a floor of 1e-39 and any kernel passes."""
    fl = R.first_step(rec)[1]
    for name, (lo, hi) in R.FLOOR_RANGE.items():
        f = fl[name]['gamma']
        print(_id(rec), name, f'{f:.2e}')
        assert f <= hi, (name, f)
        if rec.T not in R.EXEMPT_T:
            assert f >= lo, (name, f)


def test_the_exempt_cases_are_the_edge_lengths_only():
    assert set(R.EXEMPT_T) == {1, 2, 3, 129} and set(R.EXEMPT_T) < set(R.EDGE_T)


def _faulty(rec, fault):
    X, Phi, g0, pi0 = R.inputs(rec)
    truth, fl = R.first_step(rec)
    bad = R.step(X, Phi, pi0, g0, rec.lp, rec.Fa, rec.Fb, fault=fault)
    dev, bnd = R.deviation(bad, truth), R.bound(fl['float64'], 'float64', R.referee_terms(truth))
    print(_id(rec), fault, {q: f'{dev[q]:.1e}/{bnd[q]:.1e}' for q in R.QUANTITIES})
    return dev, bnd


@pytest.mark.parametrize('rec', FAULT_RECS, ids=_id)
def test_a_frame_read_2e_minus_20_off_passes_today_and_fails_the_bound(rec):
    """Frame 127 of rho scaled by 1 + 2^-20 (one frame at a tile cut read with a relative error of 2^-20)."""
    dev, bnd = _faulty(rec, 'rho127')
    # gamma moves 2e-9 ... 1.2e-8: under today's 2e-8 -- but for T = 1100, S = 30, the most sensitive state of the table
    # (float64 floor 1e-13), where the same fault is worth 4.2e-8 and today's tolerance happens to see it
    if rec != R.Rec(1100, 30):
        assert dev['gamma'] <= FP64_TOL_TODAY and dev['pi'] <= FP64_TOL_TODAY
    assert dev['gamma'] > bnd['gamma']


@pytest.mark.parametrize('rec', FAULT_RECS, ids=_id)
def test_the_dropped_1e_minus_8_fails_the_bound(rec):
    """VBx.py:158 without its 1e-8: gamma 2e-7 ... 5e-7, ELBO 1e-5 ... 8e-4 absolute."""
    dev, bnd = _faulty(rec, 'no_eps')
    assert dev['gamma'] > bnd['gamma'] and dev['pi'] > bnd['pi'] and dev['Li'] > bnd['Li']


@pytest.mark.parametrize('rec', FAULT_RECS, ids=_id)
def test_a_tile_end_without_its_neighbour_fails_the_bound(rec):
    """The last frame of a 128-frame tile with the backward vector of a recording's end instead of the next tile's."""
    dev, bnd = _faulty(rec, 'tile_end')
    assert dev['gamma'] > bnd['gamma']


def test_the_bound_accepts_the_model_it_is_made_of():
    """Both variants of the model lie within their own floor, so within the bound (a check of the bookkeeping)."""
    rec = R.Rec(1100, 10)
    X, Phi, g0, pi0 = R.inputs(rec)
    truth, fl = R.first_step(rec)
    for name, prec in (('float64', 'fp64'), ('float32', 'fp32')):
        for seq in (False, True):
            dt = np.dtype(name)
            got = R.step(X.astype(dt), Phi.astype(dt), pi0, g0, rec.lp, rec.Fa, rec.Fb, dt, seq)
            ratio = R.check(got, truth, fl, prec, f'model seq={seq}')
            bnd = R.bound(fl[name], name, R.referee_terms(truth) if name == 'float64' else None)
            assert all(ratio[q] <= 1 / R.K for q in R.QUANTITIES if bnd[q] == R.K * fl[name][q]), ratio


def test_the_shared_assertion_fails_beyond_the_bound():
    rec = R.Rec(1100, 10)
    X, Phi, g0, pi0 = R.inputs(rec)
    truth, fl = R.first_step(rec)
    bad = R.step(X, Phi, pi0, g0, rec.lp, rec.Fa, rec.Fb, fault='rho127')
    with pytest.raises(AssertionError, match='beyond the bound'):
        R.check(bad, truth, fl, 'fp64', 'planted')


def test_the_expected_plans_cover_every_instance():
    """The closing condition of tests/test_gpu_onestep.py on the plans the table EXPECTS (the GPU test asserts it on the plans
    that ran, and each plan against its expectation): every instance of chunk_post and chunk_loglik at every padded width,
    both values of half_ops and small, one to three walk levels, the three block sizes of fin_kernel."""
    plans = [(R.expected_plan(c, p), p) for c in R.CASES for p in c.precisions]
    assert R.coverage_gaps(plans) == []
    assert len({c.name for c in R.CASES}) == len(R.CASES)
    import os
    import re
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(repo, 'vbx_amd', 'csrc', 'vbx_host_launch.hpp')).read()
    # the restated instance choice goes stale when an instance is added: both functions name 5 / 5 kernels today
    post = re.search(r'auto chunk_post_instance.*?\n}\n', text, flags=re.S).group(0)
    loglik = re.search(r'auto chunk_loglik_instance.*?\n}\n', text, flags=re.S).group(0)
    assert post.count('return chunk_post_kernel<') == 5 and loglik.count('return chunk_loglik_kernel<') == 5
