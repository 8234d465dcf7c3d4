"""Every instance the launch plan of an EM iteration can pick, held to ONE referee step at its own floor -- -m gpu.

Per case of tests/onestep_ref.py and precision:
  1. the options and the recording(s) go up, ``run(1)``: gamma, pi, Li, alpha, invL against the longdouble step from the inputs;
  2. ``run(1)`` again on the same batch, against the longdouble step from the (gamma, pi) the device returned after step 1 --
     the comparison that sees the gamma^T rho partials chunk_post leaves behind (the first iteration after an upload takes alpha
     from the stand-alone mstep_acc_kernel), fin_kernel's mode 3 and the state swap; its floor is computed from that same state;
  3. ``batch.plan`` field by field against the plan the case expects.
The bound of every quantity is K x the floor of a straightforward NumPy model in the kernel's precision -- in float64 plus two
terms the floor cannot see, derived from the referee's own magnitudes: the rounding of the per-speaker bias, coherent over a
speaker's frames (onestep_ref.coherent_terms), and the summation of the ELBO (onestep_ref.li_sum_term).  The first run of this
test, on the bare K x floor, had two misses, both fp64: gamma / pi of T = 128, S = 50 at 2.42e-14 / 1.51e-14 against 1.62e-14 /
9.0e-15 -- the same figures from the fused, unfused, scan and sequential kernels alike, alpha and invL at 0.2 x their bounds --
and the ELBO of T = 153 700 at 8.1e-16 relative against 4 u = 4.4e-16.  Both are located and the terms derived where they are
defined; none is a number read off a kernel, and with them the largest error / bound is 0.63.
A final test asserts that the plans that RAN cover every instance of chunk_post / chunk_loglik at every padded width, half_ops
and small both ways, one to three walk levels and the three block sizes of fin_kernel, and prints the largest error / bound
per precision and quantity.

The first-step referee is computed once per recording and shared by the precisions.  T = 153 700 takes its floor from the
``dot`` variant of the model alone (the sequential variant is 1.3 s a call).
"""
import json

import numpy as np
import pytest

import onestep_ref as R

pytestmark = pytest.mark.gpu

PARAMS = [(case, precision) for case in R.CASES for precision in case.precisions]
_RAN = {}                     # (case name, precision) -> the plan that ran
_RATIOS = {}                  # (precision, quantity) -> (largest error / bound, where)


@pytest.fixture(scope='module')
def ctx():
    from vbx_amd import _capi
    return _capi.Context(0)


def _open(ctx, case, precision):
    from vbx_amd import _capi
    recs = case.recs
    batch = _capi.Batch(ctx, [r.T for r in recs], [r.S for r in recs], recs[0].D, precision=precision, max_iters=2,
                        streams=case.streams)
    for name, value in case.options.items():
        if name == 'FB_ALGO':
            value = getattr(_capi, 'FB_' + value)
        batch.set_option(getattr(_capi, 'OPT_' + name), value)
    if case.stream_loads:
        batch.set_stream_loads(case.stream_loads)
    for k, rec in enumerate(recs):
        X, Phi, g0, pi0 = R.inputs(rec)
        if case.shared and k > 0:
            batch.set_recording_shared(k, 0, pi0, g0, rec.lp, rec.Fa, rec.Fb)
        else:
            batch.set_recording(k, X, Phi, pi0, g0, rec.lp, rec.Fa, rec.Fb)
    return batch


def _got(res, it):
    return R.Step(res['gamma'], res['pi'], res['Li'][it], res['alpha'], res['invL'])


@pytest.mark.parametrize('case,precision', PARAMS, ids=[f'{c.name}-{p}' for c, p in PARAMS])
def test_one_step_and_the_next_within_the_floor(ctx, case, precision):
    name = R.MODEL_DTYPE[precision]
    same = len(set(case.recs)) == 1 and len(case.recs) > 1          # copies of one recording: one referee serves all
    batch = _open(ctx, case, precision)
    try:
        batch.run(1, -np.inf)
        plan = batch.plan
        first = batch.results(pinned=False)
        batch.run(1, -np.inf)
        second = batch.results(pinned=False)
        assert batch.plan == plan and batch.streams == 1
    finally:
        batch.close()
    print(f'{case.name} {precision}: plan {plan}')
    _RAN[case.name, precision] = plan
    want = R.expected_plan(case, precision)
    assert plan == want, {k: (plan[k], want[k]) for k in want if plan[k] != want[k]}
    if same:
        for k in range(1, len(case.recs)):
            for res in (first, second):
                for q in ('gamma', 'pi', 'Li', 'alpha', 'invL'):
                    assert np.array_equal(res[k][q], res[0][q]), (k, q)
    failures = []
    for k, rec in enumerate(case.recs[:1] if same else case.recs):
        label = f'{case.name} T={rec.T} S={rec.S} D={rec.D}' + (f' Fa={rec.Fa} Fb={rec.Fb}' if case.shared else '')
        assert first[k]['n_iters'] == 1 and second[k]['n_iters'] == 2
        truth, floor = R.first_step(rec)
        truth2, floor2 = R.referee(rec, first[k]['gamma'], first[k]['pi'], dtypes=(name,))
        for it, res, t, f in ((0, first, truth, floor), (1, second, truth2, floor2)):
            try:
                R.check(_got(res[k], it), t, f, precision, f'{label} step {it + 1}', _RATIOS)
            except AssertionError as exc:
                failures.append(str(exc))
    assert not failures, '\n'.join(failures)


def test_the_plans_that_ran_cover_every_instance():
    """The closing condition: over the cases above (all of them must have run in this process)."""
    missing = [f'{c.name}-{p}' for c, p in PARAMS if (c.name, p) not in _RAN]
    assert not missing, f'cases that did not run: {missing}'
    gaps = R.coverage_gaps((plan, p) for (_, p), plan in _RAN.items())
    table = {p: {q: {'ratio': round(_RATIOS[p, q][0], 3), 'where': _RATIOS[p, q][1]} for q in R.QUANTITIES if (p, q) in _RATIOS}
             for p in R.ALL3}
    print('largest error / bound per precision and quantity:')
    print('ONESTEP_RATIOS ' + json.dumps(table))
    assert gaps == []
