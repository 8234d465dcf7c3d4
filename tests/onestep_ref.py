"""ONE iteration of the VB-HMM (VBx.py:95-104) from a given (gamma, pi) in any NumPy dtype, the floor and the bound a
kernel's one step is held to, the case table of tests/test_gpu_onestep.py and the shared assertion  --  TEST INFRASTRUCTURE.

Why one step.  The end-to-end tests compare gamma / pi / Li after 2-40 iterations with the oracle at 2e-5 ... 1e-4 (fp32) and
1e-9 ... 2e-8 (fp64): bounds that have to absorb the EM map's amplification and therefore sit 10^4 - 10^5 x
above what one iteration's arithmetic adds.  One step from a given state has no history; what it is compared with can be as
tight as the working precision allows.

``step(..., dtype)`` is the linear-domain formulation of oracle/vbx_oracle_x.py::_fb_linear_x (the transition matrix as
lp I + 1 c^T, vectors kept at scale one); the per-frame constant G of VBx.py:87 stays out of the log-likelihoods and is added
to the ELBO in longdouble.

  * dtype = longdouble      the TRUTH (tests/test_onestep_ref_host.py pins it to VBx_x in both of its forms at 1e-10).
  * dtype = float32/float64 the MODEL: the same operation written straightforwardly in the kernels' working precision, inputs
                            cast first.  Two variants, for the two products gamma^T rho and rho alpha^T: BLAS ``dot``
                            (blocked, pairwise-like summation) and ``einsum(optimize=False)`` (one sequential chain).

FLOOR of a quantity in a precision = the larger deviation of the two model variants from the truth:
    gamma, pi, invL absolute;  alpha relative to max(1, max|alpha|);  Li relative.
BOUND = min(cap, max(K floor + term, 4 u)) with u the unit round-off of the precision (results come back rounded to it; every
quantity is of magnitude <= 1 in the units above) and cap what the end-to-end tests already hold the path to: 1e-4 for fp32
and split, 2e-8 for fp64 on gamma / pi, 1e-6 relative on Li.  The split path is held to the float32 floor (DESIGN section 5
puts the two fp32 paths at the same per-iteration error).

K = 4, one value for every case, quantity and precision: two legitimate summation orders of the model differ by up to 4.2 x on
these inputs (T = 20 000, S = 4, D = 32: 4.9e-6 against 2.0e-5; everywhere else 1.0-1.1 x), a kernel is a third order, and the
floor already takes the worse of two.  K is not fitted to what any kernel gives.

TERM (float64 only; referee_terms): what the floor cannot see because both variants of the model do it alike -- the rounding of
the per-speaker bias, which enters every frame's log-likelihood (coherent_terms), and the summation of the ELBO, which the
model does in longdouble (li_sum_term).  Both are chain length x u x the referee's own magnitudes, derived where they are
defined; neither is a number read off a kernel.
"""
from __future__ import annotations

import collections

import numpy as np

EPS_TR = 1e-8                 # VBx.py:158
K = 4.0
TILE = 128                    # frames of a workgroup tile (vbx_device.hpp: kTileFrames)
QUANTITIES = ('gamma', 'pi', 'alpha', 'invL', 'Li')
UNIT = {'float32': 2.0 ** -24, 'float64': 2.0 ** -53}
MODEL_DTYPE = {'fp64': 'float64', 'fp32': 'float32', 'fp32-split': 'float32'}
CAP = {'float64': {'gamma': 2e-8, 'pi': 2e-8, 'Li': 1e-6},
       'float32': {'gamma': 1e-4, 'pi': 1e-4, 'alpha': 1e-4, 'invL': 1e-4, 'Li': 1e-6}}
# every case's floor on gamma has to lie in these ranges (tests/test_onestep_ref_host.py): below it a case is vacuous (a state
# that has hardened: any kernel passes), above it ill-conditioned
FLOOR_RANGE = {'float64': (1e-15, 1e-12), 'float32': (1e-7, 1e-4)}

Step = collections.namedtuple('Step', 'gamma pi Li alpha invL mags', defaults=(None,))


def soft_start(T, S, seed=5):
    g = np.random.default_rng(seed).gamma(1.0, size=(T, S))
    return g / g.sum(1, keepdims=True)


def _fb_linear(B, pi, lp, eps, fault=None):
    """oracle/vbx_oracle_x.py::_fb_linear_x on B = exp(lls - rowmax) -> (gamma, the frames' log scales, entered).
    ``fault`` plants a structural error (tests/test_onestep_ref_host.py)."""
    dt = B.dtype
    T, S = B.shape
    c = (1 - lp) * pi + eps
    ahat = np.empty_like(B)
    lsc = np.empty(T, dtype=dt)
    a = B[0] * (pi + eps)
    s = a.sum()
    ahat[0] = a / s
    lsc[0] = np.log(s)
    for t in range(1, T):
        prev = ahat[t - 1]
        a = B[t] * (lp * prev + c * prev.sum())
        s = a.sum()
        ahat[t] = a / s
        lsc[t] = np.log(s)
    bhat = np.empty_like(B)
    bhat[-1] = 1
    for t in range(T - 2, -1, -1):
        e = B[t + 1] * bhat[t + 1]
        nb = lp * e + np.dot(c, e)
        bhat[t] = nb / nb.max()
    if fault == 'tile_end':
        # the last frame of every 128-frame tile but the recording's last takes the backward vector a tile's re-run starts
        # from at the END OF THE RECORDING (ones) instead of the one handed over by the next tile
        bhat[TILE - 1:T - 1:TILE] = 1
    g = ahat * bhat
    g /= g.sum(axis=1, keepdims=True)
    prev = ahat[:-1]
    entered = (g[1:] / (lp * prev + c * prev.sum(axis=1, keepdims=True))).sum(axis=0)
    return g, lsc, entered


def step(X, Phi, pi, gamma, lp, Fa, Fb, dtype=np.longdouble, seq=False, fault=None):
    """One iteration from (gamma, pi) in ``dtype`` -> Step(gamma', pi', ELBO, alpha, invL).  ``seq``: the two large products as
    one sequential chain each (einsum) instead of BLAS.  ``fault`` in (None, 'rho127', 'no_eps', 'tile_end')."""
    dt = np.dtype(dtype)
    ld = np.longdouble
    Xd, Phid = np.asarray(X, dtype=dt), np.asarray(Phi, dtype=dt)
    pi, gamma = np.asarray(pi, dtype=dt), np.asarray(gamma, dtype=dt)
    lp, fa, fb, half = dt.type(lp), dt.type(Fa), dt.type(Fb), dt.type(0.5)
    eps = dt.type(0.0 if fault == 'no_eps' else EPS_TR)
    D = Xd.shape[1]
    rho = Xd * np.sqrt(Phid)                                                                 # VBx.py:88-89
    if fault == 'rho127':
        rho[127] *= dt.type(1 + 2.0 ** -20)
    invL = 1 / (1 + fa / fb * gamma.sum(axis=0, keepdims=True).T * Phid)                     # VBx.py:95
    gr = np.einsum('ts,td->sd', gamma, rho, optimize=False) if seq else gamma.T.dot(rho)
    alpha = fa / fb * invL * gr                                                              # VBx.py:96
    ra = np.einsum('td,sd->ts', rho, alpha, optimize=False) if seq else rho.dot(alpha.T)
    lls = fa * (ra - half * (invL + alpha ** 2).dot(Phid))                                   # VBx.py:97 without G
    m = lls.max(axis=1)
    g, lsc, ent = _fb_linear(np.exp(lls - m[:, None]), pi, lp, eps, fault)                   # VBx.py:99
    new_pi = g[0] + (1 - lp) * pi * ent                                                      # VBx.py:101-103
    Xl = np.asarray(X, dtype=ld)
    G = -ld(0.5) * (np.sum(Xl * Xl, axis=1) + D * np.log(2 * ld(np.pi)))                     # VBx.py:87
    elbo = (ld(lsc.sum() + m.sum()) + ld(fa) * G.sum()
            + ld(fb * half * np.sum(np.log(invL) - invL - alpha ** 2 + 1)))                  # VBx.py:100
    # what the ELBO is a sum of, in absolute value over the value: the frames' log scales, row maxima and Fa G_t, the model's
    # S x D terms (the referee's own magnitudes for the summation term of the bound on Li)
    model_terms = np.abs(np.asarray(np.log(invL) - invL - alpha ** 2 + 1, dtype=ld)).sum()
    terms = ld(np.abs(lsc).sum()) + ld(np.abs(m).sum()) + ld(fa) * np.abs(G).sum() + ld(fb * half) * model_terms
    mags = {'Li': float(terms / abs(elbo)), 'Li_abs': float(abs(elbo)), 'Li_terms': 3 * Xd.shape[0] + alpha.size,
            'lls': np.asarray(lls, dtype=np.float64), 'pi': np.asarray(pi, dtype=np.float64), 'lp': float(lp), 'D': D,
            'bias_abs': np.asarray(fa * half * np.abs((invL + alpha ** 2) * Phid).sum(axis=1), dtype=np.float64)}
    return Step(g, new_pi / new_pi.sum(), elbo, alpha, invL, mags)                           # VBx.py:104


def deviation(got, truth):
    """The five deviations of ``got`` (a Step, or a dict with the same keys) from ``truth`` in the units of the floor."""
    if isinstance(got, dict):
        got = Step(*(got[k] for k in Step._fields[:5]))
    ld = np.longdouble
    d = lambda a, b: float(np.max(np.abs(np.asarray(a, dtype=ld) - np.asarray(b, dtype=ld))))
    return {'gamma': d(got.gamma, truth.gamma), 'pi': d(got.pi, truth.pi),
            'alpha': d(got.alpha, truth.alpha) / max(1.0, float(np.max(np.abs(truth.alpha)))),
            'invL': d(got.invL, truth.invL),
            'Li': float(abs(ld(got.Li) - ld(truth.Li)) / abs(ld(truth.Li)))}


def floors(X, Phi, pi, gamma, lp, Fa, Fb, truth, dtypes=('float32', 'float64'), variants=(False, True)):
    """{dtype name: {quantity: floor}} of this state: the larger deviation of the model's variants from ``truth``."""
    out = {}
    for name in dtypes:
        dt = np.dtype(name)
        devs = [deviation(step(np.asarray(X).astype(dt), np.asarray(Phi).astype(dt), pi, gamma, lp, Fa, Fb, dt, seq), truth)
                for seq in variants]
        out[name] = {q: max(d[q] for d in devs) for q in QUANTITIES}
    return out


def _estep_batch(lls, offsets, pi, lp):
    """The E-step of ``step`` in float64 for P per-speaker offsets at once: lls [T][S], offsets [P][S] (added to every frame's
    log-likelihoods) -> (gamma [P][T][S], new pi [P][S])."""
    T, S = lls.shape
    m = lls.max(axis=1)
    B = np.exp(lls - m[:, None])[None] * np.exp(offsets)[:, None, :]
    c = (1 - lp) * pi + EPS_TR
    ahat = np.empty_like(B)
    a = B[:, 0] * (pi + EPS_TR)
    ahat[:, 0] = a / a.sum(axis=1, keepdims=True)
    for t in range(1, T):
        prev = ahat[:, t - 1]
        a = B[:, t] * (lp * prev + c * prev.sum(axis=1, keepdims=True))
        ahat[:, t] = a / a.sum(axis=1, keepdims=True)
    g = np.empty_like(B)
    x = np.ones_like(B[:, 0])
    g[:, -1] = ahat[:, -1]
    for t in range(T - 2, -1, -1):
        e = B[:, t + 1] * x
        x = lp * e + (e * c).sum(axis=1, keepdims=True)
        x /= x.max(axis=1, keepdims=True)
        g[:, t] = ahat[:, t] * x
    g /= g.sum(axis=2, keepdims=True)
    prev = ahat[:, :-1]
    ent = (g[:, 1:] / (lp * prev + c * prev.sum(axis=2, keepdims=True))).sum(axis=1)
    npi = g[:, 0] + (1 - lp) * pi * ent
    return g, npi / npi.sum(axis=1, keepdims=True)


SENS_STEP = 1e-6              # finite-difference step of the sensitivities below (they are linear far beyond the offsets meant)
SENS_CELLS = 4e6              # offsets x frames x speakers taken through the E-step at once (32 MB an array)
SENS_MAX_WORK = 2e7           # S x T x S above which the sensitivities give way to the chain-length bound (S = 1030: 12 s)


def coherent_terms(truth):
    """What a rounding error of the per-speaker BIAS may add to the deviations, from the referee's own numbers.

    l[t][s] = Fa (rho_t . alpha_s + bias_s) with bias_s = -1/2 sum_d (invL + alpha^2)[s][d] Phi[d] (VBx.py:97).  The two
    variants of the model order the two large PRODUCTS differently and compute the bias alike, so the floor does not see what
    another order of that D-term sum does -- and its error is no noise: the same offset e_s enters EVERY frame's
    log-likelihood of speaker s and accumulates along the chain.  (Found on T = 128, S = 50 in fp64: the fused kernels, the
    unfused ones, the scan path and the sequential walk all came out 2.42e-14 from the truth on the same ten frames, 6 x the
    floor, with alpha and invL at 0.2 x theirs; the E-step of the referee fed with the device's own alpha and invL stayed as
    far away.  A deviation every family shares comes from what they share -- fin_kernel's bias -- and a bias two roundings of
    its magnitude off explains the figure.)

    |e_s| <= c u Fa 1/2 sum_d |(invL + alpha^2) Phi|, c = ceil(log2 D) + ceil(D / 256) + 4: each of the D terms is rounded
    three times (alpha^2, +, x Phi) and summed as fin_kernel sums it -- d strided over the 256 threads of its block, then a
    tree: at most ceil(D / 256) - 1 + ceil(log2 min(D, 256)) additions on a term's way (Higham, Accuracy and Stability of
    Numerical Algorithms, section 4.2) -- and then x 1/2, the addition to the product and x Fa.  u = 2^-53 in every precision:
    fin_kernel sums the bias in f64 and hands the fp32 paths what its rounding to f32 lost (BatchView::bias_lo), which is why
    the float32 bounds take no such term (it is 2^-29 of theirs).
    To first order the offsets move gamma[t][s] by sum_s' J[t][s][s'] e_s' with J = d gamma[t][s] / d e_s', so by at most
    sum_s' |J[t][s][s']| |e_s'|; J is taken from the referee's E-step by finite differences, one speaker at a time (float64,
    step 1e-6: the map is smooth and the offsets meant are 1e-14).  The same for pi.  Beyond S^2 T = 2e7 (S = 1030, where that
    pass takes 12 s) the chain-length bound stands in: J[t][s][s'] = sum_t' Cov(z_t = s, z_t' = s') and |Cov| <= P(z_t' = s'),
    so sum_s' |J| |e_s'| <= T max |e|; twice that for pi (numerator and normaliser).
    The log-likelihood moves by sum_s N_s e_s to first order (N_s = sum_t gamma[t][s]), at most T max |e|.
    alpha and invL do not depend on the bias."""
    mg = truth.mags
    lls, pi, lp, D = mg['lls'], mg['pi'], mg['lp'], mg['D']
    T, S = lls.shape
    chain = int(np.ceil(np.log2(max(D, 2)))) + -(-D // 256) + 4
    e = chain * UNIT['float64'] * mg['bias_abs']
    li = T * float(e.max()) / mg['Li_abs']
    if S * T * S > SENS_MAX_WORK:
        return {'gamma': T * float(e.max()), 'pi': 2 * T * float(e.max()), 'alpha': 0.0, 'invL': 0.0, 'Li': li}
    g0, p0 = _estep_batch(lls, np.zeros((1, S)), pi, lp)
    dg, dp = np.zeros((T, S)), np.zeros(S)
    per = max(1, int(SENS_CELLS // (T * S)))
    for s0 in range(0, S, per):
        idx = np.arange(s0, min(S, s0 + per))
        off = np.zeros((len(idx), S))
        off[np.arange(len(idx)), idx] = SENS_STEP
        g, p = _estep_batch(lls, off, pi, lp)
        dg += (np.abs(g - g0) / SENS_STEP * e[idx, None, None]).sum(axis=0)
        dp += (np.abs(p - p0) / SENS_STEP * e[idx, None]).sum(axis=0)
    return {'gamma': float(dg.max()), 'pi': float(dp.max()), 'alpha': 0.0, 'invL': 0.0, 'Li': li}


def li_sum_term(truth):
    """What the summation of the ELBO may add to its relative error.  Li is ONE sum of 3 T + S D terms (per frame the log scale,
    the row maximum and Fa G_t; the model's S x D terms), reduced in f64 in every precision.  The model sums G in longdouble,
    so its floor knows nothing of that reduction.  The kernels reduce in trees (a tile's frames in one block_sum, a
    recording's tiles strided over the threads of fin_kernel -- at most ceil(tiles / 256) terms in sequence -- and one
    block_sum): a term passes through at most ceil(log2(terms)) + ceil(tiles / 256) additions, and 8 more roundings for the
    products and logarithms that make the terms and the final three-term sum.  Higham section 4.2: error <= that many u times
    sum |terms|, here relative to |Li|."""
    mg = truth.mags
    T = mg['lls'].shape[0]
    chain = int(np.ceil(np.log2(mg['Li_terms']))) + -(-(-(-T // TILE)) // 256) + 8
    return chain * UNIT['float64'] * mg['Li']


def referee_terms(truth):
    """{quantity: term} the bound gains beside K x floor, computed from the truth alone; cached on it."""
    if 'terms' not in truth.mags:
        t = coherent_terms(truth)
        t['Li'] += li_sum_term(truth)
        truth.mags['terms'] = t
    return truth.mags['terms']


def bound(floor, dtype_name, terms=None):
    """{quantity: bound} from the floors of one precision and the referee-derived terms (referee_terms)."""
    u = UNIT[dtype_name]
    terms = terms or {}
    return {q: min(CAP[dtype_name].get(q, np.inf), max(K * floor[q] + terms.get(q, 0.0), 4 * u)) for q in QUANTITIES}


def check(got, truth, floor, precision, label, ratios=None):
    """The shared assertion: every quantity of ``got`` within the bound of ``precision`` ('fp64' | 'fp32' | 'fp32-split') around
    ``truth``.  Prints error / bound per quantity before it asserts; ``ratios`` (a dict) collects the largest ratio per
    (precision, quantity) with the label that gave it."""
    name = MODEL_DTYPE[precision]
    dev, bnd = deviation(got, truth), bound(floor[name], name, referee_terms(truth) if name == 'float64' else None)
    ratio = {q: dev[q] / bnd[q] for q in QUANTITIES}
    print(f'{label} {precision}: ' + '  '.join(f'{q} {dev[q]:.2e}/{bnd[q]:.2e}={ratio[q]:.2f}' for q in QUANTITIES))
    if ratios is not None:
        for q in QUANTITIES:
            if ratio[q] > ratios.get((precision, q), (-1.0, ''))[0]:
                ratios[precision, q] = (ratio[q], label)
    bad = {q: (dev[q], bnd[q]) for q in QUANTITIES if not dev[q] <= bnd[q]}
    assert not bad, f'{label} {precision}: beyond the bound: {bad}'
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------
# recordings and their referee, computed once per process and never changed
# ---------------------------------------------------------------------------------------------------------------------------
Rec = collections.namedtuple('Rec', 'T S D kappa lp Fa Fb', defaults=(32, 0.05, 0.9, 0.3, 17.0))
BIG_T = 100000                # from here the floor takes the ``dot`` variant only (the sequential einsum is 1.3 s a call)

_INPUTS, _FIRST = {}, {}


def inputs(rec):
    """(X, Phi, gamma0, pi0) of a recording: make_recording(seed = T + S), the soft random start, uniform priors."""
    key = rec[:4]
    if key not in _INPUTS:
        from vbx_amd.synth import make_recording
        X, Phi, _ = make_recording(rec.T, rec.S, D=rec.D, seed=rec.T + rec.S, kappa=rec.kappa)
        g0, pi0 = soft_start(rec.T, rec.S), np.ones(rec.S) / rec.S
        for a in (X, Phi, g0, pi0):
            a.setflags(write=False)
        _INPUTS[key] = (X, Phi, g0, pi0)
    return _INPUTS[key]


def referee(rec, gamma, pi, dtypes=('float32', 'float64')):
    """(truth, floors) of one step of ``rec`` from (gamma, pi)."""
    X, Phi = inputs(rec)[:2]
    truth = step(X, Phi, pi, gamma, rec.lp, rec.Fa, rec.Fb)
    variants = (False,) if rec.T >= BIG_T else (False, True)
    return truth, floors(X, Phi, pi, gamma, rec.lp, rec.Fa, rec.Fb, truth, dtypes=dtypes, variants=variants)


def first_step(rec):
    """(truth, floors) of the first step of ``rec`` from its inputs, cached."""
    if rec not in _FIRST:
        _, _, g0, pi0 = inputs(rec)
        _FIRST[rec] = referee(rec, g0, pi0)
    return _FIRST[rec]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_onestep.py.  A case: recordings, options, precisions, and the launch plan it must run under
# (Batch.plan) -- per precision where the precisions differ.  Everything a case does not state is DEFAULT_PLAN.
# ---------------------------------------------------------------------------------------------------------------------------
EDGE_T = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 300, 1100)
# exempt from the lower ends of FLOOR_RANGE: too few frames for rounding to add up (f64 4e-16 ... 5e-15, f32 1.4e-7 ... 2.8e-7)
EXEMPT_T = (1, 2, 3, 129)
# kappa (and loopProb) per edge recording: D = 32, kappa = 0.05, loopProb = 0.9 unless the float64 floor on gamma fell below
# FLOOR_RANGE with them (short recordings from a soft start stay near uniform: nothing for rounding to act on)
EDGE_PARAMS = {10: {64: (0.2, 0.9), 65: (0.1, 0.9), 127: (0.5, 0.9), 128: (0.5, 0.9), 191: (0.2, 0.9)},
               30: {},
               50: {63: (0.3, 0.5), 64: (0.3, 0.5), 65: (0.5, 0.9), 127: (0.5, 0.9), 300: (0.5, 0.9)}}
ALL3 = ('fp64', 'fp32', 'fp32-split')
EXACT = ('fp64', 'fp32')
SPLIT = ('fp32-split',)

Case = collections.namedtuple('Case', 'name recs options precisions plan stream_loads shared streams',
                              defaults=(None, False, 0))
# the plan of a flat walk on the fused kernels in a batch that does not fill the chip; `split` follows the precision
DEFAULT_PLAN = dict(fused_post=True, fused_loglik=True, half_ops=True, stream=False, small=True, lat=True, fold=False,
                    walk_levels=1, fin_threads=256, use_chunked=True, sgroup=1, sgroup2=1)


def edge_recs(S):
    return [Rec(T, S, 32, *EDGE_PARAMS[S].get(T, (0.05, 0.9))) for T in EDGE_T]


def _cases():
    chunked = {'FB_ALGO': 'CHUNKED'}
    out = []
    add = lambda name, recs, options, precisions, plan, **kw: out.append(Case(name, recs, options, precisions, plan, **kw))
    # tile and half-tile edges: one ragged batch per padded width, half-tile operators on and off
    for S, Sp in ((10, 16), (30, 32), (50, 64)):
        for st in (1, 2):
            add(f'edges-S{S}-halves{"on" if st == 1 else "off"}', edge_recs(S), dict(chunked, SPLIT_TILES=st), ALL3,
                dict(Sp=Sp, half_ops=st == 1, lat=Sp <= 32))
    # feature widths: LAT on (Dp <= 128), off (Dp = 160: the second slice of the staged model), padded, two K-blocks
    for D in (128, 160, 100, 40):
        add(f'width-D{D}', [Rec(777, 10, D, 0.05, 0.95)], chunked, ALL3, dict(Sp=16, lat=D != 160))
    add('width-D160-Sp32', [Rec(777, 30, 160, 0.05, 0.95)], chunked, ALL3, dict(Sp=32, lat=False))
    # the boundary walk over 9 chunks (T = 1100): a ragged last group
    r16, r32, r64 = [Rec(1100, 10)], [Rec(1100, 30)], [Rec(1100, 50)]
    add('walk-flat-Sp32', r32, dict(chunked, SCAN_GROUP=1), ALL3, dict(Sp=32))
    add('walk-2-fold-Sp16', r16, dict(chunked, SCAN_GROUP=4), ALL3, dict(Sp=16, walk_levels=2, sgroup=4, fold=True))
    add('walk-2-fold-Sp32', r32, dict(chunked, SCAN_GROUP=4), ALL3, dict(Sp=32, walk_levels=2, sgroup=4, fold=True))
    add('walk-2-Sp64', r64, dict(chunked, SCAN_GROUP=4), ALL3, dict(Sp=64, walk_levels=2, sgroup=4, lat=False))
    add('walk-2-group6-Sp32', [Rec(1700, 30)], dict(chunked, SCAN_GROUP=6), ALL3, dict(Sp=32, walk_levels=2, sgroup=6))
    add('walk-2-stream-Sp16', r16, dict(chunked, SCAN_GROUP=4), SPLIT, dict(Sp=16, walk_levels=2, sgroup=4, stream=True),
        stream_loads='on')
    add('walk-2-stream-Sp32', r32, dict(chunked, SCAN_GROUP=4), SPLIT, dict(Sp=32, walk_levels=2, sgroup=4, stream=True),
        stream_loads='on')
    three = dict(chunked, SCAN_GROUP=4, SCAN_GROUP2=2)
    add('walk-3-fold-Sp16', r16, three, ALL3, dict(Sp=16, walk_levels=3, sgroup=4, sgroup2=2, fold=True))
    add('walk-3-fold-Sp32', r32, three, ALL3, dict(Sp=32, walk_levels=3, sgroup=4, sgroup2=2, fold=True))
    add('walk-3-Sp64', r64, three, ALL3, dict(Sp=64, walk_levels=3, sgroup=4, sgroup2=2, lat=False))
    # split with non-temporal loads: every padded width, LAT on and off
    for S, Sp in ((10, 16), (30, 32)):
        for D in (128, 160):
            add(f'stream-Sp{Sp}-D{D}', [Rec(777, S, D, 0.05, 0.95)], chunked, SPLIT, dict(Sp=Sp, stream=True, lat=D == 128),
                stream_loads='on')
    add('stream-Sp64-D128', [Rec(777, 50, 128, 0.05, 0.95)], chunked, SPLIT, dict(Sp=64, stream=True, lat=False),
        stream_loads='on')
    # the block sizes of fin_kernel (256: everything above); the automatic walk of a long recording
    add('fin-512', [Rec(10300, 10)], {}, ALL3, dict(Sp=16, fin_threads=512, walk_levels=2, sgroup=4, fold=True))
    add('fin-1024', [Rec(153700, 4, 32, 0.05, 0.99)], {}, ALL3,
        dict(Sp=16, fin_threads=1024, walk_levels=3, sgroup=7, sgroup2=7, fold=True))
    # a batch that fills the chip: 17 x 122 = 2074 tiles on one stream -- no small-batch instance
    add('fills-chip', [Rec(15500, 4, 32, 0.05, 0.99)] * 17, {}, ALL3,
        dict(Sp=16, small=False, lat=False, fin_threads=512), streams=1)
    # three (Fa, Fb, loopProb) points on one rho: the tile order of a sharing group and its -1 blocks
    add('shared-rho', [Rec(777, 10, 128, 0.05, 0.95), Rec(777, 10, 128, 0.05, 0.9, 0.2, 6.0),
                       Rec(777, 10, 128, 0.05, 0.8, 0.4, 64.0)], chunked, ALL3, dict(Sp=16), shared=True, streams=1)
    # the other kernel families, one step each
    nofuse = dict(fused_post=False, fused_loglik=False, half_ops=False)
    add('fuse-0', r32, dict(chunked, FUSE=0), EXACT, dict(nofuse, Sp=32))
    add('fuse-1', r32, dict(chunked, FUSE=1), EXACT, dict(Sp=32, fused_loglik=False, half_ops=False))
    add('sequential-S30', r32, {'FB_ALGO': 'SEQUENTIAL'}, EXACT, dict(nofuse, Sp=32, use_chunked=False))
    add('sequential-S130', [Rec(1100, 130)], {'FB_ALGO': 'SEQUENTIAL'}, EXACT, dict(nofuse, Sp=256, use_chunked=False, lat=False))
    for S, Sp in ((70, 128), (130, 256)):
        add(f'wide-flat-Sp{Sp}', [Rec(1100, S)], chunked, EXACT, dict(nofuse, Sp=Sp, lat=False))
        add(f'wide-groups-Sp{Sp}', [Rec(1100, S)], dict(chunked, SCAN_GROUP=4), EXACT,
            dict(nofuse, Sp=Sp, lat=False, walk_levels=2, sgroup=4))
    add('big-S1030', [Rec(300, 1030, 64, 0.05, 0.9)], {}, EXACT,
        dict(nofuse, Sp=2048, lat=False, use_chunked=False, fin_threads=1024))
    return out


CASES = _cases()


def expected_plan(case, precision):
    p = dict(DEFAULT_PLAN, **case.plan)
    p['split'] = precision == 'fp32-split'
    return p


def instances(plan, precision):
    """The names of the chunk_post / chunk_loglik instances a plan launches (chunk_post_instance / chunk_loglik_instance of
    vbx_host_launch.hpp, restated), as 'post:<variant>:Sp<n>' -- the empty list off the fused kernels."""
    r = {'fp64': 'f64', 'fp32': 'f32', 'fp32-split': 'f32'}[precision]
    sp, out = plan['Sp'], []
    if plan['fused_post']:
        if plan['split']:
            v = 'split-fold' if plan['fold'] and sp <= 32 else 'split-stream' if plan['stream'] else 'split'
        else:
            v = f'{r}-fold' if plan['fold'] and sp <= 32 else r
        out.append(f'post:{v}:Sp{sp}')
    if plan['fused_loglik']:
        if plan['split']:
            v = 'split' + ('-lat' if plan['lat'] and sp <= 32 else '') + ('-stream' if plan['stream'] else '')
        else:
            v = r
        out.append(f'loglik:{v}:Sp{sp}')
    return out


def required_coverage():
    """Every instance chunk_post_instance and chunk_loglik_instance can return, at each Sp it exists for."""
    need = set()
    for sp in (16, 32, 64):
        for v in ('split-stream', 'split', 'f32', 'f64'):
            need |= {f'post:{v}:Sp{sp}', f'loglik:{v}:Sp{sp}'}
        if sp <= 32:
            need |= {f'post:{v}:Sp{sp}' for v in ('split-fold', 'f32-fold', 'f64-fold')}
            need |= {f'loglik:{v}:Sp{sp}' for v in ('split-lat', 'split-lat-stream')}
    return need


def coverage_gaps(plans):
    """``plans``: iterable of (plan dict, precision) -> what the closing condition still misses (empty: covered)."""
    plans = list(plans)
    have = set()
    for p, prec in plans:
        have |= set(instances(p, prec))
    gaps = sorted(required_coverage() - have)
    for field, values in (('half_ops', (False, True)), ('small', (False, True)), ('walk_levels', (1, 2, 3)),
                          ('fin_threads', (256, 512, 1024))):
        gaps += [f'{field}={v}' for v in values if not any(p[field] == v for p, _ in plans)]
    return gaps
