"""Viterbi decoding on the device (-m gpu): vbx_viterbi, vbx_batch_get_path and ``vbhmm --decode viterbi`` against the
longdouble referee of tests/viterbi_ref.py.

Exact comparison is fair where no decision of the recursion is close to a tie: every random case asserts that the referee's
smallest decision margin exceeds 1e-7 (five orders above float64 rounding at these magnitudes) -- a seed that violates it fails
loudly, none is left out -- and then asks for the identical path, and for logp within 4 T 2^-53 (max|lls| + 18.5): four
roundings per frame on values no larger than the frame's log-likelihood plus |log eps|.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import tune_util as tu
import viterbi_ref as vr

pytestmark = pytest.mark.gpu

# every instance of k = ceil(S / 64) in {1, 2, 4, 8, 16} and both sides of each lane-count edge
STATES = [1, 2, 3, 63, 64, 65, 128, 129, 513, 1024]
# both sides of the back-trace block (64) and of the look-ahead ring: a slot holds 16 / k frames from frame 1 on, three slots
# make a round -- T - 1 = 16 and 48 are edges of both for every k
FRAMES = [1, 2, 16, 17, 18, 48, 49, 50, 63, 64, 65, 129, 1000]
LOOPS = [0.5, 0.9, 0.99]
MARGIN = 1e-7
GUARD, SENTINEL = 32, -0x5A5A5A5B


def case_seed(S, T, i):
    return 1000003 * S + 101 * T + i


def logp_bound(T, lls):
    return 4.0 * T * 2.0 ** -53 * (float(np.abs(lls).max()) + 18.5)


@pytest.fixture(scope='module')
def ctx():
    from vbx_amd import _capi
    return _capi.default_context(0)


def decode(ctx, lls, pi, lp, ip=None):
    """vbx_viterbi into the interior of an over-allocated array: (path, logp), the guard bands checked."""
    import ctypes as C
    lls = np.ascontiguousarray(lls, dtype=np.float64)
    pi = np.ascontiguousarray(pi, dtype=np.float64)
    ip = None if ip is None else np.ascontiguousarray(ip, dtype=np.float64)
    T, S = lls.shape
    buf = np.full(T + 2 * GUARD, SENTINEL, dtype=np.int32)
    inner = buf[GUARD:GUARD + T]
    logp = C.c_double()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ctx.check(ctx._lib.vbx_viterbi(ctx._h, T, S, ptr(lls), ptr(pi), ptr(ip), float(lp), ptr(inner), C.byref(logp)), 'vbx_viterbi')
    assert np.all(buf[:GUARD] == SENTINEL) and np.all(buf[GUARD + T:] == SENTINEL), 'guard band written'
    return inner.copy(), logp.value


@pytest.mark.parametrize('T', FRAMES)
@pytest.mark.parametrize('S', STATES)
def test_path_equals_the_referees_and_logp_is_within_four_roundings_per_frame(S, T, ctx):
    for i, lp in enumerate(LOOPS):
        lls, pi = vr.draw(case_seed(S, T, i), T, S)
        want, want_logp, margin = vr.structured(lls, lp, pi)
        print(f'S={S} T={T} loopProb={lp}: margin {float(margin):.3e}')
        assert margin > MARGIN, (S, T, lp, float(margin))
        got, logp = decode(ctx, lls, pi, lp)
        assert np.array_equal(got, want), (S, T, lp, int(np.argmax(got != want)))
        err, bound = abs(float(vr.LD(logp) - want_logp)), logp_bound(T, lls)
        print(f'    |logp - referee| = {err:.3e}, bound {bound:.3e}')
        assert err <= bound, (S, T, lp, err, bound)


def test_python_entry_returns_int32_path_and_logp(ctx):
    from vbx_amd.VBx import viterbi
    lls, pi = vr.draw(5, 129, 7)
    want, want_logp, _ = vr.structured(lls, 0.9, pi)
    path, logp = viterbi(lls, 0.9, pi)
    assert path.dtype == np.int32 and path.shape == (129,) and np.array_equal(path, want)
    assert abs(float(logp) - float(want_logp)) <= logp_bound(129, lls)


# ---- crafted cases ---------------------------------------------------------------------------------------------------
LOG_EPS = float(np.log(1e-8))


def jump_case(bonus):
    """loopProb = 1: a change of state costs log eps = -18.42, staying log(1 + eps).  20 frames in which state 0 is ahead by 1
    each, then 20 in which state 1 collects ``bonus`` in all: all-0 scores 20, all-1 ``bonus``, the one jump at frame 20
    20 + bonus + log eps -- the best of the three iff bonus > |log eps|."""
    lls = np.zeros((40, 2))
    lls[:20, 0] = 1.0
    lls[20:, 1] = bonus / 20.0
    return lls, np.array([0.5, 0.5])


def test_loop_probability_one_jumps_through_log_eps_only_when_it_pays(ctx):
    for bonus, jumps in ((-LOG_EPS + 0.5, True), (-LOG_EPS - 0.5, False)):
        lls, pi = jump_case(bonus)
        want, want_logp, margin = vr.structured(lls, 1.0, pi)
        assert margin > MARGIN
        assert np.array_equal(want, np.r_[np.zeros(20, int), np.full(20, 1 if jumps else 0)]), (bonus, want)
        got, logp = decode(ctx, lls, pi, 1.0)
        assert np.array_equal(got, want), (bonus, got)
        assert abs(float(vr.LD(logp) - want_logp)) <= logp_bound(len(lls), lls)
        d_path, d_logp = vr.dense(lls, 1.0, pi)
        assert np.array_equal(d_path, want) and abs(float(d_logp - want_logp)) < 1e-12


def test_loop_probability_zero(ctx):
    lls, pi = vr.draw(11, 200, 5)
    # (stay_j = move_j: the best state's own "stayed or entered" is a tie by construction and the same predecessor either way)
    want, want_logp, margin = vr.structured(lls, 0.0, pi, own_state=False)
    assert margin > MARGIN
    got, logp = decode(ctx, lls, pi, 0.0)
    assert np.array_equal(got, want) and abs(float(vr.LD(logp) - want_logp)) <= logp_bound(200, lls)


def test_exact_zeros_in_pi_and_an_ip_of_its_own(ctx):
    lls, pi = vr.draw(12, 150, 70)
    pi[::3] = 0.0
    pi /= pi.sum()
    ip = np.random.default_rng(13).dirichlet(np.ones(70))
    ip[1::4] = 0.0
    want, want_logp, margin = vr.structured(lls, 0.9, pi, ip)
    assert margin > MARGIN
    got, logp = decode(ctx, lls, pi, 0.9, ip)
    assert np.array_equal(got, want) and abs(float(vr.LD(logp) - want_logp)) <= logp_bound(150, lls)
    # an ip that decides the path: all of it on one state, likelihoods too flat to pay log eps for another start
    flat, _ = vr.draw(16, 3, 70, sigma=1.0)
    start = np.zeros(70)
    start[5] = 1.0
    want2, _, margin2 = vr.structured(flat, 0.99, pi, start)
    assert margin2 > MARGIN and want2[0] == 5 and vr.structured(flat, 0.99, pi)[0][0] != 5
    assert np.array_equal(decode(ctx, flat, pi, 0.99, start)[0], want2)


@pytest.mark.parametrize('S', [1, 3, 64, 65, 1024])
def test_all_equal_likelihoods_give_the_all_zero_path(S, ctx):
    for T in (1, 2, 65, 200):
        got, logp = decode(ctx, np.full((T, S), -2.5), np.full(S, 1.0 / S), 0.9)
        assert not got.any(), (S, T)
        want = vr.score(np.zeros(T, int), np.full((T, S), -2.5), 0.9, np.full(S, 1.0 / S))
        assert abs(float(vr.LD(logp) - want)) <= logp_bound(T, np.full((1, 1), 2.5))


def test_a_column_of_minus_infinity_is_never_on_the_path(ctx):
    lls, pi = vr.draw(14, 130, 66)
    lls[:, 65] = -np.inf
    lls[:, 2] = -np.inf
    want, want_logp, margin = vr.structured(lls, 0.9, pi)
    assert margin > MARGIN and 65 not in want and 2 not in want
    got, logp = decode(ctx, lls, pi, 0.9)
    finite = np.where(np.isfinite(lls), lls, 0.0)
    assert np.array_equal(got, want) and abs(float(vr.LD(logp) - want_logp)) <= logp_bound(130, finite)


def test_two_runs_give_identical_bits(ctx):
    lls, pi = vr.draw(15, 1000, 129)
    a, la = decode(ctx, lls, pi, 0.9)
    b, lb = decode(ctx, lls, pi, 0.9)
    assert np.array_equal(a, b) and np.float64(la).tobytes() == np.float64(lb).tobytes()


def test_every_refusal_returns_its_code_and_a_message(ctx):
    import ctypes as C
    from vbx_amd import _capi
    lib, h = ctx._lib, ctx._h
    lls, pi = np.zeros((4, 3)), np.full(3, 1.0 / 3)
    path = np.zeros(4, dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(T=4, S=3, lls_=lls, pi_=pi, lp=0.9):
        rc = lib.vbx_viterbi(h, T, S, ptr(lls_), ptr(pi_), None, float(lp), ptr(path), None)
        return rc, lib.vbx_last_error(h).decode()
    INVALID, UNSUPPORTED, STATE = -1, -2, -5
    for kw in (dict(lls_=None), dict(pi_=None), dict(T=0), dict(S=0), dict(T=-1), dict(lp=-0.01), dict(lp=1.01), dict(lp=float('nan'))):
        rc, msg = call(**kw)
        assert rc == INVALID and 'vbx_viterbi' in msg, (kw, rc, msg)
    rc, msg = call(S=1025, lls_=np.zeros((4, 1025)), pi_=np.full(1025, 1.0 / 1025))
    assert rc == UNSUPPORTED and '1025' in msg, (rc, msg)
    assert call()[0] == 0
    # the batch entry: before a run, and a recording index out of range
    batch = _capi.Batch(ctx, [5], [2], 4, precision='fp64', max_iters=2)
    try:
        first = np.zeros(5, dtype=np.int32)
        rng = np.random.default_rng(1)
        g0 = rng.dirichlet(np.ones(2), size=5)
        batch.set_recording(0, rng.normal(size=(5, 4)), np.ones(4), np.full(2, 0.5), g0, 0.9, 1.0, 1.0)
        rc = lib.vbx_batch_get_path(batch._h, 0, ptr(first), None)
        assert rc == STATE and 'not run' in lib.vbx_last_error(h).decode(), rc
        for bad in (-1, 1):
            rc = lib.vbx_batch_get_path(batch._h, bad, ptr(first), None)
            assert rc == INVALID and 'out of range' in lib.vbx_last_error(h).decode(), (bad, rc)
        batch.run(2, -1e300)
        for bad in (-1, 1):
            rc = lib.vbx_batch_get_path(batch._h, bad, ptr(first), None)
            assert rc == INVALID and 'out of range' in lib.vbx_last_error(h).decode(), (bad, rc)
        assert lib.vbx_batch_get_path(batch._h, 0, ptr(first), None) == 0
    finally:
        batch.close()


# ---- batch level -----------------------------------------------------------------------------------------------------
# (T, S, seed) of the recordings; D = 32 keeps the kernels of the iteration what they are at any D and the uploads small
D_BATCH = 32
HYPER = dict(loopProb=0.9, Fa=0.3, Fb=17.0)
N_ITERS = 3                                                   # epsilon = -1e300: the ELBO test never stops a run
BATCHES = {'three-in-one': [(65, 3, 1), (300, 7, 2), (1, 2, 3)], 'S65': [(200, 65, 4)], 'S130': [(150, 130, 5)]}


def make_rec(T, S, seed):
    from vbx_amd.synth import make_recording
    X, Phi, _ = make_recording(T, S, D=D_BATCH, seed=seed, kappa=0.05)
    g0 = np.random.default_rng(seed + 100).gamma(1.0, size=(T, S))
    return np.ascontiguousarray(X, dtype=np.float64), Phi, g0 / g0.sum(1, keepdims=True)


def host_log_p(X, Phi, alpha, invL, Fa):
    """log_p_ of VBx.py:97 in float64 (G included: a per-frame shift, which the path does not see)."""
    rho = X * np.sqrt(Phi)
    G = -0.5 * (np.sum(X ** 2, axis=1, keepdims=True) + X.shape[1] * np.log(2 * np.pi))
    return Fa * (rho.dot(alpha.T) - 0.5 * (invL + alpha ** 2).dot(Phi) + G)


def second_of(gamma, first):
    """numpy on the returned responsibilities with the path masked out: the lowest index among equals; -1 for one speaker."""
    if gamma.shape[1] == 1:
        return np.full(len(gamma), -1)
    g = gamma.copy()
    g[np.arange(len(g)), first] = -np.inf
    return np.argmax(g, axis=1)


def run_batch(ctx, recs, n_iters, precision='fp64', streams=0, shared=False):
    """-> per recording (result dict, first, second) after ``n_iters`` iterations.  ``shared``: every recording after the
    first runs on the first one's x-vectors (vbx_batch_set_recording_shared; the recordings then have one T)."""
    from vbx_amd import _capi
    batch = _capi.Batch(ctx, [r[0].shape[0] for r in recs], [r[2].shape[1] for r in recs], D_BATCH, precision=precision,
                        max_iters=n_iters, streams=streams)
    try:
        for j, (X, Phi, g0) in enumerate(recs):
            pi = np.full(g0.shape[1], 1.0 / g0.shape[1])
            if shared and j:
                batch.set_recording_shared(j, 0, pi, g0, HYPER['loopProb'], HYPER['Fa'], HYPER['Fb'])
            else:
                batch.set_recording(j, X, Phi, pi, g0, HYPER['loopProb'], HYPER['Fa'], HYPER['Fb'])
        batch.run(n_iters, -1e300)
        out = []
        for j in range(len(recs)):
            res = batch.result(j)
            first, second = batch.path(j)
            out.append((res, first, second))
        return out
    finally:
        batch.close()


def check_against_referee(recs, before, after):
    """``after`` (n iterations) decodes the model of its last E-step: alpha / invL of that iteration, the priors ``before``
    (n - 1 iterations) ended with."""
    for (X, Phi, _g0), (res0, _f0, _s0), (res, first, second) in zip(recs, before, after):
        assert res0['n_iters'] == N_ITERS - 1 and res['n_iters'] == N_ITERS
        lls = host_log_p(X, Phi, res['alpha'], res['invL'], HYPER['Fa'])
        want, _logp, margin = vr.structured(lls, HYPER['loopProb'], res0['pi'])
        print(f'T={X.shape[0]} S={res0["pi"].shape[0]}: margin {float(margin):.3e}')
        assert margin > MARGIN, float(margin)
        assert np.array_equal(first, want), int(np.argmax(first != want))
        want2 = second_of(res['gamma'], first)
        assert (second is None and want2[0] == -1) or np.array_equal(second, want2)


@pytest.mark.parametrize('name', list(BATCHES))
def test_batch_path_is_the_referees_on_the_model_of_the_last_e_step(name, ctx):
    recs = [make_rec(*r) for r in BATCHES[name]]
    before = run_batch(ctx, recs, N_ITERS - 1)
    after = run_batch(ctx, recs, N_ITERS)
    check_against_referee(recs, before, after)


def test_batch_path_of_a_recording_that_shares_its_x_vectors(ctx):
    base = make_rec(300, 7, 2)
    other = (base[0], base[1], make_rec(300, 7, 9)[2])        # the same x-vectors from another start
    recs = [base, other]
    before = run_batch(ctx, recs, N_ITERS - 1, shared=True)
    after = run_batch(ctx, recs, N_ITERS, shared=True)
    check_against_referee(recs, before, after)


def test_batch_path_in_a_two_stream_group(ctx):
    from vbx_amd import _capi
    recs = [make_rec(*r) for r in [(65, 3, 1), (300, 7, 2), (129, 5, 6), (200, 4, 7)]]
    probe = _capi.Batch(ctx, [r[0].shape[0] for r in recs], [r[2].shape[1] for r in recs], D_BATCH, precision='fp64', max_iters=1,
                        streams=2)
    try:
        groups = {probe.stream_of(j) for j in range(len(recs))}
    finally:
        probe.close()
    assert groups == {0, 1}, groups                           # (an explicit stream count is taken at these sizes)
    before = run_batch(ctx, recs, N_ITERS - 1, streams=2)
    after = run_batch(ctx, recs, N_ITERS, streams=2)
    check_against_referee(recs, before, after)


def test_python_entries_append_the_path_last(ctx):
    from vbx_amd.VBx import VBx
    from vbx_amd.batch import VBx_batch, VBx_sweep
    X, Phi, g0 = make_rec(300, 7, 2)
    kw = dict(pi=7, gamma=g0, maxIters=N_ITERS, epsilon=-1e300, precision='fp64', **HYPER)
    plain = VBx(X, Phi, **kw)
    out = VBx(X, Phi, return_model=True, return_path=True, **kw)
    assert len(plain) == 3 and len(out) == 6 and np.array_equal(out[0], plain[0])
    recs = [make_rec(300, 7, 2)]
    after = run_batch(ctx, recs, N_ITERS)
    assert np.array_equal(out[5], after[0][1])
    b = VBx_batch([dict(X=X, Phi=Phi, pi=7, gamma=g0, **HYPER)], maxIters=N_ITERS, epsilon=-1e300, precision='fp64', return_path=True)
    assert len(b[0]) == 4 and np.array_equal(b[0][3], out[5])
    s = VBx_sweep(X, Phi, [dict(pi=7, gamma=g0, **HYPER)], maxIters=N_ITERS, epsilon=-1e300, precision='fp64', return_path=True)
    assert len(s[0]) == 4 and np.array_equal(s[0][3], out[5])
    for call in (lambda: VBx(X, Phi, return_path=True, **dict(kw, maxIters=0)),
                 lambda: VBx_batch([dict(X=X, Phi=Phi, pi=7, gamma=g0)], maxIters=0, return_path=True),
                 lambda: VBx_sweep(X, Phi, [dict(pi=7, gamma=g0)], maxIters=0, return_path=True)):
        with pytest.raises(ValueError, match='E-step'):
            call()


# ---- fp32: the path scores within the model's own error of the optimum -------------------------------------------------
K_FLOOR = 4                                                   # the margin tests/test_gpu_onestep.py gives its floors
WINDOW = 36.84                                                # 2 |log eps|: below that a state is never on the best path


@pytest.mark.parametrize('precision', ['fp32', 'fp32-split'])
def test_fp32_path_scores_within_the_measured_error_of_the_optimum(precision, ctx):
    """S_ref(device path) >= S_ref(referee path) - K 2 T e.  e is measured: the largest difference, after subtracting each
    frame's maximum and over entries within 36.84 of it, between vbx_loglik in fp32 and numpy float64 on the same model.
    Largest gap / bound measured when the test was written: see DESIGN section 26."""
    worst = 0.0
    for T, S, seed in [(65, 3, 1), (300, 7, 2), (1, 2, 3)]:
        recs = [make_rec(T, S, seed)]
        X, Phi, _ = recs[0]
        before = run_batch(ctx, recs, N_ITERS - 1, precision=precision)
        after = run_batch(ctx, recs, N_ITERS, precision=precision)
        res0, res, first = before[0][0], after[0][0], after[0][1]
        assert res0['n_iters'] == N_ITERS - 1 and res['n_iters'] == N_ITERS
        lls = host_log_p(X, Phi, res['alpha'], res['invL'], HYPER['Fa'])
        dev = ctx.loglik(X, Phi, res['alpha'], res['invL'], HYPER['Fa'], precision='fp32')
        a, b = lls - lls.max(1, keepdims=True), dev - dev.max(1, keepdims=True)
        near = (a >= -WINDOW) | (b >= -WINDOW)
        e = float(np.abs(a - b)[near].max())
        want, _logp, _margin = vr.structured(lls, HYPER['loopProb'], res0['pi'])
        gap = float(vr.score(want, lls, HYPER['loopProb'], res0['pi']) - vr.score(first, lls, HYPER['loopProb'], res0['pi']))
        bound = K_FLOOR * 2 * T * e
        print(f'{precision} T={T} S={S}: e = {e:.3e}, gap {gap:.3e}, bound {bound:.3e}, gap / bound {gap / bound if bound else 0.0:.3e}, '
              f'labels that differ: {int(np.count_nonzero(first != want))}')
        assert gap <= bound, (T, S, gap, bound)
        worst = max(worst, gap / bound if bound else 0.0)
    print(f'{precision}: largest gap / bound {worst:.3e}')


# ---- the driver ------------------------------------------------------------------------------------------------------
REPO = tu.REPO
ENV = dict(os.environ, PYTHONPATH=REPO)
DRIVER = ['--init', 'AHC+VB', '--Fa', '0.3', '--Fb', '17', '--loopP', '0.99']


def run_vbhmm(paths, out, extra):
    argv = [a for a in tu.data_argv(paths) if a not in ('--ref-rttm-dir', paths['ref'])]
    done = subprocess.run([sys.executable, '-m', 'vbx_amd.vbhmm', '--out-rttm-dir', out] + argv + DRIVER + extra, cwd=REPO, env=ENV,
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    return {f: open(os.path.join(out, f), 'rb').read() for f in sorted(os.listdir(out))}


def test_vbhmm_writes_the_referees_path_and_posterior_is_todays_bytes(tmp_path):
    """``--decode viterbi`` in a fresh process writes the RTTM files of ``merge_adjacent_labels`` over the referee's path on
    log_p_ recomputed on the host from the model of the last iteration; ``--decode posterior`` writes what no flag writes."""
    import argparse
    from scipy.special import softmax
    from oracle import vbx_oracle
    from vbx_amd import vbhmm
    from vbx_amd.kaldi_formats import read_xvector_timing_dict
    paths = tu.make_dev_set(tmp_path, 2, 150, seed=3)
    plain = run_vbhmm(paths, str(tmp_path / 'plain'), [])
    assert run_vbhmm(paths, str(tmp_path / 'posterior'), ['--decode', 'posterior']) == plain and len(plain) == 2
    got = run_vbhmm(paths, str(tmp_path / 'viterbi'), ['--decode', 'viterbi'])

    # the same run in this process, on stages that keep what the referee needs: the AHC labels and the last model
    class Keep(vbhmm.DeviceStages):
        def vb(self, ks, labels, *a, **k):
            self.ahc_labels = dict(zip(ks, labels))
            return super().vb(ks, labels, *a, **k)

        def _read_out(self, batch, decode):
            read = super()._read_out(batch, decode)
            self.results = getattr(self, 'results', [])

            def keep(b):
                self.results.append(batch.result(b))
                return read(b)
            return keep

        def close(self):
            self.fea = [self.xv.get('fea', self.row0[k], self.T[k]) for k in range(len(self.T))]
            super().close()
    args = argparse.Namespace(init='AHC+VB', threshold=-0.015, lda_dim=128, Fa=0.3, Fb=17.0, loopP=0.99, init_smoothing=5.0,
                              output_2nd=False, out_rttm_dir=None, xvec_ark_file=paths['ark'], segments_file=paths['seg'],
                              xvec_transform=paths['transform'], plda_file=paths['plda'], decode='viterbi', random_restarts=None,
                              seed=None, init_rttm_dir=None)
    stages = Keep()
    try:
        state, _ = vbhmm.diarize(args, stages=stages, log=lambda *_: None)
    finally:
        stages.close()
    segs = read_xvector_timing_dict(paths['seg'])
    assert len(stages.results) == 2 and all(r['pi'].shape[0] <= 16 for r in stages.results)    # (one batch: in archive order)
    for k, name in enumerate(paths['names']):
        res, lab, fea = stages.results[k], stages.ahc_labels[k], stages.fea[k]
        S = int(lab.max()) + 1
        q = np.zeros((len(lab), S))
        q[np.arange(len(lab)), lab] = 1.0
        q = softmax(q * 5.0, axis=1)
        n = res['n_iters']
        pi_prev = np.full(S, 1.0 / S) if n == 1 else vbx_oracle.VBx(fea, stages.Phi, loopProb=0.99, Fa=0.3, Fb=17.0, pi=S, gamma=q,
                                                                      maxIters=n - 1, epsilon=-1e300)[1]
        lls = host_log_p(fea, stages.Phi, res['alpha'], res['invL'], 0.3)
        want, _logp, margin = vr.structured(lls, 0.99, pi_prev)
        print(f'{name}: S={S}, {n} iterations, margin {float(margin):.3e}')
        assert margin > MARGIN and np.array_equal(state[name]['labels1st'], want)
        start, end = segs[name][1].T
        b, e, s = vbhmm.merge_adjacent_labels(start, end, want)
        import io
        text = io.StringIO()
        vbhmm.write_rttm(text, name, s, b, e)
        assert got[name + '.rttm'] == text.getvalue().encode(), name
