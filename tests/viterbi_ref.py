"""Referee of the Viterbi decode, NumPy longdouble.  Not a test module.

The model is forward_backward's (VBx.py:146-175): tr = loopProb I + (1 - loopProb) 1 pi^T, eps = 1e-8 added to tr and to ip
before the logarithm.  ``structured`` is the recursion the device runs, ``dense`` the textbook max-plus Viterbi on
log(tr + eps), ``brute_force`` the best of all S^T paths; ``score`` is the log-probability of a given path.
"""
import itertools

import numpy as np

EPS = 1e-8
LD = np.longdouble


def _model(loopProb, pi, ip):
    pi = np.asarray(pi, dtype=LD)
    ip = pi if ip is None else np.asarray(ip, dtype=LD)
    lp = LD(loopProb)
    move = np.log((1 - lp) * pi + LD(EPS))
    stay = np.log(lp + (1 - lp) * pi + LD(EPS))
    return stay, move, np.log(ip + LD(EPS))


def structured(lls, loopProb, pi, ip=None, own_state=True):
    """(path int64 [T], logp, margin).  margin: the smallest, over the frames, of (a) the gap between the largest and the
    second largest d and (b) min_j |d(j) - m + stay_j - move_j| -- how far every decision of the recursion is from a tie
    (inf where there is nothing to decide: one state, one frame).  ``own_state=False`` leaves the state a_t itself out of (b):
    whether it "stayed" or "came from a_t" is the same predecessor, and with loopProb = 0 the two score the same by
    construction (stay_j = move_j)."""
    with np.errstate(invalid='ignore', divide='ignore'):
        lls = np.asarray(lls, dtype=LD)
        T, S = lls.shape
        stay, move, lip = _model(loopProb, pi, ip)
        d = lls[0] + lip
        stayed = np.zeros((T, S), dtype=bool)
        came = np.zeros(T, dtype=np.int64)
        total = LD(0)
        margin = LD(np.inf)

        def top_gap(v):
            if S < 2:
                return LD(np.inf)
            two = np.partition(v, S - 2)[S - 2:]
            g = two[1] - two[0]
            return g if np.isfinite(g) else LD(np.inf)

        for t in range(1, T):
            a = int(np.argmax(d))                     # (the first among equals)
            m = d[a]
            margin = min(margin, top_gap(d))
            sv = d - m + stay
            diff = np.abs(sv - move)
            if not own_state:
                diff[a] = np.inf
            diff = diff[np.isfinite(diff)]
            if diff.size:
                margin = min(margin, diff.min())
            stayed[t] = sv >= move
            came[t] = a
            total += m
            d = lls[t] + np.where(stayed[t], sv, move)
        margin = min(margin, top_gap(d))
        path = np.zeros(T, dtype=np.int64)
        path[T - 1] = int(np.argmax(d))
        logp = total + d[path[T - 1]]
        for t in range(T - 1, 0, -1):
            path[t - 1] = path[t] if stayed[t, path[t]] else came[t]
        return path, logp, margin


def log_transitions(loopProb, pi):
    pi = np.asarray(pi, dtype=LD)
    S = len(pi)
    tr = LD(loopProb) * np.eye(S, dtype=LD) + (1 - LD(loopProb)) * np.tile(pi, (S, 1))
    return np.log(tr + LD(EPS))


def dense(lls, loopProb, pi, ip=None):
    """(path, logp) of the max-plus recursion on the full S x S matrix; the first index among equals everywhere."""
    with np.errstate(invalid='ignore', divide='ignore'):
        lls = np.asarray(lls, dtype=LD)
        T, S = lls.shape
        ltr = log_transitions(loopProb, pi)
        lip = _model(loopProb, pi, ip)[2]
        d = lls[0] + lip
        back = np.zeros((T, S), dtype=np.int64)
        for t in range(1, T):
            cand = d[:, None] + ltr
            back[t] = np.argmax(cand, axis=0)
            d = lls[t] + cand[back[t], np.arange(S)]
        path = np.zeros(T, dtype=np.int64)
        path[T - 1] = int(np.argmax(d))
        for t in range(T - 1, 0, -1):
            path[t - 1] = back[t, path[t]]
        return path, d[path[T - 1]]


def score(path, lls, loopProb, pi, ip=None):
    """log-probability of ``path`` (longdouble)."""
    with np.errstate(invalid='ignore', divide='ignore'):
        lls = np.asarray(lls, dtype=LD)
        path = np.asarray(path, dtype=np.int64)
        T = len(path)
        ltr = log_transitions(loopProb, pi)
        lip = _model(loopProb, pi, ip)[2]
        return lip[path[0]] + lls[np.arange(T), path].sum() + ltr[path[:-1], path[1:]].sum()


def brute_force(lls, loopProb, pi, ip=None):
    """(best score, every path that attains it to 1e-15) over all S^T paths."""
    lls = np.asarray(lls, dtype=LD)
    T, S = lls.shape
    best, arg = None, []
    for q in itertools.product(range(S), repeat=T):
        v = score(q, lls, loopProb, pi, ip)
        if best is None or v > best + LD(1e-15):
            best, arg = v, [q]
        elif abs(v - best) <= LD(1e-15):
            arg.append(q)
    return best, arg


def draw(seed, T, S, sigma=5.0):
    """The random case of the tests: lls ~ N(0, sigma^2), pi ~ Dirichlet(1)."""
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, sigma, size=(T, S)), rng.dirichlet(np.ones(S))
