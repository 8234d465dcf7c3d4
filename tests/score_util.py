"""Shared by the tests of ``vbx_amd.score``: the rounding bound a float64 scorer is held to against the exact referee
(``tests/score_ref.py``), and random turns with millisecond decimals, as RTTM files have."""
from fractions import Fraction

import numpy as np

KEYS = ('ref_time', 'miss', 'fa', 'confusion')


def rounding_bound(exact):
    """2 n 2^-53 sum(w): n additions in float64 of terms that sum to at most sum(w) (the scored length), doubled for the
    conversion of the decimal inputs to float64."""
    return 2 * exact['n_cells'] * 2.0 ** -53 * float(exact['scored'])


def assert_within_bound(got, exact, what=''):
    """every quantity of a record of score_turns within the rounding bound of the referee's; the DER within what that allows"""
    bound = rounding_bound(exact)
    for key in KEYS:
        err = abs(Fraction(got[key]) - exact[key])
        print(f'{what} {key}: got {got[key]!r}, error {float(err):.3e}, bound {bound:.3e}')
        assert err <= bound, (what, key)
    names = {(r, s): got['C'][i, j] for i, r in enumerate(got['ref_speakers']) for j, s in enumerate(got['sys_speakers'])}
    assert set(names) == set(exact['C'])
    for key, v in exact['C'].items():
        assert abs(Fraction(float(names[key])) - v) <= bound, (what, key)
    if exact['der'] is None:
        assert np.isnan(got['der'])
    else:
        # d DER = 100 (d err - err / ref d ref) / ref with |d err| <= 3 bound, |d ref| <= bound, err / ref = DER / 100
        slack = 100.0 * (3 * bound + float(exact['der']) / 100.0 * bound) / float(exact['ref_time']) + 1e-13 * float(exact['der'])
        print(f'{what} der: got {got["der"]!r}, exact {float(exact["der"])!r}, slack {slack:.3e}')
        assert abs(got['der'] - float(exact['der'])) <= slack, what


def random_pair(seed, n_ref, n_sys, n_turns, seconds=60):
    """turns with millisecond decimals, as RTTM files have: (float turns, Fraction turns) of either side"""
    rng = np.random.default_rng(seed)

    def side(n_spk, tag):
        fl, ex = [], []
        for _ in range(n_turns):
            start, dur = f'{rng.integers(0, seconds * 1000) / 1000:.3f}', f'{rng.integers(0, 4000) / 1000:.3f}'
            spk = f'{tag}{rng.integers(n_spk)}'
            fl.append((float(start), float(start) + float(dur), spk))
            ex.append((Fraction(start), Fraction(start) + Fraction(dur), spk))
        return fl, ex
    return side(n_ref, 'r'), side(n_sys, 's')
