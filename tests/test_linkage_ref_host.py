"""The numpy referee of the device linkage (tests/linkage_ref.py) against SciPy, on the CPU: for every crafted input of
tests/test_gpu_linkage.py the model of the rounds gives SciPy's tree, the input does what it exists for (its round log),
and check_dendrogram has teeth: two faulty models fail it."""
import numpy as np
import pytest
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import squareform

import linkage_ref as R

# (builder, sizes, largest model-vs-SciPy height error in ulp that the input is known for, or None)
SPEAKERS = {35: lambda n: R.cosine(R.speaker_xvectors(n, 0.35)), 5: lambda n: R.cosine(R.speaker_xvectors(n, 0.05))}
CASES = [('example', lambda n: R.cosine(R.example_xvectors(n)), (255, 256, 257, 300, 511, 512, 513, 1023)),
         ('random', lambda n: R.cosine(R.random_xvectors(n)), (256, 600, 700, 2049)),
         ('speakers35', SPEAKERS[35], (256, 600, 700)),
         ('speakers05', SPEAKERS[5], (256, 600, 640, 700)),
         ('pairing', R.perfect_pairing, (256, 384, 392, 512, 1000, 2050)),
         ('growing', R.growing_staircase, (400,)),
         ('shrinking', R.shrinking_staircase, (500,))]
ULP = {('example', n): 3 for n in CASES[0][2]}
ULP.update({('random', 256): 12, ('random', 600): 12, ('speakers05', 640): 9})
_cache = {}


def scipy_tree(S):
    return linkage(squareform(-S, checks=False), 'average')


def case(kind, n):
    """(S, SciPy's Z, the model's Z, round log, chain statistics), computed once"""
    if (kind, n) not in _cache:
        S = dict((c[0], c[1]) for c in CASES)[kind](n)
        assert np.array_equal(S, S.T) and S.dtype == np.float64
        stats = {}
        Z, log = R.rounds_model(S, stats=stats)
        _cache[kind, n] = (S, scipy_tree(S), Z, log, stats)
    return _cache[kind, n]


@pytest.mark.parametrize('kind,n', [(c[0], n) for c in CASES for n in c[2]])
def test_the_model_of_the_rounds_gives_scipys_tree(kind, n):
    """Columns 0, 1, 3 identical to linkage(squareform(-S), 'average'), all heights of that tree distinct, heights within
    the shared bounds (against SciPy and against the exact means), and within the ulp figure the input is listed with."""
    S, Zs, Z, log, _ = case(kind, n)
    assert np.all(np.diff(Zs[:, 2]) > 0), 'tied heights'
    out = R.check_dendrogram(S, Z, Zs, label=f'{kind} model')
    if (kind, n) in ULP:
        assert out['ulp_vs_ref'] <= ULP[kind, n], out


def test_the_example_recording_runs_rounds_from_256_clusters_on():
    assert case('example', 255)[3] == []                                  # the chain alone
    for n in CASES[0][2][1:]:
        log = case('example', n)[3]
        assert log and log[0][1] == n and max(p for p, _ in log) > 1, (n, log)
        assert log[-1][1] > 48 and log[-1][1] - log[-1][0] <= 48, (n, log)      # stopped by the count, not by a stall


def test_random_and_clustered_inputs_never_stall():
    for kind in ('random', 'speakers35', 'speakers05'):
        for n in dict((c[0], c[2]) for c in CASES)[kind]:
            log = case(kind, n)[3]
            assert all(p * 64 >= live for p, live in log), (kind, n, log)
            assert log[-1][1] - log[-1][0] <= 48


def test_perfect_pairing_halves_the_live_clusters_every_round():
    for n in (256, 384, 392, 512, 1000, 2050):
        log = case('pairing', n)[3]
        assert log[0] == (n // 2, n), (n, log)                            # d_pairs filled to its last slot but one
    assert case('pairing', 384)[3] == [(192, 384), (96, 192), (48, 96)]   # exactly 48 left: the rounds stop
    assert case('pairing', 384)[4]['chain_clusters'] == 48
    assert case('pairing', 392)[3] == [(196, 392), (98, 196), (49, 98), (24, 49)]      # 49 left: one more round
    assert case('pairing', 392)[4]['chain_clusters'] == 25
    assert case('pairing', 2050)[3][0][0] == 1025                         # three blocks of rnn_pairs, a carry of 1024 + 1


def test_the_staircases_stall_and_leave_the_chain_nearly_everything():
    for kind, n in (('growing', 400), ('shrinking', 500)):
        _, _, _, log, stats = case(kind, n)
        assert log == [(1, n), (1, n - 1), (1, n - 2)] and all(p * 64 < live for p, live in log)
        assert stats['chain_clusters'] == n - 3
    # at 8200 the chain gets 8197 >= 8192 clusters: stages, one compaction in between (rounds only: the chain is SciPy's)
    stats = {}
    _, log = R.rounds_model(R.growing_staircase(8200), chain_too=False, stats=stats)
    assert log == [(1, 8200), (1, 8199), (1, 8198)] and stats['chain_clusters'] == 8197


def test_the_shrinking_staircase_grows_a_chain_of_all_points():
    stats = {}
    S = R.shrinking_staircase(500)
    Z, log = R.rounds_model(S, rounds_from=10 ** 9, stats=stats)           # the chain form
    assert log == [] and stats['max_chain'] == 500
    assert np.array_equal(Z, scipy_tree(S))
    assert case('shrinking', 500)[4]['max_chain'] >= 490                   # ... and after the three stalled rounds
    # 8200 points: every gap positive and distinct, every point's nearest neighbour the right-hand one -> the chain that
    # starts at point 0 reaches the last point before its first merge, and is still long at the first stage boundary
    p = -R.shrinking_staircase(8200)[0]
    gaps = np.diff(p)
    assert gaps.min() > 1 and np.all(np.diff(gaps) < 0)


def test_the_constant_matrix_stalls_and_stays_a_valid_dendrogram():
    S = R.constant(300)
    stats = {}
    Z, log = R.rounds_model(S, stats=stats)
    assert log == [(1, 300), (1, 299), (1, 298)] and stats['chain_clusters'] == 297
    R.check_dendrogram(S, Z, scipy_tree(S), distinct=False, label='constant model')
    assert np.all(Z[:, 2] == -0.25)


# ---- teeth ----------------------------------------------------------------------------------------------------------------------
def fails(S, Z, Zs):
    try:
        R.check_dendrogram(S, Z, Zs, label='faulty model')
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('kind,n', [('growing', 400), ('random', 256)])
def test_swapped_sizes_in_the_update_fail_the_check(kind, n):
    """faulty model (a): n_a and n_b swapped in the update"""
    S, Zs, Z, _, _ = case(kind, n)
    assert not fails(S, Z, Zs)
    assert fails(S, R.rounds_model(S, update=R.swapped_update)[0], Zs)


@pytest.mark.parametrize('kind,n', [('growing', 400), ('random', 256)])
def test_highest_index_tie_rule_fails_the_check(kind, n):
    """faulty model (b): the highest index among equals.  Where all distances are distinct no tie rule is ever consulted
    -- the faulty model is the model, bit for bit, and nothing can tell them apart -- so it is shown on the same two
    kinds of input with exact ties that SciPy resolves by its own lowest-index rule: a staircase whose every third point
    lies half-way between its neighbours, and random cosine similarities where two points are both the nearest
    neighbour of point 0, the start of SciPy's chain.  There the model still gives SciPy's tree and the faulty one fails."""
    S = case(kind, n)[0]
    assert np.array_equal(R.rounds_model(S, tie='high')[0], case(kind, n)[2])
    S = R.tied_staircase(n) if kind == 'growing' else R.random_with_a_tie(n)
    Zs = scipy_tree(S)
    assert not fails(S, R.rounds_model(S)[0], Zs)
    assert fails(S, R.rounds_model(S, tie='high')[0], Zs)
