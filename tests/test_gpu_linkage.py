"""The device average linkage as it runs by default (vbx_scores_linkage_average, vbx_ahc.hpp): rounds of reciprocal
pairs from 256 clusters on, the hand-over to the chain at 48 live clusters with the compaction in front of it, the exit
after three stalled rounds, the staged chain behind it, and a long live chain carried across a compaction.

Every matrix goes up through _capi.Scores.upload (crafted) or _capi.Scores.cos_similarity (x-vectors); the reference is
scipy.cluster.hierarchy.linkage on the condensed negated matrix read back from the device -- the very bits it holds -- and
the exact mean pairwise distances in np.longdouble (tests/linkage_ref.py, where the assertions are stated).  That every
input does what it is here for -- stalls, stops at exactly 48, fills the pair list -- is asserted on the CPU in
tests/test_linkage_ref_host.py."""
import numpy as np
import pytest
from scipy.cluster.hierarchy import linkage

import linkage_ref as R

pytestmark = pytest.mark.gpu

XVECTORS = {'example': R.example_xvectors, 'random': R.random_xvectors,
            'speakers35': lambda n: R.speaker_xvectors(n, 0.35), 'speakers05': lambda n: R.speaker_xvectors(n, 0.05)}
CRAFTED = {'pairing': R.perfect_pairing, 'growing': R.growing_staircase, 'shrinking': R.shrinking_staircase}
BROAD = (256, 600, 700, 2047, 2048, 2049)                    # (the last three straddle rnn_rowmin's 8 x 256 stride)
CASES = ([('example', n) for n in (255, 256, 257, 300, 511, 512, 513, 1023)] + [('random', n) for n in BROAD] +
         [('speakers35', n) for n in BROAD] + [('speakers05', n) for n in BROAD + (640,)] +
         [('pairing', n) for n in (256, 384, 392, 512, 1000, 2050)] + [('growing', 400), ('growing', 8200), ('shrinking', 500),
                                                                      ('shrinking', 8200)])


def run_device(monkeypatch, kind, n, form=None, S=None):
    """(S as the device holds it, the condensed negated matrix, the device's Z) in the default form or the one forced"""
    from vbx_amd import _capi
    if form is None:
        monkeypatch.delenv('VBX_AMD_EXPERIMENT', raising=False)
        monkeypatch.delenv('VBX_AMD_LINKAGE_DEVICE', raising=False)
    else:
        monkeypatch.setenv('VBX_AMD_EXPERIMENT', '1')
        monkeypatch.setenv('VBX_AMD_LINKAGE_DEVICE', form)
    ctx = _capi.default_context()
    if kind in XVECTORS:
        sc = _capi.Scores.cos_similarity(ctx, XVECTORS[kind](n))
    else:
        S = CRAFTED[kind](n) if S is None else S
        sc = _capi.Scores.upload(ctx, S)
    try:
        cond = sc.get_condensed(n, -1.0)
        if kind in XVECTORS:
            full = sc.get().reshape(n, n)
            S = np.triu(full) + np.triu(full, 1).T                         # (the triangle the condensed form is taken from)
        Z = sc.linkage_average(n)
    finally:
        sc.close()
    return S, cond, Z


@pytest.mark.parametrize('kind,n', CASES)
def test_default_linkage_gives_scipys_tree_and_exact_heights(kind, n, monkeypatch):
    """check_dendrogram against SciPy on the device's own bits (same tree, same flat clusters, heights within
    max(16 ulp, 1e-15 max|S|) and within 4 u depth max|S| of the exact means, SciPy held to the same), then the heights
    against the host routine and the chain form of the device; below 256 clusters the default IS the chain, bit for bit.
    The growing staircase of 8200 has seven pairs of exactly equal heights in SciPy's own tree (equal means of arithmetic
    progressions in disjoint subtrees); every other reference tree here has distinct heights, asserted."""
    from vbx_amd import _capi
    S, cond, Z = run_device(monkeypatch, kind, n)
    Zs = linkage(cond, 'average')
    if (kind, n) != ('growing', 8200):
        assert np.all(np.diff(Zs[:, 2]) > 0), 'tied heights: the input is wrong'
    R.check_dendrogram(S, Z, Zs, label=f'{kind} device')
    Zh = _capi.linkage_average(cond)
    _, _, Zc = run_device(monkeypatch, kind, n, form='chain', S=S)
    smax = np.abs(S).max()
    print('  ulp against the host routine, the chain form:', R.check_heights(smax, Z, Zh, 'host'), R.check_heights(smax, Z, Zc, 'chain'))
    assert np.array_equal(Zc, Zh) and np.array_equal(np.signbit(Zc), np.signbit(Zh))
    if n < 256:
        assert np.array_equal(Z, Zh) and np.array_equal(np.signbit(Z), np.signbit(Zh))
    if n <= 2050:
        # the numpy model does the device's operations on the device's numbers in the device's order: the same bits
        assert np.array_equal(Z, R.rounds_model(S)[0]), 'the device and its numpy model disagree'


@pytest.mark.parametrize('kind,n', [('tied_staircase', 400), ('random_with_a_tie', 256)])
def test_exact_ties_that_scipy_resolves_by_the_lowest_index(kind, n, monkeypatch):
    """The two inputs on which a highest-index tie rule fails the check (tests/test_linkage_ref_host.py): the device's
    lowest-index rule gives SciPy's tree on them, and the bits of its numpy model."""
    S = R.tied_staircase(n) if kind == 'tied_staircase' else R.random_with_a_tie(n)
    _, cond, Z = run_device(monkeypatch, kind, n, S=S)
    R.check_dendrogram(S, Z, linkage(cond, 'average'), label=f'{kind} device')
    assert np.array_equal(Z, R.rounds_model(S)[0])


def test_long_live_chain_across_the_stage_boundary(monkeypatch):
    """The shrinking staircase of 8200 in the chain form: the chain holds every point before its first merge and is still
    some 4000 long when linkage_compact_index_kernel re-indexes it after the first stage of 2050 merges."""
    from vbx_amd import _capi
    S, cond, Z = run_device(monkeypatch, 'shrinking', 8200, form='chain')
    Zh = _capi.linkage_average(cond)
    assert np.array_equal(Z, Zh) and np.array_equal(np.signbit(Z), np.signbit(Zh))
    R.check_dendrogram(S, Z, linkage(cond, 'average'), label='shrinking chain form')


def test_constant_matrix_is_a_valid_dendrogram_at_one_height(monkeypatch):
    """All similarities 0.25: every nearest neighbour is a tie, the rounds merge one pair each and stall, the chain does
    the rest.  Valid, every height within 4 u depth |c| of -c, all singletons below it and one cluster above."""
    from vbx_amd import _capi
    T, c = 300, 0.25
    monkeypatch.delenv('VBX_AMD_EXPERIMENT', raising=False)
    monkeypatch.delenv('VBX_AMD_LINKAGE_DEVICE', raising=False)
    sc = _capi.Scores.upload(_capi.default_context(), R.constant(T, c))
    Z = sc.linkage_average(T)
    sc.close()
    R.check_valid(Z, T)
    assert np.all(np.abs(Z[:, 2] + c) <= 4 * R.U * R.node_depths(Z) * abs(c))
    assert len(set(_capi.fcluster_distance(Z, -c - 0.01).tolist())) == T
    assert len(set(_capi.fcluster_distance(Z, -c + 0.01).tolist())) == 1


@pytest.mark.parametrize('kind,n', [('pairing', 384), ('growing', 400)])
def test_default_linkage_is_deterministic(kind, n, monkeypatch):
    first = run_device(monkeypatch, kind, n)[2]
    again = run_device(monkeypatch, kind, n)[2]
    assert first.tobytes() == again.tobytes()
